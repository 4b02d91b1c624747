#!/usr/bin/env python3
"""Pose graphs on one GPU, fp16: yolo11n-pose and yolo11s-pose (nc = 1, 17 x 3 keypoints) at 640 x 640, batch 64, beside the detect
graph of the same scale (nc = 1) on the same build -- what the three cv4 branches and the keypoint rows of the decode launch cost
over detect.  Three engines per scale: the pose plan, the detect plan (fused head, no decode launch) and the detect plan with
fuse_head off (the same decode launch without keypoint rows).  One warm-up forward each (it also tunes the conv configurations),
then --runs rounds that visit the engines in turn (interleaved: drift hits all three alike); per round a window of --fwd forwards
between one pair of events and one per-op profile (YoloEngine.profile -> bsy_plan_profile: HIP events around every op, serial).
Medians over the rounds.  Synthetic weights (weights.synth_state_dict); prints a table and one JSON line.

    python tools/pose_time.py [--runs 7] [--fwd 20] [--batch 64] [--out FILE.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bs_yolo_amd import lib as L  # noqa: E402
from bs_yolo_amd.engine import YoloEngine  # noqa: E402
from bs_yolo_amd.graphs import stock_cfg  # noqa: E402
from bs_yolo_amd.plan import Plan  # noqa: E402
from bs_yolo_amd.weights import synth_state_dict  # noqa: E402

DEV = "cuda:0"
SIZE = 640


def wall_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def engines(scale):
    out = {}
    for key, task, kw in (("pose", "pose", {}), ("detect", "detect", {}), ("detect_unfused", "detect", {"fuse_head": False})):
        cfg = stock_cfg("yolo11", scale, 1, task, kpt_shape=(17, 3))  # (read by the pose task alone)
        out[key] = YoloEngine(cfg, synth_state_dict(Plan(cfg, 1, 64, 64, **kw), 0), **kw)
    return out


def measure(scale, B, runs, fwd):
    x = torch.rand(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(0)).half().to(DEV)
    engs = engines(scale)
    for e in engs.values():
        e(x, want_raw=False)  # warm-up: builds the plan, tunes the convs
    torch.cuda.synchronize()
    wall = {k: [] for k in engs}
    prof = {k: [] for k in engs}
    plans = {}
    for _ in range(runs):
        for k, e in engs.items():
            def burst(e=e):
                for _ in range(fwd):
                    e(x, want_raw=False)
            wall[k].append(wall_ms(burst) / fwd)
        for k, e in engs.items():
            ops, plans[k] = e.profile(x)
            prof[k].append(ops)
    res = {}
    for k, e in engs.items():
        names = [(n, kind) for n, kind, _ in prof[k][0]]
        med = [statistics.median(p[i][2] for p in prof[k]) for i in range(len(names))]
        dec = [t for (n, kind), t in zip(names, med) if kind == L.OP_DECODE]
        cv4 = sum(t for (n, kind), t in zip(names, med) if ".cv4." in n)
        ms = statistics.median(wall[k])
        res[k] = {"launches": len(names), "forward_ms": round(ms, 4), "images_per_s": round(B / ms * 1e3, 1), "sum_ops_ms": round(sum(med), 4),
                  "decode_ms": round(dec[0], 4) if dec else None, "cv4_ms": round(cv4, 4)}
        e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--fwd", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"workload": f"fp16, {SIZE} x {SIZE}, batch {a.batch}, nc 1, kpt_shape (17, 3), synthetic weights, want_raw=False; forward_ms = a window "
           f"of {a.fwd} forwards / {a.fwd}, engines interleaved; per-op times from YoloEngine.profile", "runs": a.runs, "cases": []}
    print(f"{'graph':24s} {'launches':>8s} {'forward ms':>10s} {'images/s':>9s} {'sum ops ms':>10s} {'decode ms':>9s} {'cv4 ms':>8s}")
    for scale in ("n", "s"):
        r = measure(scale, a.batch, a.runs, a.fwd)
        for k, v in r.items():
            v.update(graph=f"yolo11{scale}", plan=k)
            res["cases"].append(v)
            dec = f"{v['decode_ms']:9.4f}" if v["decode_ms"] is not None else f"{'-':>9s}"
            print(f"{'yolo11' + scale + ' ' + k:24s} {v['launches']:8d} {v['forward_ms']:10.4f} {v['images_per_s']:9.1f} {v['sum_ops_ms']:10.4f} "
                  f"{dec} {v['cv4_ms']:8.4f}", flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
