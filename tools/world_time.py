#!/usr/bin/env python3
"""YOLO-World v2 on one GPU, fp16: YOLOv8s-worldv2 beside YOLOv8s (nc = 80) at 640 x 640, batch 64 and batch 1, on the same build -- what the
four C2fAttn blocks (a proj_conv and a max-sigmoid gate each, a wider cv2) and the text-folded head cost over the plain graph -- and the
engine's per-op profile of the four MAXSIG launches at nc = 80 and nc = 1203 (LVIS, the family's usual vocabulary), beside each launch the
bytes it moves: two reads and one write of its c channels per pixel (the guide is read from the cache).  One warm-up forward per engine
(it also tunes the conv configurations), then --runs rounds that visit the engines in turn (interleaved: drift hits all alike); per round
a window of --fwd forwards between one pair of events and one per-op profile (YoloEngine.profile -> bsy_plan_profile: HIP events around
every op, serial).  Medians over the rounds.  Synthetic weights and text (weights.synth_state_dict); prints a table and one JSON line.

    python tools/world_time.py [--runs 5] [--fwd 10] [--out FILE.json]"""
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


def engines():
    out = {}
    v8 = stock_cfg("yolov8", "s", 80)
    out["yolov8s"] = YoloEngine(v8, synth_state_dict(Plan(v8, 1, 64, 64), 0))
    world = stock_cfg("yolov8-worldv2", "s", 80)
    for nc in (80, 1203):
        out[f"yolov8s-worldv2 nc={nc}"] = YoloEngine(world, synth_state_dict(Plan(world, 1, 64, 64, text_nc=nc), 0))  # (the text rows come with it)
    return out


def measure(B, runs, fwd):
    x = torch.rand(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(0)).half().to(DEV)
    engs = engines()
    for e in engs.values():
        e(x, want_raw=False)  # warm-up: builds the plan, tunes the convs
    torch.cuda.synchronize()
    wall, prof, plans = {k: [] for k in engs}, {k: [] for k in engs}, {}
    for _ in range(runs):
        for k, e in engs.items():
            def burst(e=e):
                for _ in range(fwd):
                    e(x, want_raw=False)
            wall[k].append(wall_ms(burst) / fwd)
        for k, e in engs.items():
            ops, plans[k] = e.profile(x)
            prof[k].append(ops)
    res = []
    for k, e in engs.items():
        names = [(n, kind) for n, kind, _ in prof[k][0]]
        med = [statistics.median(p[i][2] for p in prof[k]) for i in range(len(names))]
        ms = statistics.median(wall[k])
        gates = []
        for o, t in zip(plans[k].ops, med):
            if o["kind"] == L.OP_MAXSIG:
                px, c = B * o["H"] * o["W"], o["src0"].C
                mb = 3 * px * c * 2 / 1e6
                gates.append({"op": o["name"], "map": [o["H"], o["W"]], "c": c, "heads": o["heads"], "nc": o["nc"], "ms": round(t, 4), "MB": round(mb, 2),
                              "GB_per_s": round(mb / t, 1) if t > 0 else None, "TFLOP_per_s": round(2 * px * c * o["nc"] / t / 1e9, 1) if t > 0 else None})
        proj = sum(t for (n, _), t in zip(names, med) if n.endswith(".attn.proj_conv"))
        res.append({"graph": k, "batch": B, "launches": len(names), "forward_ms": round(ms, 4), "images_per_s": round(B / ms * 1e3, 1),
                    "sum_ops_ms": round(sum(med), 4), "maxsig_ms": round(sum(g_["ms"] for g_ in gates), 4), "proj_conv_ms": round(proj, 4), "maxsig": gates})
        e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--fwd", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"workload": f"fp16, {SIZE} x {SIZE}, synthetic weights and text, want_raw=False; forward_ms = a window of {a.fwd} forwards / {a.fwd}, engines "
           "interleaved; per-op times from YoloEngine.profile; MB = two reads and one write of c channels per pixel", "runs": a.runs, "cases": []}
    print(f"{'graph':28s} {'batch':>5s} {'launches':>8s} {'forward ms':>10s} {'images/s':>9s} {'sum ops ms':>10s} {'maxsig ms':>9s} {'proj ms':>8s}")
    for B in (64, 1):
        for v in measure(B, a.runs, a.fwd):
            res["cases"].append(v)
            print(f"{v['graph']:28s} {B:5d} {v['launches']:8d} {v['forward_ms']:10.4f} {v['images_per_s']:9.1f} {v['sum_ops_ms']:10.4f} "
                  f"{v['maxsig_ms']:9.4f} {v['proj_conv_ms']:8.4f}", flush=True)
            for g in v["maxsig"]:
                print(f"    {g['op']:18s} {g['map'][0]:3d} x {g['map'][1]:3d} c {g['c']:4d} heads {g['heads']:2d} nc {g['nc']:5d}: {g['ms']:8.4f} ms  {g['MB']:8.2f} MB  "
                      f"{g['GB_per_s']} GB/s  {g['TFLOP_per_s']} TFLOP/s", flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
