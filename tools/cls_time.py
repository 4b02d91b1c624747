#!/usr/bin/env python3
"""Classification graphs on one GPU, fp16: yolo11n-cls and yolo11s-cls at 224 x 224 (the reference's default size), batch 1 and 64,
nc = 1000.  Per-op device times of one forward (YoloEngine.profile -> bsy_plan_profile: HIP events around every op, serial), the
head's four ops (1x1 Conv to 1280 channels, global mean, linear, softmax / top-k tail) and the forward's wall time and images/s.  One
warm-up forward (it also tunes the conv configurations), then the median of --runs profiles and of --runs timed windows of 50 forwards
each.  Synthetic weights (weights.synth_state_dict); prints a table and one JSON line.

    python tools/cls_time.py [--runs 7] [--out FILE.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bs_yolo_amd.engine import YoloEngine  # noqa: E402
from bs_yolo_amd.graphs import stock_cfg  # noqa: E402
from bs_yolo_amd.plan import Plan  # noqa: E402
from bs_yolo_amd.weights import synth_state_dict  # noqa: E402

DEV = "cuda:0"
NC, SIZE = 1000, 224
FWD_PER_WINDOW = 50
CASES = [("yolo11n-cls", "n", 1), ("yolo11n-cls", "n", 64), ("yolo11s-cls", "s", 1), ("yolo11s-cls", "s", 64)]


def wall_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(cfg, sd, x, runs):
    eng = YoloEngine(cfg, sd)
    eng(x)  # warm-up: builds the plan, tunes the convs
    torch.cuda.synchronize()
    profs = []
    for _ in range(runs):
        ops, plan = eng.profile(x)
        profs.append([t for _, _, t in ops])
    names = [n for n, _, _ in ops]
    med = [statistics.median(p[i] for p in profs) for i in range(len(names))]
    head = f"model.{plan.meta['n_layers'] - 1}."
    head_ops = [[n[len(head):], round(t, 4)] for n, t in zip(names, med) if n.startswith(head)]

    def burst():  # a single forward is a fraction of a millisecond: time FWD_PER_WINDOW of them between one pair of events
        for _ in range(FWD_PER_WINDOW):
            eng(x)

    fwd = statistics.median(wall_ms(burst) for _ in range(runs)) / FWD_PER_WINDOW
    eng.close()
    return {"ops": len(names), "sum_ops_ms": round(sum(med), 4), "head_ops_ms": head_ops, "forward_ms": round(fwd, 4),
            "images_per_s": round(x.shape[0] / fwd * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"workload": f"fp16, {SIZE} x {SIZE}, nc {NC}, synthetic weights; per-op times from YoloEngine.profile, forward_ms = a window of "
           f"{FWD_PER_WINDOW} forwards / {FWD_PER_WINDOW}", "runs": a.runs, "cases": []}
    print(f"{'graph':12s} {'B':>3s} {'ops':>4s} {'sum ops ms':>10s} {'forward ms':>10s} {'images/s':>9s}  head ops (ms)")
    for tag, scale, B in CASES:
        cfg = stock_cfg("yolo11", scale, NC, "classify")
        sd = synth_state_dict(Plan(cfg, 1, 64, 64), 0)
        x = torch.rand(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(0)).half().to(DEV)
        r = measure(cfg, sd, x, a.runs)
        r.update(graph=tag, batch=B)
        res["cases"].append(r)
        print(f"{tag:12s} {B:3d} {r['ops']:4d} {r['sum_ops_ms']:10.4f} {r['forward_ms']:10.4f} {r['images_per_s']:9.1f}  "
              + "  ".join(f"{n} {t:.4f}" for n, t in r["head_ops_ms"]), flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
