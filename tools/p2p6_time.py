#!/usr/bin/env python3
"""Four-level (P2 / P6) graphs on one GPU, fp16: per-op device times of one forward (YoloEngine.profile: HIP events around every op,
serial) and the forward's wall time, with the fused head (the conv epilogue decodes) and with the decode launch (fuse_head=False),
for yolov8s-p2 at 640 x 640 batch 64, yolov8s-p6 at 1280 x 1280 batch 16, and the three-level yolov8s at both sizes.  One warm-up
forward (it also tunes the conv configurations), then the median of --runs profiles / timed forwards.  Synthetic weights
(weights.synth_state_dict), nc = 80; prints a table and one JSON line.

    python tools/p2p6_time.py [--runs 5] [--top 6] [--out FILE.json]"""
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
CASES = [("yolov8s-p2", "yolov8-p2", 640, 64), ("yolov8s", "yolov8", 640, 64), ("yolov8s-p6", "yolov8-p6", 1280, 16), ("yolov8s", "yolov8", 1280, 16)]


def wall_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(cfg, sd, x, fuse_head, runs, top):
    eng = YoloEngine(cfg, sd, fuse_head=fuse_head)
    eng(x, want_raw=False)  # warm-up: builds the plan, tunes the convs
    torch.cuda.synchronize()
    profs = []
    for _ in range(runs):
        ops, plan = eng.profile(x)
        profs.append([t for _, _, t in ops])
    names = [n for n, _, _ in ops]
    med = [statistics.median(p[i] for p in profs) for i in range(len(names))]
    head = f"model.{plan.meta['n_layers'] - 1}."
    head_ops = sorted(((t, n) for n, t in zip(names, med) if n.startswith(head)), reverse=True)
    fwd = statistics.median(wall_ms(lambda: eng(x, want_raw=False)) for _ in range(runs))
    raw = statistics.median(wall_ms(lambda: eng(x)) for _ in range(runs))
    out = {"ops": len(names), "levels": len(plan.meta["levels"]), "anchors": plan.meta["A"], "sum_ops_ms": round(sum(med), 3),
           "head_ops_ms": round(sum(t for t, _ in head_ops), 3), "forward_ms": round(fwd, 3), "forward_raw_ms": round(raw, 3),
           "slowest_head_ops": [[n, round(t, 3)] for t, n in head_ops[:top]]}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--top", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"workload": "fp16, nc 80, synthetic weights; per-op times from YoloEngine.profile", "runs": a.runs, "cases": []}
    print(f"{'graph':12s} {'size':>5s} {'B':>3s} {'head':8s} {'ops':>4s} {'anchors':>7s} {'sum ops ms':>10s} {'head ops ms':>11s} {'forward ms':>10s} {'+raw maps ms':>12s}")
    for tag, family, size, B in CASES:
        cfg = stock_cfg(family, "s", 80, "detect")
        sd = synth_state_dict(Plan(cfg, 1, 64, 64), 0)
        x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(0)).half().to(DEV)
        for fuse_head in (True, False):
            r = measure(cfg, sd, x, fuse_head, a.runs, a.top)
            r.update(graph=tag, size=size, batch=B, head="fused" if fuse_head else "decode")
            res["cases"].append(r)
            print(f"{tag:12s} {size:5d} {B:3d} {r['head']:8s} {r['ops']:4d} {r['anchors']:7d} {r['sum_ops_ms']:10.3f} {r['head_ops_ms']:11.3f} "
                  f"{r['forward_ms']:10.3f} {r['forward_raw_ms']:12.3f}", flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
