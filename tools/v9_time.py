#!/usr/bin/env python3
"""YOLOv9 on one GPU, fp16.  (1) The two modes of the pooling front end (csrc/pool_down.hip, bsy_pool_down) at every shape
YOLOv9c's ADown blocks give them at batch 32, 640 x 640 -- the views the plan uses (a half of the block's input, ld = 2 C) --
with the achieved GB/s against the bytes they must move (mode 0: read and write H x W x C; mode 1: read H x W x C, write a
quarter of it).  Shapes whose source and destination together fit the 256 MiB Infinity Cache are marked: their rate is not an
HBM rate.  (2) The YOLOv9c and YOLOv9t forwards: wall time (with and without raw maps), the sum of the per-op device times
(YoloEngine.profile) and the pool-down ops' share.  One warm-up (the forward's also tunes the conv configurations), then the
median of --runs.  Synthetic weights (weights.synth_state_dict), nc = 80; prints tables and one JSON line.

    python tools/v9_time.py [--runs 5] [--batch 32] [--size 640] [--out FILE.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bs_yolo_amd import lib as L  # noqa: E402
from bs_yolo_amd import ops as O  # noqa: E402
from bs_yolo_amd.engine import YoloEngine  # noqa: E402
from bs_yolo_amd.graphs import stock_cfg  # noqa: E402
from bs_yolo_amd.plan import Plan  # noqa: E402
from bs_yolo_amd.weights import synth_state_dict  # noqa: E402

DEV = "cuda:0"
CACHE = 256 << 20


def wall_ms(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def pool_cases(B, size):
    """(mode, H, W, C, ld, coff) of every distinct pool-down launch of YOLOv9c's plan."""
    plan = Plan(stock_cfg("yolov9", "c", 80), B, size, size)
    seen = []
    for o in plan.ops:
        if o["kind"] == L.OP_POOL_DOWN:
            c = (o["level"], o["H"], o["W"], o["src0"].C, o["src0"].ld, o["src0"].coff)
            if c not in seen:
                seen.append(c)
    return seen


def time_pool(B, case, runs):
    mode, H, W, C, ld, coff = case
    x = torch.randn(B, H, W, ld, dtype=torch.float16, device=DEV)
    out = torch.empty((B, H // 2, W // 2, C) if mode else (B, H, W, C), dtype=torch.float16, device=DEV)
    fn = lambda: O.pool_down_nhwc(x, mode, C=C, coff=coff, out=out)  # noqa: E731
    fn()
    torch.cuda.synchronize()
    ms = statistics.median(wall_ms(fn, 20) for _ in range(runs))
    moved = 2 * (B * H * W * C + out.numel())
    return {"mode": mode, "H": H, "W": W, "C": C, "ld": ld, "coff": coff, "ms": round(ms, 4), "mbytes": round(moved / 1e6, 1),
            "gb_s": round(moved / ms / 1e6, 1), "fits_cache": moved <= CACHE}


def time_forward(scale, B, size, runs):
    cfg = stock_cfg("yolov9", scale, 80)
    sd = synth_state_dict(Plan(cfg, 1, 64, 64), 0)
    x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(0)).half().to(DEV)
    eng = YoloEngine(cfg, sd)
    eng(x, want_raw=False)  # warm-up: builds the plan, tunes the convs
    torch.cuda.synchronize()
    profs = []
    for _ in range(runs):
        ops, plan = eng.profile(x)
        profs.append([t for _, _, t in ops])
    names = [n for n, _, _ in ops]
    med = [statistics.median(p[i] for p in profs) for i in range(len(names))]
    pool = sum(t for t, o in zip(med, plan.ops) if o["kind"] == L.OP_POOL_DOWN)
    fwd = statistics.median(wall_ms(lambda: eng(x, want_raw=False)) for _ in range(runs))
    raw = statistics.median(wall_ms(lambda: eng(x)) for _ in range(runs))
    gflop = sum(o.get("mfma_flops", 0) for o in plan.ops) / 1e9
    out = {"graph": f"yolov9{scale}", "batch": B, "size": size, "ops": len(names), "conv_gflop": round(gflop, 1), "sum_ops_ms": round(sum(med), 3),
           "pool_down_ops_ms": round(pool, 3), "forward_ms": round(fwd, 3), "forward_raw_ms": round(raw, 3),
           "img_s": round(B / fwd * 1e3, 1), "tflops": round(gflop / fwd, 1)}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "v9_time.py measures on the GPU"
    res = {"workload": "fp16, nc 80, synthetic weights", "runs": a.runs, "device": torch.cuda.get_device_name(0), "pool_down": [], "forward": []}
    print(f"{'mode':>4s} {'H':>4s} {'W':>4s} {'C':>4s} {'ld':>4s} {'coff':>4s} {'ms':>8s} {'MB moved':>9s} {'GB/s':>8s}  note")
    for case in pool_cases(a.batch, a.size):
        r = time_pool(a.batch, case, a.runs)
        res["pool_down"].append(r)
        print(f"{r['mode']:4d} {r['H']:4d} {r['W']:4d} {r['C']:4d} {r['ld']:4d} {r['coff']:4d} {r['ms']:8.4f} {r['mbytes']:9.1f} {r['gb_s']:8.1f}  "
              f"{'fits the 256 MiB cache' if r['fits_cache'] else ''}", flush=True)
    print(f"{'graph':8s} {'B':>3s} {'size':>5s} {'ops':>4s} {'GFLOP':>7s} {'sum ops ms':>10s} {'pool ops ms':>11s} {'forward ms':>10s} {'+raw maps ms':>12s} {'img/s':>8s} {'TFLOP/s':>8s}")
    for scale in ("c", "t"):
        r = time_forward(scale, a.batch, a.size, a.runs)
        res["forward"].append(r)
        print(f"{r['graph']:8s} {r['batch']:3d} {r['size']:5d} {r['ops']:4d} {r['conv_gflop']:7.1f} {r['sum_ops_ms']:10.3f} {r['pool_down_ops_ms']:11.3f} "
              f"{r['forward_ms']:10.3f} {r['forward_raw_ms']:12.3f} {r['img_s']:8.1f} {r['tflops']:8.1f}", flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
