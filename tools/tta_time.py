#!/usr/bin/env python3
"""Test-time augmentation throughput: YOLO11s, 640 x 640, batch 64 (default), fp16 -- the engine's TTA forward (augment=True) next
to its three single-scale forwards at the pass sizes (640 / 544 / 448), all in one process, and the two TTA kernels alone
(bsy_scale_img per scaled pass, bsy_tta_merge) with their bytes over time.

    python tools/tta_time.py [--batch 64] [--size 640] [--steps 20] [--warmup 5] [--out FILE.json]

Run it under `rocprofv3 --kernel-trace --stats` (with --steps small) for the kernels' share of a TTA step in the trace."""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bs_yolo_amd import ops as O  # noqa: E402
from bs_yolo_amd.engine import YoloEngine  # noqa: E402
from bs_yolo_amd.graphs import stock_cfg  # noqa: E402
from oracle import yolo_ref as R  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--scale", default="s")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, S = a.batch, a.size
    P = R.synth_params(R.Model("yolo11", a.scale, 80, "detect"), 0)
    eng = YoloEngine(stock_cfg("yolo11", a.scale), P)
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(0)).half().to("cuda:0")
    passes = eng.tta_geometry(S, S)
    res = {"workload": f"YOLO11{a.scale} {S}x{S} bs={B} fp16", "steps": a.steps, "warmup": a.warmup, "passes": []}
    single = 0.0
    for p in passes:
        xi = O.scale_img(x, p.ratio, p.flip, 32) if p.ratio != 1.0 else x
        ms = timed(lambda: eng(xi, want_raw=False), a.steps, a.warmup)
        single += ms
        res["passes"].append({"padded": list(p.padded), "window": list(p.window), "forward_ms": round(ms, 4),
                              "images_per_s": round(B / ms * 1e3, 1)})
    ms_tta = timed(lambda: eng(x, augment=True), a.steps, a.warmup)
    res.update(tta_ms=round(ms_tta, 4), tta_images_per_s=round(B / ms_tta * 1e3, 1), sum_of_single_forwards_ms=round(single, 4))
    # the glue alone: every scaled pass's bsy_scale_img + the one bsy_tta_merge, on the pass outputs of a TTA step
    ys = [eng(O.scale_img(x, p.ratio, p.flip, 32) if p.ratio != 1.0 else x, want_raw=False)[0].clone() for p in passes]
    outs = {i: O.scale_img(x, p.ratio, p.flip, 32) for i, p in enumerate(passes) if p.ratio != 1.0}
    esz = x.element_size()
    kern = {}
    for i, p in enumerate(passes):
        if p.ratio == 1.0:
            continue
        ms = timed(lambda: O.scale_img(x, p.ratio, p.flip, 32, out=outs[i]), a.steps, a.warmup)
        byts = (x.numel() + outs[i].numel()) * esz  # image read once + scaled input written
        kern[f"scale_img_{p.padded[0]}x{p.padded[1]}"] = {"ms": round(ms, 4), "bytes": byts, "TB_per_s": round(byts / ms / 1e9, 2)}
    wins = [p.window for p in passes]
    merged = O.tta_merge(ys, wins, [p.ratio for p in passes], [p.flip for p in passes], (S, S))
    ms = timed(lambda: O.tta_merge(ys, wins, [p.ratio for p in passes], [p.flip for p in passes], (S, S), out=merged), a.steps,
               a.warmup)
    byts = 2 * merged.numel() * esz  # kept windows read + merged output written
    kern["tta_merge"] = {"ms": round(ms, 4), "bytes": byts, "TB_per_s": round(byts / ms / 1e9, 2)}
    glue = sum(v["ms"] for v in kern.values())
    res.update(kernels=kern, glue_ms=round(glue, 4), glue_share_of_tta_step=round(glue / ms_tta, 4))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
