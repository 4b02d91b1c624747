#!/usr/bin/env python3
"""OBB throughput on one GPU, fp16, 1024 x 1024 (the OBB default size): YOLO11s-OBB forward and forward + rotated NMS
(non_max_suppression(rotated=True) on the device, conf 0.25 / iou 0.7, nc = 15) at batch 16 and 64, the same for YOLO11s detect
(forward + bsy_nms), and the rotated NMS alone at ~300 / 3 000 / 30 000 candidates per image against a torch fast-NMS (the same
probiou matrix, column max, on the same GPU).  Synthetic weights (weights.synth_state_dict); prints one JSON line.

    python tools/obb_time.py [--size 1024] [--batches 16,64] [--steps 10] [--warmup 3] [--out FILE.json]"""
import argparse
import json
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bs_yolo_amd import nms as HN  # noqa: E402
from bs_yolo_amd.engine import YoloEngine  # noqa: E402
from bs_yolo_amd.graphs import stock_cfg  # noqa: E402
from bs_yolo_amd.plan import Plan  # noqa: E402
from bs_yolo_amd.weights import synth_state_dict  # noqa: E402

DEV = "cuda:0"


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


def torch_fast_nms(boxes, scores, thr, chunk=2048):
    """Fast-NMS on xywhr boxes with torch ops: keep i iff max_{j<i} probiou(j, i) < thr (scores sorted descending inside)."""
    order = scores.argsort(descending=True)
    b = boxes[order]
    a, c_, t = b[:, 2] ** 2 / 12, b[:, 3] ** 2 / 12, b[:, 4]
    co, si = t.cos(), t.sin()
    ca, cb, cc = a * co ** 2 + c_ * si ** 2, a * si ** 2 + c_ * co ** 2, (a - c_) * co * si
    det = (ca * cb - cc ** 2).clamp(min=0)
    n = b.shape[0]
    colmax = torch.zeros(n, device=b.device)
    idx = torch.arange(n, device=b.device)
    for j0 in range(0, n, chunk):  # rows j of the upper triangle, a chunk at a time (30 000^2 floats do not fit comfortably)
        j = slice(j0, min(n, j0 + chunk))
        sa, sb, sc = ca[j, None] + ca[None], cb[j, None] + cb[None], cc[j, None] + cc[None]
        dx, dy = b[j, None, 0] - b[None, :, 0], b[j, None, 1] - b[None, :, 1]
        den = sa * sb - sc ** 2
        bd = (sa * dy ** 2 + sb * dx ** 2) / (den + 1e-7) * 0.25 - (sc * dx * dy) / (den + 1e-7) * 0.5 \
            + ((den / (4 * (det[j, None] * det[None]).sqrt() + 1e-7)) + 1e-7).log() * 0.5
        iou = 1 - (1 - (-bd.clamp(1e-7, 100.0)).exp() + 1e-7).sqrt()
        iou = iou * (idx[j, None] < idx[None])
        colmax = torch.maximum(colmax, iou.max(0).values)
    return order[colmax < thr]


def candidates(n, seed=0):
    """(1, 4 + 15 + 1, n) prediction whose every anchor passes conf 0.25: clusters of 8 jittered rotated boxes over 1024 x 1024."""
    g = torch.Generator().manual_seed(seed)
    base = max(n // 8, 1)
    rep = -(-n // base)
    jit = lambda v, s: (v.repeat(rep)[:n] + torch.randn(n, generator=g) * s)  # noqa: E731
    box = torch.stack([jit(torch.rand(base, generator=g) * 1000 + 12, 3), jit(torch.rand(base, generator=g) * 1000 + 12, 3),
                       jit(torch.rand(base, generator=g) * 60 + 8, 2).abs() + 2, jit(torch.rand(base, generator=g) * 60 + 8, 2).abs() + 2])
    cls = torch.rand(15, n, generator=g) * 0.7 + 0.26
    ang = jit((torch.rand(base, generator=g) - 0.25) * math.pi, 0.1)[None]
    return torch.cat([box, cls, ang])[None].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S = a.size
    res = {"workload": f"YOLO11s-OBB / YOLO11s {S}x{S} fp16, nc 15 / 80, synthetic weights", "steps": a.steps, "warmup": a.warmup}
    for task, nc in (("obb", 15), ("detect", 80)):
        cfg = stock_cfg("yolo11", "s", nc, task)
        eng = YoloEngine(cfg, synth_state_dict(Plan(cfg, 1, 64, 64), 0))
        for B in [int(v) for v in a.batches.split(",")]:
            x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(0)).half().to(DEV)
            fwd = timed(lambda: eng(x, want_raw=False), a.steps, a.warmup)
            if task == "obb":
                post = lambda: HN.nms_rotated_batched(eng(x, want_raw=False)[0], 0.25, 0.7, nc=nc)  # noqa: E731
            else:
                post = lambda: HN.nms_batched(eng(x, want_raw=False)[0], 0.25, 0.7)  # noqa: E731
            both = timed(post, a.steps, a.warmup)
            det, counts = post()
            res[f"{task}_b{B}"] = {"forward_ms": round(fwd, 3), "forward_img_s": round(B / fwd * 1e3, 1),
                                   "forward_nms_ms": round(both, 3), "forward_nms_img_s": round(B / both * 1e3, 1),
                                   "mean_kept": round(float(counts.float().mean()), 1)}
        eng.close()
    for n in (300, 3000, 30000):
        p = candidates(n).to(DEV)
        steps = a.steps if n < 30000 else max(2, a.steps // 5)
        dev_ms = timed(lambda: HN.nms_rotated_batched(p, 0.25, 0.7, nc=15), steps, 1)
        _, counts = HN.nms_rotated_batched(p, 0.25, 0.7, nc=15)
        x = p[0].T
        conf, cls = x[:, 4:19].max(1)
        boxes = torch.cat([x[:, :2] + cls[:, None].float() * 7680, x[:, 2:4], x[:, -1:]], 1)
        ref_ms = timed(lambda: torch_fast_nms(boxes, conf, 0.7), steps, 1)
        res[f"nms_rotated_{n}"] = {"device_ms": round(dev_ms, 3), "torch_fast_nms_ms": round(ref_ms, 3), "kept": int(counts[0]),
                                   "torch_kept": int(torch_fast_nms(boxes, conf, 0.7).numel())}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
