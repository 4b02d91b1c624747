#!/usr/bin/env python3
"""YOLOv10's NMS-free postprocess on one GPU: bsy_end2end_topk (csrc/topk.hip) against the reference's torch ops
(v10Detect.postprocess, nn/modules/head.py:151-172: amax / topk / gather / topk / gather / cat) on the same device tensors, at the
sizes the engine serves -- 8 400 anchors (640 x 640) and 33 600 (1280 x 1280), nc = 80, max_det = 300 -- in fp16 and fp32.
Synthetic predictions (scores spread over [0, 1)); prints one JSON line.
    python tools/topk_time.py [--steps 50] [--warmup 5] [--out FILE.json]"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bs_yolo_amd import lib as L  # noqa: E402
from bs_yolo_amd import ops as O  # noqa: E402

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


def torch_postprocess(preds, max_det, nc):
    """head.py:151-172 as the reference runs it, on a (B, A, 4 + nc) view."""
    batch_size, anchors, _ = preds.shape
    boxes, scores = preds.split([4, nc], dim=-1)
    index = scores.amax(dim=-1).topk(min(max_det, anchors))[1].unsqueeze(-1)
    boxes = boxes.gather(dim=1, index=index.repeat(1, 1, 4))
    scores = scores.gather(dim=1, index=index.repeat(1, 1, nc))
    scores, index = scores.flatten(1).topk(min(max_det, anchors))
    i = torch.arange(batch_size, device=preds.device)[..., None]
    return torch.cat([boxes[i, index // nc], scores[..., None], (index % nc)[..., None].float()], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"workload": "v10Detect.postprocess, nc 80, max_det 300, synthetic predictions", "steps": a.steps, "warmup": a.warmup}
    nc, md = 80, 300
    for B, A in ((1, 8400), (16, 8400), (64, 8400), (16, 33600)):
        for dt in (torch.float16, torch.float32):
            g = torch.Generator().manual_seed(B + A)
            x = torch.cat([torch.rand(B, 4, A, generator=g) * 640, torch.rand(B, nc, A, generator=g) ** 3], 1).to(dt).to(DEV)
            out = torch.empty((B, min(md, A), 6), dtype=torch.float32, device=DEV)
            ws = torch.empty(L.lib.bsy_end2end_topk_workspace_bytes(B, A, nc, md), dtype=torch.uint8, device=DEV)
            dev_ms = timed(lambda: O.end2end_topk(x, md, out=out, workspace=ws), a.steps, a.warmup)
            ref_ms = timed(lambda: torch_postprocess(x.permute(0, 2, 1), md, nc), a.steps, a.warmup)
            ref = torch_postprocess(x.permute(0, 2, 1), md, nc)
            res[f"b{B}_a{A}_{str(dt)[6:]}"] = {"device_ms": round(dev_ms, 4), "torch_ms": round(ref_ms, 4),
                                               "scores_equal": bool(torch.equal(out[..., 4], ref[..., 4]))}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
