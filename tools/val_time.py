#!/usr/bin/env python3
"""The validator's matching step on one GPU, per batch of B images: the three device matchers (bsy_val_match, bsy_val_match_masks with
its packing, bsy_val_match_rotated) against the reference's own steps on the same device tensors, image by image as its
update_metrics loop runs them -- the IoU matrix with torch ops (box_iou; mask_iou's float matmul over H W pixels; batch_probiou),
the class mask, `.cpu().numpy()` and numpy match_predictions (oracle/val_ref.py restates it).  Wall time per batch, host work and
synchronisation included on both sides (the reference's path synchronises per image by construction; the device path once, at
the end).  Cases: 160 x 160 and 640 x 640 masks, 300 detections, 8 / 64 labels, B = 1 / 16 / 64.  Synthetic inputs; one JSON line.
    python tools/val_time.py [--steps 10] [--warmup 2] [--out FILE.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bs_yolo_amd import val as V  # noqa: E402
from oracle import val_ref as VR  # noqa: E402

DEV = "cuda:0"


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def torch_box_iou(b1, b2, eps=1e-7):  # utils/metrics.py:52-70
    (a1, a2), (c1, c2) = b1.float().unsqueeze(1).chunk(2, 2), b2.float().unsqueeze(0).chunk(2, 2)
    inter = (torch.min(a2, c2) - torch.max(a1, c1)).clamp_(0).prod(2)
    return inter / ((a2 - a1).prod(2) + (c2 - c1).prod(2) - inter + eps)


def torch_mask_iou(m1, m2, eps=1e-7):  # utils/metrics.py:220-236
    inter = torch.matmul(m1, m2.T).clamp_(0)
    return inter / ((m1.sum(1)[:, None] + m2.sum(1)[None]) - inter + eps)


def _cov(b):  # utils/metrics.py:261-278
    g = torch.cat((b[:, 2:4].pow(2) / 12, b[:, 4:]), dim=-1)
    a, bb, c = g.split(1, dim=-1)
    cos, sin = c.cos(), c.sin()
    return a * cos.pow(2) + bb * sin.pow(2), a * sin.pow(2) + bb * cos.pow(2), (a - bb) * cos * sin


def torch_probiou(o1, o2, eps=1e-7):  # utils/metrics.py:327-358
    x1, y1 = o1[..., :2].split(1, dim=-1)
    x2, y2 = (x.squeeze(-1)[None] for x in o2[..., :2].split(1, dim=-1))
    a1, b1, c1 = _cov(o1)
    a2, b2, c2 = (x.squeeze(-1)[None] for x in _cov(o2))
    den = (a1 + a2) * (b1 + b2) - (c1 + c2).pow(2)
    t1 = (((a1 + a2) * (y1 - y2).pow(2) + (b1 + b2) * (x1 - x2).pow(2)) / (den + eps)) * 0.25
    t2 = (((c1 + c2) * (x2 - x1) * (y1 - y2)) / (den + eps)) * 0.5
    t3 = (den / (4 * ((a1 * b1 - c1.pow(2)).clamp_(0) * (a2 * b2 - c2.pow(2)).clamp_(0)).sqrt() + eps) + eps).log() * 0.5
    bd = (t1 + t2 + t3).clamp(eps, 100.0)
    return 1 - (1.0 - (-bd).exp() + eps).sqrt()


def ref_match(det_cls, gt_cls, iou):  # engine/validator.py:236-262: the device -> host copy of the matrix, then numpy
    return VR.match_predictions(det_cls.cpu().numpy(), gt_cls.cpu().numpy(), iou.cpu().numpy())


def inputs(B, nd, nl, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.rand(B, nl, 2, generator=g) * 500 + 20
    wh = torch.rand(B, nl, 2, generator=g) * 100 + 20
    src = torch.randint(0, nl, (B, nd), generator=g)
    bi = torch.arange(B)[:, None]
    dxy, dwh = lab[bi, src] + torch.randn(B, nd, 2, generator=g) * 4, wh[bi, src] + torch.randn(B, nd, 2, generator=g).abs() * 4
    gcls = torch.randint(0, 8, (B, nl), generator=g).float()
    conf = torch.rand(B, nd, 1, generator=g)
    dcls = gcls[bi, src][..., None]
    ang, dang = (torch.rand(B, nl, 1, generator=g) - 0.25) * 3.14159, torch.randn(B, nd, 1, generator=g) * 0.05
    box_det = torch.cat([dxy - dwh / 2, dxy + dwh / 2, conf, dcls], 2)
    rot_det = torch.cat([dxy, dwh, conf, dcls, ang[bi, src] + dang], 2)
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    # masks: the boxes filled, at the mask resolution of a 640-pixel frame; built on the device, image by image (float, as the
    # validator holds them: 64 x 300 masks of 640 x 640 are 31 GB)
    ys, xs = torch.arange(H, device=DEV)[None, :, None] * (640.0 / H), torch.arange(W, device=DEV)[None, None, :] * (640.0 / W)

    def fill(c, s):
        out = torch.empty((B, c.shape[1], H, W), dtype=torch.float32, device=DEV)
        lo, hi = d(c - s / 2)[..., None, None], d(c + s / 2)[..., None, None]
        for b in range(B):
            out[b] = ((xs >= lo[b, :, 0]) & (xs < hi[b, :, 0]) & (ys >= lo[b, :, 1]) & (ys < hi[b, :, 1])).float()
        return out

    return dict(box_det=d(box_det), rot_det=d(rot_det), gt_box=d(torch.cat([lab - wh / 2, lab + wh / 2], 2)), gt_rbox=d(torch.cat([lab, wh, ang], 2)),
                gt_cls=d(gcls), pred_masks=fill(dxy, dwh), gt_masks=fill(lab, wh),
                counts=torch.full((B,), nd, dtype=torch.int32, device=DEV), gt_counts=torch.full((B,), nl, dtype=torch.int32, device=DEV))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"workload": "validator matching per batch, 300 detections, ms wall (device matchers vs the reference's torch + numpy steps)",
           "steps": a.steps, "warmup": a.warmup}
    nd = 300
    for (H, W) in ((160, 160), (640, 640)):
        for nl in (8, 64):
            for B in (1, 16, 64):
                x = inputs(B, nd, nl, H, W, B + nl + H)
                r = {}
                if H == 160:  # boxes and rotated boxes do not depend on the mask size
                    r["box_device_ms"] = timed(lambda: V.match_batched(x["box_det"], x["counts"], x["gt_box"], x["gt_cls"], x["gt_counts"]), a.steps, a.warmup)
                    r["box_torch_ms"] = timed(lambda: [ref_match(x["box_det"][b, :, 5], x["gt_cls"][b], torch_box_iou(x["gt_box"][b], x["box_det"][b, :, :4]))
                                                       for b in range(B)], a.steps, a.warmup)
                    r["rotated_device_ms"] = timed(lambda: V.match_rotated_batched(x["rot_det"], x["counts"], x["gt_rbox"], x["gt_cls"], x["gt_counts"]),
                                                   a.steps, a.warmup)
                    r["rotated_torch_ms"] = timed(lambda: [ref_match(x["rot_det"][b, :, 5], x["gt_cls"][b],
                                                                     torch_probiou(x["gt_rbox"][b], x["rot_det"][b][:, [0, 1, 2, 3, 6]])) for b in range(B)],
                                                  a.steps, a.warmup)

                def dev_masks():
                    return V.match_masks_batched(x["box_det"], x["counts"], V.pack_masks(x["pred_masks"]), V.pack_masks(x["gt_masks"]), x["gt_cls"],
                                                 x["gt_counts"])

                pp, gp = V.pack_masks(x["pred_masks"]), V.pack_masks(x["gt_masks"])
                r["masks_device_ms"] = timed(dev_masks, a.steps, a.warmup)
                r["masks_device_packed_ms"] = timed(lambda: V.match_masks_batched(x["box_det"], x["counts"], pp, gp, x["gt_cls"], x["gt_counts"]),
                                                    a.steps, a.warmup)
                r["masks_torch_ms"] = timed(lambda: [ref_match(x["box_det"][b, :, 5], x["gt_cls"][b],
                                                               torch_mask_iou(x["gt_masks"][b].view(nl, -1), x["pred_masks"][b].view(nd, -1)))
                                                     for b in range(B)], a.steps, a.warmup)
                want = np.stack([ref_match(x["box_det"][b, :, 5], x["gt_cls"][b], torch_mask_iou(x["gt_masks"][b].view(nl, -1), x["pred_masks"][b].view(nd, -1)))
                                 for b in range(B)])
                r["masks_tp_equal"] = bool(np.array_equal(dev_masks().cpu().numpy(), want))
                res[f"{H}x{W}_l{nl}_b{B}"] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}
                del x, pp, gp
                torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
