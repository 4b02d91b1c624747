#!/usr/bin/env python3
"""Generate the segment / OBB validator-matching fixtures by RUNNING THE REFERENCE (build container only).

    python tests/golden/make_val_task_fixtures.py

The reference is imported in-process with make_fixtures.py's stand-ins.  SegmentationValidator._process_batch
(models/yolo/segment/val.py:173-217) and OBBValidator._process_batch (models/yolo/obb/val.py:53-80) run unbound on a namespace that
carries `iouv` and BaseValidator.match_predictions (engine/validator.py:222-262).  Nothing of the reference is modified or copied.
  val_masks.npz    per case: detections (nd, 6), label boxes / classes, predicted masks (nd, H, W) and label masks (nl, h, w) or, with
           overlap, the (1, h, w) index map -- all 0 / 1 (or small integers), stored with np.packbits / as uint8; the reference's
           mask_iou matrix (after its own resize where h, w differ), tp (boxes) and tp_m (masks).
  val_rotated.npz  per case: detections (nd, 7) [x, y, w, h, conf, cls, theta], labels (nl, 5) xywhr, the reference's batch_probiou
           (fp32, CPU) and tp; meta records, from a float64 evaluation of the same formula, the largest fp32 error and how many
           detections have a class-matching IoU within 4 x that of a threshold (the test's band comes from the GPU's own error).
Tie condition (asserted here, on the inputs): no detection has two class-matching labels of EQUAL IoU >= 0.5 -- the reference's
argsort is unstable there, so its answer would not be defined.
"""
import json
import math
import sys
import types
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_fixtures as MF  # noqa: E402,F401  (stand-ins + the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ultralytics.engine.validator import BaseValidator  # noqa: E402
from ultralytics.models.yolo.obb.val import OBBValidator  # noqa: E402
from ultralytics.models.yolo.segment.val import SegmentationValidator  # noqa: E402
from ultralytics.utils import metrics as rmetrics  # noqa: E402
import ultralytics.models.yolo.segment.val as segval  # noqa: E402

IOUV = torch.linspace(0.5, 0.95, 10)  # detect/val.py:36


def validator_ns():
    ns = types.SimpleNamespace(iouv=IOUV)
    ns.match_predictions = types.MethodType(BaseValidator.match_predictions, ns)
    return ns


def assert_no_ties(iou, det_cls, gt_cls, tag):
    m = iou * (gt_cls[:, None] == det_cls[None]).astype(np.float32)
    for d in range(m.shape[1]):
        v = m[:, d][m[:, d] >= 0.5]
        assert len(np.unique(v)) == len(v), f"{tag}: detection {d} has tied class-matching labels"


# ---- masks -----------------------------------------------------------------------------------------------------------------
def blob(p, H, W):
    """A wobbly ellipse in normalised coordinates p = (cx, cy, rx, ry, k, phase), rasterised at (H, W)."""
    cx, cy, rx, ry, k, ph = p
    y, x = np.mgrid[0:H, 0:W]
    u, v = ((x + 0.5) / W - cx) / rx, ((y + 0.5) / H - cy) / ry
    r = 1.0 + 0.18 * np.sin(k * np.arctan2(v, u) + ph)
    return (u * u + v * v <= r * r).astype(np.uint8)


def boxes_of(masks):
    out = np.zeros((len(masks), 4), np.float32)
    for i, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        if len(ys):
            out[i] = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
    return out


def mask_case(seed, nd, nl, ncls, pred_hw, gt_hw, overlap, jitter=0.02):
    rng = np.random.default_rng(seed)
    lp = np.stack([rng.uniform(0.15, 0.85, nl), rng.uniform(0.15, 0.85, nl), rng.uniform(0.05, 0.2, nl), rng.uniform(0.05, 0.2, nl),
                   rng.integers(2, 6, nl), rng.uniform(0, 6.28, nl)], 1) if nl else np.zeros((0, 6))
    lcls = rng.integers(0, ncls, nl).astype(np.float32)
    src = rng.integers(0, max(nl, 1), nd)
    dp = lp[src].copy() if nl else np.stack([rng.uniform(0.2, 0.8, nd), rng.uniform(0.2, 0.8, nd), rng.uniform(0.05, 0.2, nd),
                                              rng.uniform(0.05, 0.2, nd), rng.integers(2, 6, nd), rng.uniform(0, 6.28, nd)], 1)
    dp[:, :2] += rng.normal(0, jitter, (nd, 2))
    dp[:, 2:4] *= rng.uniform(0.8, 1.25, (nd, 2))
    dcls = np.where(rng.random(nd) < 0.8, lcls[src] if nl else 0, rng.integers(0, ncls, nd)).astype(np.float32)
    pred = np.stack([blob(p, *pred_hw) for p in dp]) if nd else np.zeros((0, *pred_hw), np.uint8)
    gt = np.stack([blob(p, *gt_hw) for p in lp]) if nl else np.zeros((0, *gt_hw), np.uint8)
    if overlap:  # the dataset's index map: a later label overwrites an earlier one (data/utils.py polygons2masks_overlap sorts by area;
        idx = np.zeros((1, *gt_hw), np.uint8)  # here: in label order -- _process_batch only reads the map)
        for l in range(nl):
            idx[0][gt[l] > 0] = l + 1
        gt = idx
    det = np.zeros((nd, 6), np.float32)
    det[:, :4] = boxes_of(pred)
    det[:, 4] = np.sort(rng.uniform(0.25, 1.0, nd))[::-1]
    det[:, 5] = dcls
    return det, lcls, pred, gt, overlap


def edge_case():
    """Hand-built 32 x 48 masks: an empty prediction, an empty label, a union of exactly 1 pixel, identical masks, disjoint masks."""
    H, W = 32, 48
    gt = np.zeros((5, H, W), np.uint8)
    pred = np.zeros((7, H, W), np.uint8)
    gt[0, 4:20, 4:30] = 1            # label 0: identical to prediction 0
    gt[1, 25, 40] = 1                # label 1: one pixel, equal to prediction 1 (union 1)
    # label 2 stays empty
    gt[3, 20:30, 2:20] = 1           # label 3: overlapped by prediction 3 (IoU 0.8) and prediction 4 (IoU 0.5)
    gt[4, 0:3, 40:48] = 1            # label 4: no prediction near it
    pred[0, 4:20, 4:30] = 1
    pred[1, 25, 40] = 1
    # prediction 2 stays empty
    pred[3, 20:28, 2:20] = 1
    pred[4, 20:25, 2:20] = 1
    pred[5, 25, 41] = 1              # one pixel beside label 1: intersection 0, union 2
    pred[6, 10:14, 30:47] = 1        # touches nothing of its class
    lcls = np.array([0, 1, 1, 2, 0], np.float32)
    det = np.zeros((7, 6), np.float32)
    det[:, :4] = boxes_of(pred)
    det[:, 4] = np.linspace(0.9, 0.3, 7)
    det[:, 5] = [0, 1, 1, 2, 2, 1, 0]
    return det, lcls, pred, gt, False


MASK_CASES = [  # tag, builder
    ("plain", lambda: mask_case(1, 40, 9, 3, (160, 160), (160, 160), False)),
    ("overlap", lambda: mask_case(2, 40, 9, 3, (160, 160), (160, 160), True)),
    ("resize", lambda: mask_case(3, 30, 8, 2, (160, 160), (40, 40), False)),
    ("overlap_resize", lambda: mask_case(4, 30, 8, 2, (100, 150), (50, 75), True)),
    ("odd", lambda: mask_case(5, 25, 6, 2, (100, 150), (100, 150), False)),
    ("odd_overlap", lambda: mask_case(6, 25, 6, 2, (100, 150), (100, 150), True)),
    ("many_labels", lambda: mask_case(7, 120, 70, 4, (96, 96), (96, 96), False, jitter=0.01)),
    ("d1024", lambda: mask_case(8, 1024, 20, 3, (64, 64), (64, 64), False)),
    ("edges", edge_case),
]


def mask_fixtures():
    out, meta = {}, []
    ns = validator_ns()
    seen = {}
    real_iou = segval.mask_iou

    def spy(a, b, eps=1e-7):  # records the matrix the reference's own _process_batch computes (after its own resize)
        seen["iou"] = real_iou(a, b, eps)
        return seen["iou"]

    segval.mask_iou = spy
    try:
        for tag, make in MASK_CASES:
            det, lcls, pred, gt, overlap = make()
            d, c = torch.from_numpy(det), torch.from_numpy(lcls)
            pm, gm = torch.from_numpy(pred).float(), torch.from_numpy(gt).float()  # the validator's masks are float (segment/val.py:66)
            # label boxes at the predictions' resolution, from the masks the reference itself matches against
            if overlap:
                lab_masks = np.concatenate([(gt == l + 1) for l in range(len(lcls))]).astype(np.uint8)
            else:
                lab_masks = gt
            sy, sx = pred.shape[1] / gt.shape[1], pred.shape[2] / gt.shape[2]
            gb = boxes_of(lab_masks) * np.array([sx, sy, sx, sy], np.float32)
            tp_m = SegmentationValidator._process_batch(ns, d, torch.from_numpy(gb), c, pm, gm, overlap, masks=True)
            iou = seen["iou"].numpy()
            tp = SegmentationValidator._process_batch(ns, d, torch.from_numpy(gb), c)
            assert iou.shape == (len(lcls), len(det)) and iou.dtype == np.float32
            assert_no_ties(iou, det[:, 5], lcls, tag)
            out[f"{tag}.det"], out[f"{tag}.gt_boxes"], out[f"{tag}.gt_cls"] = det, gb, lcls
            out[f"{tag}.pred_bits"] = np.packbits(pred)
            if overlap:
                out[f"{tag}.gt_map"] = gt
            else:
                out[f"{tag}.gt_bits"] = np.packbits(gt)
            out[f"{tag}.iou"], out[f"{tag}.tp"], out[f"{tag}.tp_m"] = iou, tp.numpy(), tp_m.numpy()
            meta.append({"tag": tag, "overlap": bool(overlap), "pred_shape": list(pred.shape), "gt_shape": list(gt.shape)})
            print("masks", tag, pred.shape, gt.shape, "overlap", overlap, "tp_m@.5", int(tp_m[:, 0].sum()), "tp_m@.95", int(tp_m[:, -1].sum()),
                  "iou max", float(iou.max()) if iou.size else None)
    finally:
        segval.mask_iou = real_iou
    out["meta"] = json.dumps(meta)
    np.savez_compressed(HERE / "val_masks.npz", **out)


# ---- rotated ---------------------------------------------------------------------------------------------------------------
def probiou64(gt, det, eps=1e-7):
    """batch_probiou (metrics.py:327-358) in float64 on the fp32 inputs: the yardstick for the fp32 implementations' error."""
    return rmetrics.batch_probiou(torch.from_numpy(gt).double(), torch.from_numpy(det).double(), eps).numpy()


def rot_case(seed, nd, nl, ncls, jitter, zero_wh=False):
    rng = np.random.default_rng(seed)
    lab = np.stack([rng.uniform(20, 620, nl), rng.uniform(20, 620, nl), rng.uniform(8, 140, nl), rng.uniform(8, 140, nl),
                    (rng.random(nl) - 0.25) * math.pi], 1).astype(np.float32)
    lcls = rng.integers(0, ncls, nl).astype(np.float32)
    src = rng.integers(0, nl, nd)
    box = lab[src] + np.concatenate([rng.normal(0, jitter, (nd, 2)), rng.normal(0, jitter, (nd, 2)), rng.normal(0, 0.06, (nd, 1))], 1)
    box[:, 2:4] = np.abs(box[:, 2:4]) + 2
    far = rng.random(nd) < 0.15
    box[far, :2] = rng.uniform(20, 620, (int(far.sum()), 2))
    det = np.zeros((nd, 7), np.float32)
    det[:, :4] = box[:, :4]
    det[:, 4] = np.sort(rng.uniform(0.25, 1.0, nd))[::-1]
    det[:, 5] = np.where(rng.random(nd) < 0.8, lcls[src], rng.integers(0, ncls, nd))
    det[:, 6] = box[:, 4]
    if zero_wh:  # axis-aligned only: at a general angle the sign of a degenerate determinant hangs on the last ulp of cos / sin
        for sl, cols in ((slice(0, None, 5), [2]), (slice(1, None, 7), [3]), (slice(2, None, 11), [2, 3])):
            det[sl, cols] = 0.0
            det[sl, 6] = 0.0
        lab[::4, 2] = 0.0
        lab[::4, 4] = 0.0
    return det, lab, lcls


ROT_CASES = [("small", lambda: rot_case(11, 40, 12, 3, 3.0)), ("dota", lambda: rot_case(12, 300, 60, 15, 4.0)),
             ("single", lambda: rot_case(13, 7, 1, 1, 2.0)), ("dense", lambda: rot_case(14, 1024, 100, 5, 5.0)),
             ("zero_wh", lambda: rot_case(15, 200, 24, 4, 3.0, zero_wh=True))]


def rotated_fixtures():
    out, meta = {}, []
    ns = validator_ns()
    err, total = 0.0, 0
    results = []
    for tag, make in ROT_CASES:
        det, lab, lcls = make()
        d, g, c = torch.from_numpy(det), torch.from_numpy(lab), torch.from_numpy(lcls)
        iou = rmetrics.batch_probiou(g, torch.cat([d[:, :4], d[:, -1:]], dim=-1)).numpy()
        tp = OBBValidator._process_batch(ns, d, g, c).numpy()
        i64 = probiou64(lab, det[:, [0, 1, 2, 3, 6]])
        ok = np.isfinite(iou) & np.isfinite(i64)
        assert (np.isfinite(iou) == np.isfinite(i64)).all(), tag
        err = max(err, float(np.abs(iou[ok] - i64[ok]).max()))
        assert_no_ties(np.nan_to_num(iou), det[:, 5], lcls, tag)
        results.append((tag, det, lab, lcls, iou, tp))
        total += len(det)
    band = 4 * err
    excluded = 0
    for tag, det, lab, lcls, iou, tp in results:
        m = np.nan_to_num(iou) * (lcls[:, None] == det[None, :, 5])
        near = (np.abs(m[None] - IOUV.numpy()[:, None, None]) <= band).any((0, 1))
        excluded += int(near.sum())
        out[f"{tag}.det"], out[f"{tag}.gt"], out[f"{tag}.gt_cls"], out[f"{tag}.iou"], out[f"{tag}.tp"] = det, lab, lcls, iou, tp
        meta.append({"tag": tag, "nd": len(det), "nl": len(lab), "near_f64_band": int(near.sum())})
        print("rotated", tag, det.shape, lab.shape, "tp@.5", int(tp[:, 0].sum()), "tp@.95", int(tp[:, -1].sum()), "near", int(near.sum()))
    assert excluded < 0.01 * total, (excluded, total)
    out["meta"] = json.dumps({"cases": meta, "fp32_vs_f64_max_err": err, "f64_band": band, "excluded_f64_band": excluded, "detections": total})
    print("rotated: fp32 CPU vs float64 max err", err, "band", band, "excluded", excluded, "of", total)
    np.savez_compressed(HERE / "val_rotated.npz", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    mask_fixtures()
    rotated_fixtures()
    for f in ("val_masks.npz", "val_rotated.npz"):
        print(f, (HERE / f).stat().st_size, "bytes")
