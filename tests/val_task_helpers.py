"""Host-side restatements the validator-task tests need (tests/test_val_tasks.py): the fixtures of
tests/golden/make_val_task_fixtures.py unpacked, mask IoU from popcounts, and the detections the rotated test may compare."""
import json

import numpy as np

from conftest import GOLDEN

IOUV = np.linspace(0.5, 0.95, 10, dtype=np.float64).astype(np.float32)  # == torch.linspace(0.5, 0.95, 10), checked in the tests


def mask_cases():
    z = np.load(GOLDEN / "val_masks.npz", allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def mask_case(z, m):
    """-> dict: det (nd, 6), gt_boxes, gt_cls, pred (nd, H, W) uint8, gt = (nl, h, w) uint8 masks or the (1, h, w) index map, overlap,
    iou (nl, nd), tp, tp_m."""
    t = m["tag"]
    ps, gs = tuple(m["pred_shape"]), tuple(m["gt_shape"])
    pred = np.unpackbits(z[f"{t}.pred_bits"])[: int(np.prod(ps))].reshape(ps)
    gt = z[f"{t}.gt_map"] if m["overlap"] else np.unpackbits(z[f"{t}.gt_bits"])[: int(np.prod(gs))].reshape(gs)
    return dict(tag=t, det=z[f"{t}.det"], gt_boxes=z[f"{t}.gt_boxes"], gt_cls=z[f"{t}.gt_cls"], pred=pred, gt=gt, overlap=m["overlap"],
                iou=z[f"{t}.iou"], tp=z[f"{t}.tp"], tp_m=z[f"{t}.tp_m"])


def rotated_cases():
    z = np.load(GOLDEN / "val_rotated.npz", allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return [dict(tag=c["tag"], det=z[f"{c['tag']}.det"], gt=z[f"{c['tag']}.gt"], gt_cls=z[f"{c['tag']}.gt_cls"], iou=z[f"{c['tag']}.iou"],
                 tp=z[f"{c['tag']}.tp"]) for c in meta["cases"]], meta


def to_words(masks):
    """(n, ...) 0 / non-zero -> (n, ceil(hw / 64)) uint64 words, bit (p & 63) of word (p >> 6) = pixel p: the layout of bsy_pack_masks."""
    n = masks.shape[0]
    flat = (masks.reshape(n, -1) != 0)
    hw = flat.shape[1]
    words = (hw + 63) // 64
    pad = np.zeros((n, words * 64), bool)
    pad[:, :hw] = flat
    by = np.packbits(pad, axis=1, bitorder="little")  # byte k holds pixels 8k .. 8k + 7, bit i = pixel 8k + i
    return np.ascontiguousarray(by).view("<u8").reshape(n, words)


def popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(*a.shape, 8), axis=-1).sum(-1, dtype=np.int64)


def popcount_iou(gt_words, pred_words):
    """mask_iou (utils/metrics.py:220-236) of 0 / 1 masks from their bit planes: integer counts, then the reference's fp32 operations."""
    inter = np.stack([popcount(g[None, :] & pred_words).sum(-1) for g in gt_words]).astype(np.float32) if len(gt_words) else \
        np.zeros((0, len(pred_words)), np.float32)
    ag = popcount(gt_words).sum(-1).astype(np.float32)[:, None]
    ap = popcount(pred_words).sum(-1).astype(np.float32)[None, :]
    return inter / (((ag + ap) - inter) + np.float32(1e-7))


def matmul_iou(gt, pred):
    """mask_iou in the reference's own form on (n, H, W) 0 / 1 arrays, for sizes where unpacking bits on the host is too slow: the
    fp32 matmul of 0 / 1 values is a sum of integers below 2^24, exact in any order."""
    import torch
    a, b = torch.from_numpy(gt).float().flatten(1), torch.from_numpy(pred).float().flatten(1)
    inter = a @ b.T
    return (inter / (((a.sum(1)[:, None] + b.sum(1)[None]) - inter) + 1e-7)).numpy()


def label_masks(c, resize):
    """The (nl, H, W) 0 / 1 label masks the reference matches against (segment/val.py:205-212): the index map unfolded, then `resize`
    (the caller's F.interpolate + > 0.5) when the label resolution differs from the prediction's."""
    gt = c["gt"]
    if c["overlap"]:
        nl = len(c["gt_cls"])
        gt = np.concatenate([(gt == l + 1) for l in range(nl)]).astype(np.uint8) if nl else np.zeros((0, *gt.shape[1:]), np.uint8)
    if gt.shape[1:] != c["pred"].shape[1:]:
        gt = resize(gt, c["pred"].shape[1:])
    return gt


def comparable(iou_ref, det_cls, gt_cls, band):
    """Detections none of whose class-matching reference IoUs lies within `band` of a threshold: a decision there cannot flip on an
    IoU error below the band.  (nd,) bool."""
    m = np.nan_to_num(iou_ref) * (gt_cls[:, None] == det_cls[None, :])
    near = (np.abs(m[None].astype(np.float64) - IOUV.astype(np.float64)[:, None, None]) <= band).any((0, 1))
    return ~near
