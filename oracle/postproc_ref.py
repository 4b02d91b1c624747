"""CPU restatement of the reference's detection post-processing.

TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py.

  * ``greedy_nms``  : torchvision.ops.nms (un-vendored third-party dependency, ``torchvision>=0.9.0``
                      unpinned in the reference's pyproject.toml:74; call site utils/ops.py:296).
                      Restates the published CPU algorithm (torchvision/csrc/ops/cpu/nms_kernel.cpp,
                      ``nms_kernel_impl``): order = argsort(scores, descending); keep i unless
                      suppressed; suppress j when inter/(area_i+area_j-inter) > thr (strict).
                      Tie order among equal scores is implementation-defined upstream; the oracle
                      (and the HIP kernel) break ties by ascending candidate index.  PARITY UNPINNED.
  * ``non_max_suppression`` : utils/ops.py:167-316 (rotated / labels / end2end branches omitted).
  * ``xywh2xyxy`` :416-433, ``scale_boxes`` :92-127, ``clip_boxes`` :319-337,
    ``process_mask`` :663-694, ``crop_mask`` :644-660.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def greedy_nms(boxes: torch.Tensor, scores: torch.Tensor, iou_thres: float) -> torch.Tensor:
    """Indices of kept boxes, in descending-score order.  fp32 arithmetic, op order as nms_kernel_impl."""
    if boxes.numel() == 0:
        return torch.zeros((0,), dtype=torch.long)
    b = boxes.detach().to(torch.float32).cpu().numpy()
    s = scores.detach().to(torch.float32).cpu().numpy()
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    areas = ((x2 - x1) * (y2 - y1)).astype(np.float32)
    order = np.argsort(-s, kind="stable")  # ties: ascending index
    thr = np.float32(iou_thres)
    n = len(order)
    suppressed = np.zeros(n, dtype=bool)
    keep = []
    # work in sorted space so the inner step vectorises
    x1, y1, x2, y2, areas = x1[order], y1[order], x2[order], y2[order], areas[order]
    for i in range(n):
        if suppressed[i]:
            continue
        keep.append(order[i])
        if i + 1 == n:
            break
        xx1 = np.maximum(x1[i], x1[i + 1:])
        yy1 = np.maximum(y1[i], y1[i + 1:])
        xx2 = np.minimum(x2[i], x2[i + 1:])
        yy2 = np.minimum(y2[i], y2[i + 1:])
        w = np.maximum(np.float32(0), xx2 - xx1)
        h = np.maximum(np.float32(0), yy2 - yy1)
        inter = (w * h).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / (areas[i] + areas[i + 1:] - inter)
        suppressed[i + 1:] |= ovr > thr
    return torch.from_numpy(np.asarray(keep, dtype=np.int64))


def xywh2xyxy(x):  # utils/ops.py:416-433
    y = torch.empty_like(x)
    xy = x[..., :2]
    wh = x[..., 2:] / 2
    y[..., :2] = xy - wh
    y[..., 2:] = xy + wh
    return y


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False,
                        multi_label=False, max_det=300, nc=0, max_nms=30000, max_wh=7680, in_place=True,
                        nms_fn=greedy_nms, boxes_xyxy=False):
    """utils/ops.py:167-316 without the wall-clock bail-out (:238,:312-314)."""
    assert 0 <= conf_thres <= 1 and 0 <= iou_thres <= 1
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    if classes is not None:
        classes = torch.tensor(classes, device=prediction.device)
    bs = prediction.shape[0]
    nc = nc or (prediction.shape[1] - 4)
    nm = prediction.shape[1] - nc - 4
    mi = 4 + nc
    xc = prediction[:, 4:mi].amax(1) > conf_thres
    multi_label &= nc > 1
    prediction = prediction.transpose(-1, -2)
    if boxes_xyxy:  # test hook: the caller already converted the boxes (fp16 parity case)
        pass
    elif in_place:
        prediction[..., :4] = xywh2xyxy(prediction[..., :4])
    else:
        prediction = torch.cat((xywh2xyxy(prediction[..., :4]), prediction[..., 4:]), dim=-1)
    output = [torch.zeros((0, 6 + nm), device=prediction.device)] * bs
    for xi, x in enumerate(prediction):
        x = x[xc[xi]]
        if not x.shape[0]:
            continue
        box, cls, mask = x.split((4, nc, nm), 1)
        if multi_label:
            i, j = torch.where(cls > conf_thres)
            x = torch.cat((box[i], x[i, 4 + j, None], j[:, None].float(), mask[i]), 1)
        else:
            conf, j = cls.max(1, keepdim=True)
            x = torch.cat((box, conf, j.float(), mask), 1)[conf.view(-1) > conf_thres]
        if classes is not None:
            x = x[(x[:, 5:6] == classes).any(1)]
        n = x.shape[0]
        if not n:
            continue
        if n > max_nms:
            x = x[x[:, 4].argsort(descending=True, stable=True)[:max_nms]]
        c = x[:, 5:6] * (0 if agnostic else max_wh)
        scores = x[:, 4]
        boxes = x[:, :4] + c
        i = nms_fn(boxes, scores, iou_thres)
        i = i[:max_det]
        output[xi] = x[i]
    return output


def clip_boxes(boxes, shape):  # utils/ops.py:319-337
    boxes[..., 0] = boxes[..., 0].clamp(0, shape[1])
    boxes[..., 1] = boxes[..., 1].clamp(0, shape[0])
    boxes[..., 2] = boxes[..., 2].clamp(0, shape[1])
    boxes[..., 3] = boxes[..., 3].clamp(0, shape[0])
    return boxes


def scale_boxes(img1_shape, boxes, img0_shape, ratio_pad=None, padding=True, xywh=False):  # utils/ops.py:92-127
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1),
               round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1))
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    if padding:
        boxes[..., 0] -= pad[0]
        boxes[..., 1] -= pad[1]
        if not xywh:
            boxes[..., 2] -= pad[0]
            boxes[..., 3] -= pad[1]
    boxes[..., :4] /= gain
    return clip_boxes(boxes, img0_shape)


def crop_mask(masks, boxes):  # utils/ops.py:644-660
    _, h, w = masks.shape
    x1, y1, x2, y2 = torch.chunk(boxes[:, :, None], 4, 1)
    r = torch.arange(w, dtype=x1.dtype)[None, None, :]
    c = torch.arange(h, dtype=x1.dtype)[None, :, None]
    return masks * ((r >= x1) * (r < x2) * (c >= y1) * (c < y2))


def process_mask(protos, masks_in, bboxes, shape, upsample=False):  # utils/ops.py:663-694
    c, mh, mw = protos.shape
    ih, iw = shape
    masks = (masks_in @ protos.float().view(c, -1)).view(-1, mh, mw)
    width_ratio = mw / iw
    height_ratio = mh / ih
    db = bboxes.clone()
    db[:, 0] *= width_ratio
    db[:, 2] *= width_ratio
    db[:, 3] *= height_ratio
    db[:, 1] *= height_ratio
    masks = crop_mask(masks, db)
    if upsample:
        masks = F.interpolate(masks[None], shape, mode="bilinear", align_corners=False)[0]
    return masks.gt_(0.0)


def scale_masks(masks, shape, padding=True):  # utils/ops.py:712-737
    import torch.nn.functional as F
    mh, mw = masks.shape[2:]
    gain = min(mh / shape[0], mw / shape[1])
    pad = [mw - shape[1] * gain, mh - shape[0] * gain]
    if padding:
        pad[0] /= 2
        pad[1] /= 2
    top, left = (int(pad[1]), int(pad[0])) if padding else (0, 0)
    bottom, right = (int(mh - pad[1]), int(mw - pad[0]))
    masks = masks[..., top:bottom, left:right]
    return F.interpolate(masks, shape, mode="bilinear", align_corners=False)


def process_mask_native(protos, masks_in, bboxes, shape):  # utils/ops.py:696-709
    c, mh, mw = protos.shape
    masks = (masks_in @ protos.float().view(c, -1)).view(-1, mh, mw)
    masks = scale_masks(masks[None], shape)[0]
    masks = crop_mask(masks, bboxes)
    return masks.gt_(0.0)


# ------------------------------------------------------------------------------------------------------------
# float64 restatement of the mask functions, with a per-pixel error bound (tests/test_postprocess_edges.py)
# ------------------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24  # fp32 unit roundoff


def _src_index(n_in: int, n_out: int, fused: bool = True):
    """aten's area_pixel_compute_source_index (align_corners=False, size given): the source coordinate and the two
    weights are part of the operation's definition and are fp32 for fp32 / fp16 tensors, so they are computed in
    fp32 here as well and only then widened.  `fused`: scale * (dst + 0.5) - 0.5 rounded once (a fused multiply-add,
    what ATen's builds do -- the CPU kernels here reproduce it bit for bit) or after each operation (what
    csrc/masks.hip does, compiled with -ffp-contract=off); the two coordinates differ by at most one fp32 ulp."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    d = np.arange(n_out, dtype=np.float32) + f(0.5)
    s = (np.float64(scale) * d.astype(np.float64) - 0.5).astype(np.float32) if fused else scale * d - f(0.5)
    s = np.maximum(s, f(0))
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(np.float32)
    l0 = f(1) - l1
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def bilinear64(src: np.ndarray, oh: int, ow: int, fused: bool = True) -> np.ndarray:
    """F.interpolate(src, (oh, ow), mode="bilinear", align_corners=False) over the last two axes, float64 sums."""
    y0, y1, ly0, ly1 = _src_index(src.shape[-2], oh, fused)
    x0, x1, lx0, lx1 = _src_index(src.shape[-1], ow, fused)
    top, bot = src[..., y0, :], src[..., y1, :]
    return (ly0[:, None] * (lx0 * top[..., x0] + lx1 * top[..., x1]) +
            ly1[:, None] * (lx0 * bot[..., x0] + lx1 * bot[..., x1]))


def crop_inside(boxes: torch.Tensor, h: int, w: int) -> np.ndarray:
    """crop_mask's (n, h, w) in-box predicate, fp32 comparisons as the reference makes them (utils/ops.py:656-660)."""
    x1, y1, x2, y2 = torch.chunk(boxes.float()[:, :, None], 4, 1)
    r = torch.arange(w, dtype=x1.dtype)[None, None, :]
    c = torch.arange(h, dtype=x1.dtype)[None, :, None]
    return ((r >= x1) * (r < x2) * (c >= y1) * (c < y2)).numpy().astype(bool)


def _lowres64(protos, masks_in):
    """(n, mh, mw) float64 masks, S = sum_k |c_k p_k| and the fp32 dot-product bound (nm + 2) * 2^-24 * S, which holds
    for any summation order (fused or not) of an nm-term fp32 dot product."""
    c, mh, mw = protos.shape
    P = protos.detach().double().numpy().reshape(c, -1)  # fp16 prototypes: the reference upcasts them (protos.float())
    Cf = masks_in.detach().double().numpy()
    low = (Cf @ P).reshape(-1, mh, mw)
    S = (np.abs(Cf) @ np.abs(P)).reshape(-1, mh, mw)
    return low, S, (c + 2) * U32 * S


def process_mask64(protos, masks_in, bboxes, shape, upsample=False, fused=True):
    """process_mask in float64 -> (v, e): the pre-threshold value per output pixel and a bound on what an fp32
    implementation may differ from it.  The crop arithmetic on the boxes is the reference's own fp32 (bboxes.clone(),
    *= mw / iw).  e = e_low without the resize, interp(e_low) + 8 * 2^-24 * interp(S) with it.  Where the crop zeroes
    every contributing pixel, v = e = 0 exactly: such a pixel is known to be 0, not ambiguous (see classify_masks)."""
    c, mh, mw = protos.shape
    ih, iw = shape
    low, S, e_low = _lowres64(protos, masks_in)
    db = bboxes.detach().float().clone()
    db[:, 0] *= mw / iw
    db[:, 2] *= mw / iw
    db[:, 3] *= mh / ih
    db[:, 1] *= mh / ih
    inside = crop_inside(db, mh, mw)
    low, S, e_low = low * inside, S * inside, e_low * inside
    if not upsample:
        return low, e_low
    return bilinear64(low, ih, iw, fused), bilinear64(e_low, ih, iw, fused) + 8 * U32 * bilinear64(S, ih, iw, fused)


def _window64(mh, mw, shape, padding=True):
    gain = min(mh / shape[0], mw / shape[1])
    pad = [mw - shape[1] * gain, mh - shape[0] * gain]
    if padding:
        pad[0] /= 2
        pad[1] /= 2
    top, left = (int(pad[1]), int(pad[0])) if padding else (0, 0)
    return top, left, int(mh - pad[1]), int(mw - pad[0])


def scale_masks64(masks, shape, padding=True, fused=True):
    """scale_masks in float64 -> (v, e) with e = 8 * 2^-24 * interp(|masks|) (four products, three sums)."""
    m = masks.detach().double().numpy()
    top, left, bottom, right = _window64(m.shape[-2], m.shape[-1], shape, padding)
    m = m[..., top:bottom, left:right]
    return bilinear64(m, shape[0], shape[1], fused), 8 * U32 * bilinear64(np.abs(m), shape[0], shape[1], fused)


def process_mask_native64(protos, masks_in, bboxes, shape, fused=True):
    """process_mask_native in float64 -> (v, e); the crop (boxes in output pixels, fp32 comparisons) comes last."""
    c, mh, mw = protos.shape
    low, S, e_low = _lowres64(protos, masks_in)
    top, left, bottom, right = _window64(mh, mw, shape, True)
    w = (slice(None), slice(top, bottom), slice(left, right))
    v = bilinear64(low[w], shape[0], shape[1], fused)
    e = bilinear64(e_low[w], shape[0], shape[1], fused) + 8 * U32 * bilinear64(S[w], shape[0], shape[1], fused)
    inside = crop_inside(bboxes.detach().float(), shape[0], shape[1])
    return v * inside, e * inside


def classify_masks(got, v, e):
    """Compare a 0/1 mask with the float64 reference: (number of mismatching pixels that are NOT ambiguous, number of
    mismatching pixels, ambiguous share of the case).  A pixel is ambiguous iff |v| <= e and e > 0; e == 0 means the
    crop removed every contribution, the value is exactly 0 in any arithmetic and the mask must be 0."""
    got = np.asarray(got)
    amb = (np.abs(v) <= e) & (e > 0)
    diff = (got != 0) != (v > 0)
    return int((diff & ~amb).sum()), int(diff.sum()), float(amb.mean())
