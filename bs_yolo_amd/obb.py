"""OBBPredictor.postprocess (models/yolo/obb/predict.py:27-53) over the HIP kernels, for a whole batch.

``nms.nms_rotated_batched`` gives the device-resident (det, counts) of non_max_suppression(rotated=True); ``postprocess`` then
applies regularize_rboxes + scale_boxes(xywh=True) + clip_boxes (utils/ops.py:775-791, :92-127, :319-338) to every kept row in one
launch (bsy_obb_scale) and slices the per-image results in the column order ``Results(obb=...)`` takes: [x, y, w, h, theta, conf,
cls].  One host synchronisation, for the slicing.
"""
from __future__ import annotations

import ctypes as C
from typing import List

import torch

from . import lib as L
from .nms import scale_params


def scale_batched(det: torch.Tensor, counts: torch.Tensor, img1_shape, img0_shapes, ratio_pads=None) -> torch.Tensor:
    """In place on bsy_nms_rotated's rows (B, max_det, 7) [x, y, w, h, conf, cls, theta]: regularised, scaled to the original
    images and clipped.  Gain / pads per image from the host, with the reference's Python arithmetic (round())."""
    B, max_det, row = det.shape
    t = scale_params(B, img1_shape, img0_shapes, ratio_pads, det.device)
    stream = L.stream_ptr(det.device)
    L.check(L.lib.bsy_obb_scale(C.c_void_p(det.data_ptr()), C.c_void_p(counts.data_ptr()), B, max_det, row,
                                C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()), C.c_void_p(t[2].data_ptr()),
                                C.c_void_p(t[3].data_ptr()), C.c_void_p(t[4].data_ptr()), stream))
    return det


def postprocess(det: torch.Tensor, counts: torch.Tensor, img1_shape, img0_shapes, ratio_pads=None) -> List[torch.Tensor]:
    """-> per image an (n, 7) f32 tensor [x, y, w, h, theta, conf, cls] in original-image pixels (predict.py:48-51).  `det` is
    modified in place."""
    if det.dim() != 3 or det.shape[-1] != 7:
        raise ValueError("det must be bsy_nms_rotated's (B, max_det, 7) rows of a one-angle OBB head")
    scale_batched(det, counts, img1_shape, img0_shapes, ratio_pads)
    order = torch.tensor([0, 1, 2, 3, 6, 4, 5], device=det.device)
    out = det.index_select(2, order)
    return [out[b, :k] for b, k in enumerate(counts.tolist())]
