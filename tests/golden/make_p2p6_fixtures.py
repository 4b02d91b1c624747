#!/usr/bin/env python3
"""Generate the four-level (P2 / P6) graph fixtures by RUNNING THE REFERENCE (build container only).

    python tests/golden/make_p2p6_fixtures.py

The reference is imported in-process with make_fixtures.py's stand-ins (this script imports it for them and for `fill`); nothing of
the reference is modified or copied.
  graph_yolov8n_p2.npz      DetectionModel of cfg/models/v8/yolov8-p2.yaml      (Detect on strides 4, 8, 16, 32)
  graph_yolov8n_p6.npz      DetectionModel of cfg/models/v8/yolov8-p6.yaml      (Detect on strides 8, 16, 32, 64)
  graph_yolov5n_p6.npz      DetectionModel of cfg/models/v5/yolov5-p6.yaml
  graph_yolov8n_seg_p6.npz  SegmentationModel of cfg/models/v8/yolov8-seg-p6.yaml
all at scale n with nc = 12 (the fork's own class count), parameters written by fill() (oracle.yolo_ref.synth_param, names stored),
inputs (1, 64, 64) and (2, 96, 128) for P2 / (2, 128, 192) for P6 from seeds (torch.rand on a seeded CPU generator; checksums
stored).  Per shape: y, the four raw level maps (shape 0 only where the file would pass 1 MiB), for Segment mc and proto, and
non_max_suppression(y, conf, 0.7, nc=12) per image; for yolov8n_p6 also _predict_augment's output (model(x, augment=True)) on
shape 1.  conf is 0.25 unless no graph would keep a detection at it (synthetic head scores are low): then the largest of 0.25,
0.1, 0.01, 0.001 at which the graph keeps one; the value used is in meta["nms_conf"].
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_fixtures as MF  # noqa: E402  (stand-ins + the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402
from ultralytics.nn.tasks import DetectionModel, SegmentationModel  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

NC = 12
P2_SHAPES = [(1, 64, 64), (2, 96, 128)]
P6_SHAPES = [(1, 64, 64), (2, 128, 192)]
LIMIT = 1 << 20
GRAPHS = [  # tag, yaml, family (bs_yolo_amd.graphs), task, shapes, augment
    ("yolov8n_p2", "v8/yolov8-p2.yaml", "yolov8-p2", "detect", P2_SHAPES, False),
    ("yolov8n_p6", "v8/yolov8-p6.yaml", "yolov8-p6", "detect", P6_SHAPES, True),
    ("yolov5n_p6", "v5/yolov5-p6.yaml", "yolov5-p6", "detect", P6_SHAPES, False),
    ("yolov8n_seg_p6", "v8/yolov8-seg-p6.yaml", "yolov8-p6", "segment", P6_SHAPES, False),
]


def graph_fixture(tag, cfg, family, task, shapes, augment, seed=0):
    d = yaml.safe_load(open(MF.CFG / cfg))
    d["scale"], d["nc"] = "n", NC
    m = (DetectionModel if task == "detect" else SegmentationModel)(d, ch=3, nc=NC, verbose=False).eval()
    names = MF.fill(m, "", seed)
    nparam = sum(p.numel() for p in m.parameters())
    m.fuse(verbose=False)
    out, xs, ys, raws = {}, [], [], {}
    for si, (b, h, w) in enumerate(shapes):
        x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + si))
        xs.append({"sum": float(x.double().sum()), "first": x.flatten()[:8].tolist()})
        with torch.inference_mode():
            res = m(x)
            if task == "detect":
                y, raw = res
            else:
                y, (raw, mc, proto) = res
                assert torch.equal(y[:, 4 + NC:], mc)
                out[f"mc{si}"], out[f"proto{si}"] = mc.numpy(), proto.numpy()
            if augment and si == 1:
                ya, aux = m(x, augment=True)
                assert aux is None
                out[f"aug{si}"] = ya.numpy()
        assert len(raw) == 4
        out[f"y{si}"] = y.numpy()
        ys.append(y)
        for li, r in enumerate(raw):
            raws[f"raw{si}_{li}"] = r.numpy()
    # conf as in make_obb_fixtures.py: 0.25 where the graph keeps detections at it, else the largest lower value at which it does
    conf = 0.25
    for conf in (0.25, 0.1, 0.01, 0.001):
        with torch.inference_mode():
            dets = [rops.non_max_suppression(y.clone(), conf, 0.7, nc=NC) for y in ys]
        if sum(len(r) for dd in dets for r in dd) > 0:
            break
    for si, dd in enumerate(dets):
        for bi, r in enumerate(dd):
            out[f"nms{si}_{bi}"] = r.numpy()
        print(tag, si, tuple(ys[si].shape), "conf", conf, "detections", [len(r) for r in dd])
    meta = {"family": family, "scale": "n", "task": task, "nc": NC, "seed": seed, "names": names, "nparam": nparam,
            "stride": [float(s) for s in m.stride], "shapes": shapes, "x": xs, "nms_conf": conf, "nms_iou": 0.7, "raw_shapes": [0, 1]}
    path = HERE / f"graph_{tag}.npz"
    np.savez_compressed(path, **out, **raws, meta=json.dumps(meta))
    if path.stat().st_size >= LIMIT:  # keep the file under the size the other goldens keep: raw maps of shape 0 only
        meta["raw_shapes"] = [0]
        np.savez_compressed(path, **out, **{k: v for k, v in raws.items() if k.startswith("raw0_")}, meta=json.dumps(meta))
    assert path.stat().st_size < LIMIT, (tag, path.stat().st_size)
    print(tag, path.stat().st_size, "bytes, raw maps of shapes", meta["raw_shapes"])


if __name__ == "__main__":
    torch.set_num_threads(8)
    for g in GRAPHS:
        graph_fixture(*g)
