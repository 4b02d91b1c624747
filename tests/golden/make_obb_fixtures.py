#!/usr/bin/env python3
"""Generate the OBB fixtures by RUNNING THE REFERENCE (build container only).

    python tests/golden/make_obb_fixtures.py

The reference is imported in-process with make_fixtures.py's stand-ins (this script imports it for them and for `fill`).  The fork's
utils/ops.py leaves its `batch_probiou` import commented out (ops.py:14), so nms_rotated (:146-164) raises NameError as shipped;
the name is bound here to the reference's own utils.metrics.batch_probiou, the same kind of binding make_fixtures.py makes for
torchvision.ops.nms.  Nothing of the reference is modified or copied.
  graph_{yolo11n,yolov8n}_obb.npz  OBBModel of cfg/models/11/yolo11-obb.yaml / v8/yolov8-obb.yaml, scale n, nc = 15 (DOTA),
           parameters written by fill() (oracle.yolo_ref.synth_param, names stored), inputs (1, 64, 64) and (2, 96, 128) from seeds
           (torch.rand on a seeded CPU generator; checksums stored): y, the raw level maps, the angle, and
           non_max_suppression(y, conf, 0.7, nc=15, rotated=True) per image (conf 0.25 for yolo11n; 0.001 for yolov8n, whose
           synthetic head scores stay below 0.01).
  obb_nms.npz    non_max_suppression(rotated=True) on seeded synthetic (B, 4 + nc + 1, A) predictions (CASES below).
  obb_scale.npz  regularize_rboxes + scale_boxes(xywh=True), chained as OBBPredictor.postprocess does (obb/predict.py:48-51), on
           seeded rows [x, y, w, h, conf, cls, theta].
"""
import json
import math
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_fixtures as MF  # noqa: E402  (stand-ins + the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402
from ultralytics.nn.tasks import OBBModel  # noqa: E402
from ultralytics.utils import metrics as rmetrics, ops as rops  # noqa: E402

rops.batch_probiou = rmetrics.batch_probiou  # ops.py:14: unbound in the fork

NC = 15
SHAPES = [(1, 64, 64), (2, 96, 128)]


def graph_fixture(tag, family, conf, seed=0):
    d = yaml.safe_load(open(MF.CFG / ("11/yolo11-obb.yaml" if family == "yolo11" else "v8/yolov8-obb.yaml")))
    d["scale"], d["nc"] = "n", NC
    m = OBBModel(d, ch=3, nc=NC, verbose=False).eval()
    names = MF.fill(m, "", seed)
    nparam = sum(p.numel() for p in m.parameters())
    m.fuse(verbose=False)
    out, xs = {}, []
    for si, (b, h, w) in enumerate(SHAPES):
        x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + si))
        xs.append({"sum": float(x.double().sum()), "first": x.flatten()[:8].tolist()})
        with torch.inference_mode():
            y, (raw, angle) = m(x)
            dets = rops.non_max_suppression(y.clone(), conf, 0.7, nc=NC, rotated=True)
        assert torch.equal(y[:, -1:], angle)
        out[f"y{si}"] = y.numpy()
        out[f"angle{si}"] = angle.numpy()
        for li, r in enumerate(raw):
            out[f"raw{si}_{li}"] = r.numpy()
        for bi, r in enumerate(dets):
            out[f"nms{si}_{bi}"] = r.numpy()
        print(tag, si, tuple(y.shape), "detections", [len(r) for r in dets])
    out["meta"] = json.dumps({"family": family, "scale": "n", "task": "obb", "nc": NC, "seed": seed, "names": names, "nparam": nparam,
                              "stride": [float(s) for s in m.stride], "shapes": SHAPES, "x": xs, "nms_conf": conf, "nms_iou": 0.7})
    np.savez_compressed(HERE / f"graph_{tag}.npz", **out)


def obb_pred(b, nc, a, seed, spread=600.0, size=(6.0, 120.0), jitter=4.0, peaky=True):
    """(B, 4 + nc + 1, A) OBB prediction: clusters of jittered copies of random rotated boxes, class scores, the angle row last."""
    g = torch.Generator().manual_seed(seed)
    base = max(a // 8, 1)
    cx, cy = torch.rand(b, base, generator=g) * spread + 20, torch.rand(b, base, generator=g) * spread + 20
    w, h = torch.rand(b, base, generator=g) * size[1] + size[0], torch.rand(b, base, generator=g) * size[1] + size[0]
    t = (torch.rand(b, base, generator=g) - 0.25) * math.pi
    rep = (a + base - 1) // base
    jit = lambda v, s: v.repeat(1, rep)[:, :a] + torch.randn(b, a, generator=g) * s  # noqa: E731
    box = torch.stack((jit(cx, jitter), jit(cy, jitter), jit(w, jitter).abs() + 2, jit(h, jitter).abs() + 2), 1)
    ang = jit(t, 0.15)[:, None]
    cls = torch.rand(b, nc, a, generator=g) ** 8 if peaky else torch.rand(b, nc, a, generator=g) * 0.6
    return torch.cat([box, cls, ang], 1)


def chain_pred():
    """Three 40 x 20 boxes 12 px apart: probiou 0.645 between neighbours, 0.354 between the outer two -- at thr 0.5 fast-NMS keeps
    only the first (greedy NMS would keep the first and the third)."""
    p = torch.zeros(1, 4 + 2 + 1, 3)
    p[0, 0] = torch.tensor([100.0, 112.0, 124.0])
    p[0, 1] = 100.0
    p[0, 2], p[0, 3] = 40.0, 20.0
    p[0, 4] = torch.tensor([0.9, 0.8, 0.7])
    p[0, 5] = 0.1
    return p


CASES = [  # tag, prediction, kwargs of non_max_suppression (rotated=True added); sizes keep the file under 1 MiB
    ("chain", lambda: chain_pred(), dict(conf_thres=0.25, iou_thres=0.5, nc=2)),
    ("dense", lambda: obb_pred(2, 8, 1200, 1, spread=300.0), dict(conf_thres=0.25, iou_thres=0.7, nc=8)),
    ("dense_low_iou", lambda: obb_pred(2, 8, 800, 2, spread=200.0), dict(conf_thres=0.2, iou_thres=0.3, nc=8)),
    ("agnostic", lambda: obb_pred(2, 8, 800, 3), dict(conf_thres=0.2, iou_thres=0.5, agnostic=True, nc=8)),
    ("classes", lambda: obb_pred(2, 8, 800, 4), dict(conf_thres=0.2, iou_thres=0.5, classes=[1, 3, 6], nc=8)),
    ("multi_label", lambda: obb_pred(2, 6, 600, 5, peaky=False), dict(conf_thres=0.3, iou_thres=0.6, multi_label=True, nc=6)),
    ("max_det", lambda: obb_pred(1, 8, 1000, 6), dict(conf_thres=0.1, iou_thres=0.7, max_det=20, nc=8)),
    ("iou0", lambda: obb_pred(1, 8, 200, 7), dict(conf_thres=0.2, iou_thres=0.0, nc=8)),
    ("iou1", lambda: obb_pred(1, 8, 200, 8), dict(conf_thres=0.2, iou_thres=1.0, nc=8)),
    ("empty", lambda: obb_pred(2, 8, 100, 9), dict(conf_thres=0.9999, iou_thres=0.7, nc=8)),
    ("zero_wh", None, dict(conf_thres=0.2, iou_thres=0.7, nc=8)),
    ("fp16", lambda: obb_pred(2, NC, 1000, 11).half(), dict(conf_thres=0.25, iou_thres=0.7, nc=NC)),
    ("max_nms_cap", lambda: obb_pred(1, 4, 1600, 12, peaky=False), dict(conf_thres=0.05, iou_thres=0.7, max_nms=1000, nc=4)),
]


def zero_wh_pred():
    """Zero-width / zero-height boxes, axis-aligned: at a general angle a degenerate box's covariance determinant is zero only up to
    rounding, and its sign -- a NaN probiou (suppress) or a finite one -- then hangs on the last ulp of cos / sin, which no two
    libms share."""
    p = obb_pred(1, 8, 600, 10, spread=200.0)
    for sl, rows in ((slice(0, None, 5), [2]), (slice(1, None, 7), [3]), (slice(2, None, 11), [2, 3])):
        for r in rows:
            p[:, r, sl] = 0.0  # zero width / height / both
        p[:, -1, sl] = 0.0
    return p


def nms_fixtures():
    out, cfgs = {}, []
    for tag, make, kw in CASES:
        pred = zero_wh_pred() if tag == "zero_wh" else make()
        # fp16 predictions: the reference on their exact fp32 values (its fp16 CPU path overflows cls * max_wh); the kernel upcasts
        res = rops.non_max_suppression(pred.float().clone(), rotated=True, **kw)
        out[tag + ".pred"] = pred.numpy()
        for i, r in enumerate(res):
            out[f"{tag}.out{i}"] = r.numpy()
        cfgs.append((tag, kw, len(res)))
        print("nms", tag, tuple(pred.shape), [len(r) for r in res])
    out["cases"] = json.dumps(cfgs)
    np.savez_compressed(HERE / "obb_nms.npz", **out)


def scale_fixtures():
    g = torch.Generator().manual_seed(21)
    cases = [((640, 640), (480, 640), None), ((1024, 1024), (3000, 4000), None), ((640, 480), (1080, 810), None),
             ((1024, 1024), (1024, 1024), None), ((640, 640), (333, 500), ((0.9, 0.9), (12.5, 3.0))),
             ((1024, 768), (2048, 1536), ((0.5, 0.5), (0, 0)))]
    out, cfg = {}, []
    for ci, (s1, s0, rp) in enumerate(cases):
        n = 96
        rows = torch.zeros(n, 7)
        rows[:, 0] = torch.rand(n, generator=g) * (s1[1] + 200) - 100   # centres, some outside the image
        rows[:, 1] = torch.rand(n, generator=g) * (s1[0] + 200) - 100
        rows[:, 2] = torch.rand(n, generator=g) * 300 + 1
        rows[:, 3] = torch.rand(n, generator=g) * 300 + 1
        rows[::6, 3] = rows[::6, 2]                                      # h == w (swapped: h >= w)
        rows[:, 4] = torch.rand(n, generator=g)
        rows[:, 5] = torch.randint(0, NC, (n,), generator=g).float()
        rows[:, 6] = (torch.rand(n, generator=g) - 0.25) * math.pi
        rows[1::8, 6] = torch.tensor([0.0, 1e-8, -1e-8, math.pi / 2, -math.pi / 4, 3 * math.pi / 4, 3.1415925, 3.1415927,
                                      -3e-7, math.pi / 2 - 1e-7, 1.5707964, 2.0][: len(rows[1::8])])
        rb = rops.regularize_rboxes(torch.cat([rows[:, :4], rows[:, -1:]], dim=-1))
        rb[:, :4] = rops.scale_boxes(s1, rb[:, :4], s0, ratio_pad=rp, xywh=True)
        out[f"case{ci}.rows"] = rows.numpy()
        out[f"case{ci}.obb"] = torch.cat([rb, rows[:, 4:6]], dim=-1).numpy()
        cfg.append((s1, s0, rp))
    out["cases"] = json.dumps(cfg)
    np.savez_compressed(HERE / "obb_scale.npz", **out)
    print("scale", len(cases), "cases")


if __name__ == "__main__":
    torch.set_num_threads(8)
    graph_fixture("yolo11n_obb", "yolo11", 0.25)
    graph_fixture("yolov8n_obb", "yolov8", 0.001)
    nms_fixtures()
    scale_fixtures()
    for f in ("graph_yolo11n_obb.npz", "graph_yolov8n_obb.npz", "obb_nms.npz", "obb_scale.npz"):
        print(f, (HERE / f).stat().st_size, "bytes")
