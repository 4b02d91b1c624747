#!/usr/bin/env python3
"""Generate the whole-graph pose fixtures by RUNNING THE REFERENCE (build container only).

    python tests/golden/make_pose_graph_fixtures.py

The reference is imported in-process with make_fixtures.py's stand-ins (this script imports it for them and for `fill`).  Nothing of
the reference is modified or copied.  Every file is a PoseModel built from one of the reference's pose yamls, parameters written by
fill() (oracle.yolo_ref.synth_param, names stored), the model fused, inputs from seeds (torch.rand on a seeded CPU generator; checksums
stored):
  graph_yolo11n_pose.npz     11/yolo11-pose.yaml    n, nc 1, kpt_shape (17, 3), (1, 64, 64) and (2, 96, 128): cv4 is 51 channels wide
  graph_yolov8n_pose.npz     v8/yolov8-pose.yaml    n, nc 1, kpt_shape (17, 3), the same inputs
  graph_yolo11n_pose_k5.npz  11/yolo11-pose.yaml    n, nc 3, kpt_shape (5, 2): no visibility row, 10 keypoint channels
  graph_yolo11m_pose.npz     11/yolo11-pose.yaml    m, nc 1, kpt_shape (17, 3), (1, 64, 64): cv4 is 64 channels wide
  graph_yolov8n_pose_p6.npz  v8/yolov8-pose-p6.yaml n, nc 1, kpt_shape (17, 3), (1, 64, 64) and (1, 128, 64): four levels
Per input: y, kpt (the raw keypoint logits Pose.forward returns) and the raw level maps (those of the larger input are dropped where
the file would pass 1 MiB).  meta holds the yaml's own `scales`, `backbone`, `head` and `kpt_shape` (yaml.safe_load of the file): what
graphs.stock_cfg must restate; the BatchNorm eps; and `nms_conf`: the largest confidence threshold of LADDER at which
non_max_suppression(y, conf, 0.7, nc=nc) keeps between 5 and 300 rows for EVERY image of the file (asserted here, counts printed),
so that an NMS test on these graphs cannot pass empty or saturated.
"""
import copy
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_fixtures as MF  # noqa: E402  (stand-ins + the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402
from ultralytics.nn.tasks import PoseModel  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

LIMIT = 1 << 20
SMALL = [(1, 64, 64), (2, 96, 128)]
LADDER = [0.25, 0.1, 0.05, 0.02, 0.01, 5e-3, 2e-3, 1e-3, 5e-4, 2e-4, 1e-4, 5e-5, 2e-5, 1e-5, 1e-6, 1e-7]
GRAPHS = [  # tag, yaml, family (bs_yolo_amd.graphs), scale, nc, kpt_shape, shapes
    ("yolo11n_pose", "11/yolo11-pose.yaml", "yolo11", "n", 1, (17, 3), SMALL),
    ("yolov8n_pose", "v8/yolov8-pose.yaml", "yolov8", "n", 1, (17, 3), SMALL),
    ("yolo11n_pose_k5", "11/yolo11-pose.yaml", "yolo11", "n", 3, (5, 2), SMALL),
    ("yolo11m_pose", "11/yolo11-pose.yaml", "yolo11", "m", 1, (17, 3), SMALL[:1]),
    ("yolov8n_pose_p6", "v8/yolov8-pose-p6.yaml", "yolov8-p6", "n", 1, (17, 3), [(1, 64, 64), (1, 128, 64)]),
]


def graph_fixture(tag, cfg, family, scale, nc, kpt_shape, shapes, seed=0):
    d = yaml.safe_load(open(MF.CFG / cfg))
    stock = copy.deepcopy({k: d[k] for k in ("scales", "backbone", "head", "kpt_shape")})
    d["scale"], d["nc"] = scale, nc
    m = PoseModel(d, ch=3, nc=nc, data_kpt_shape=kpt_shape, verbose=False).eval()
    assert tuple(m.model[-1].kpt_shape) == tuple(kpt_shape)
    names = MF.fill(m, "", seed)
    nparam = sum(p.numel() for p in m.parameters())
    eps = {float(b.eps) for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)}
    assert len(eps) == 1
    m.fuse(verbose=False)
    nk = kpt_shape[0] * kpt_shape[1]
    out, xs, ys, raws = {}, [], [], {}
    for si, (b, h, w) in enumerate(shapes):
        x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + si))
        xs.append({"sum": float(x.double().sum()), "first": x.flatten()[:8].tolist()})
        with torch.inference_mode():
            y, (raw, kpt) = m(x)
        assert tuple(y.shape) == (b, 4 + nc + nk, kpt.shape[-1]) and tuple(kpt.shape[:2]) == (b, nk)
        out[f"y{si}"], out[f"kpt{si}"] = y.numpy(), kpt.numpy()
        ys.append(y)
        for li, r in enumerate(raw):
            raws[f"raw{si}_{li}"] = r.numpy()
    conf, counts = None, None
    for c in LADDER:
        with torch.inference_mode():
            counts = [[len(r) for r in rops.non_max_suppression(y.clone(), c, 0.7, nc=nc)] for y in ys]
        if all(5 <= n <= 300 for per in counts for n in per):
            conf = c
            break
    assert conf is not None, (tag, "no threshold of LADDER keeps 5 .. 300 rows for every image", counts)
    print(tag, "nms conf", conf, "rows kept per image", counts)
    meta = {"family": family, "scale": scale, "task": "pose", "nc": nc, "kpt_shape": list(kpt_shape), "seed": seed, "names": names,
            "nparam": nparam, "stride": [float(s) for s in m.stride], "bn_eps": eps.pop(), "shapes": [list(s) for s in shapes], "x": xs,
            "yaml": stock, "nms_conf": conf, "nms_iou": 0.7, "nms_counts": counts, "raw_shapes": list(range(len(shapes)))}
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
