#!/usr/bin/env python3
"""Generate the classification fixtures by RUNNING THE REFERENCE (build container only).

    python tests/golden/make_cls_fixtures.py

The reference is imported in-process with make_fixtures.py's stand-ins (this script imports it for them and for `fill`).  Nothing of
the reference is modified or copied.
  graph_{yolo11n,yolov8n}_cls.npz  ClassificationModel of cfg/models/11/yolo11-cls.yaml / v8/yolov8-cls.yaml, scale n, nc = 10,
           parameters written by fill() (oracle.yolo_ref.synth_param, names stored), the model fused, inputs (1, 64, 64), (2, 96, 128)
           and (1, 224, 224) from seeds (torch.rand on a seeded CPU generator; checksums stored).  224 is the reference's default
           size: a 7 x 7 final map.  Per input: y (the softmax), x (the logits) and the pooled (B, 1280) vector, taken with a forward
           hook on Classify.pool.
  graph_yolo11n_cls1000.npz        the same graph with nc = 1000, the first two inputs.
meta holds the model's BatchNorm eps (1e-5: a ClassificationModel keeps torch's default, where DetectionModel sets 1e-3), which whoever
folds the stored un-fused parameters needs, and the yaml's own `scales`, `backbone` and `head` (yaml.safe_load of the file): what graphs.stock_cfg must restate.
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
from ultralytics.nn.tasks import ClassificationModel  # noqa: E402

SHAPES = [(1, 64, 64), (2, 96, 128), (1, 224, 224)]
FILES = {"yolo11": "11/yolo11-cls.yaml", "yolov8": "v8/yolov8-cls.yaml"}


def graph_fixture(tag, family, nc, shapes, seed=0):
    d = yaml.safe_load(open(MF.CFG / FILES[family]))
    stock = {k: d[k] for k in ("scales", "backbone", "head")}
    d["scale"], d["nc"] = "n", nc
    m = ClassificationModel(d, ch=3, nc=nc, verbose=False).eval()
    names = MF.fill(m, "", seed)
    nparam = sum(p.numel() for p in m.parameters())
    eps = {float(b.eps) for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)}
    assert len(eps) == 1  # 1e-5, torch's default: ClassificationModel._from_yaml does not call initialize_weights (1e-3, tasks.py:324)
    m.fuse(verbose=False)
    pooled = []
    m.model[-1].pool.register_forward_hook(lambda mod, inp, out: pooled.append(out.flatten(1).clone()))
    out, xs = {}, []
    for si, (b, h, w) in enumerate(shapes):
        x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + si))
        xs.append({"sum": float(x.double().sum()), "first": x.flatten()[:8].tolist()})
        with torch.inference_mode():
            y, lg = m(x)
        assert tuple(y.shape) == (b, nc) and tuple(lg.shape) == (b, nc) and tuple(pooled[-1].shape) == (b, 1280)
        out[f"y{si}"], out[f"x{si}"], out[f"pool{si}"] = y.numpy(), lg.numpy(), pooled[-1].numpy()
        top = lg.sort(1, descending=True).values[:, :min(nc, 5) + 1]
        print(tag, si, tuple(y.shape), f"logits {float(lg.min()):.3g} .. {float(lg.max()):.3g}, smallest gap among the top-5 (and to the "
              f"sixth) {float((top[:, :-1] - top[:, 1:]).min()):.3g}")
    out["meta"] = json.dumps({"family": family, "scale": "n", "task": "classify", "nc": nc, "seed": seed, "names": names, "nparam": nparam,
                              "stride": [float(s) for s in m.stride], "bn_eps": eps.pop(), "shapes": shapes, "x": xs, "yaml": stock})
    np.savez_compressed(HERE / f"graph_{tag}.npz", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    graph_fixture("yolo11n_cls", "yolo11", 10, SHAPES)
    graph_fixture("yolov8n_cls", "yolov8", 10, SHAPES)
    graph_fixture("yolo11n_cls1000", "yolo11", 1000, SHAPES[:2])
    for f in ("graph_yolo11n_cls.npz", "graph_yolov8n_cls.npz", "graph_yolo11n_cls1000.npz"):
        print(f, (HERE / f).stat().st_size, "bytes")
