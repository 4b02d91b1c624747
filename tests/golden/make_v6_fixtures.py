#!/usr/bin/env python3
"""Generate the YOLOv6 graph fixtures by RUNNING THE REFERENCE (build container only; never on the GPU box).

    python tests/golden/make_v6_fixtures.py

The reference is imported in-process with make_fixtures.py's stand-ins (this script imports it for them and for `fill`); nothing of
the reference is modified or copied.
  graph_yolov6n.npz           DetectionModel of cfg/models/v6/yolov6.yaml at scale n, AS THIS FORK BUILDS IT: `activation: nn.ReLU()` reaches the
                              top-level Convs and the Detect head; SPPF's cv1 / cv2 stay SiLU (nn/modules/block.py:13 shadows Conv for every
                              class of block.py, parse_model sets default_act on nn.modules.conv.Conv alone).  meta["sppf_act"] = "silu"
  graph_yolov6n_upstream.npz  the same weights with model.9.cv1.act / cv2.act set to nn.ReLU() on the live module before the run: the form an
                              upstream-pickled checkpoint has.  meta["sppf_act"] = "relu"
  graph_yolov6m.npz           scale m (depth 0.67: chains of 4 / 8 / 12 / 4 in the backbone and 6 in the neck; max_channels 768) with the
                              width multiple of its `scales` entry set to 0.25, at which every width (16, 32, 64, 128, 192) is a multiple
                              of 16 and the last stage is cut by max_channels (1024 -> 768 before scaling).  meta["width_multiple"] = 0.25
all with nc = 12, parameters written by fill() (oracle.yolo_ref.synth_param, names stored), inputs (1, 64, 64) and (2, 96, 128) from
seeds 100 + si (checksums stored).  Per shape: y, the raw level maps, and non_max_suppression(y, conf, 0.7, nc=12) per image at the
largest conf of 0.25 / 0.1 / 0.01 / 0.001 that keeps a detection (meta["nms_conf"]).  meta["yaml"] is the yaml file as parsed (nc = 80,
the scales table as shipped), so that a test can compare graphs.stock_cfg with it where the reference is absent.

Admission, make_v3_fixtures.py's rule: on both shapes (1) every top-level layer's output stays below 256 in magnitude in the reference's
fp32 run and (2) the reference's own .half() run is finite and within HALF of the project's fp16 bounds of its fp32 run (score 5e-3, box
0.5 px, raw maps 5e-3 of the map's maximum).  meta["ref_fp16"] records that distance and the largest layer output.
Damping (meta["damp"] = {"prefix": "model.28.cv", "suffix": ".2.weight", "factor": f}).  YOLOv6 has no residual chain whose gain could
grow, and under the plain synthetic fill its largest layer output is 12.4; but the reference's own fp16 run then moves a box by 0.53 px
(yolov6n; score 2.7e-3, raw 1.4e-3) and at scale m a score by 5.6e-3 and a box by 0.73 px, past condition (2).  A box is stride x the DFL
expectation of 16 logits and a score the sigmoid of one, so both distances scale with the gain of the logits: after fill() the weight of
the LAST conv of every Detect branch (the six tensors model.28.cv2.<l>.2.weight and model.28.cv3.<l>.2.weight) is multiplied by ONE
factor, the largest of 1, 1/2, 1/4, 1/8, 1/16 for which both conditions hold (each graph finds its own, as in make_v3_fixtures.py).  A
test that regenerates the state dict from synth_param applies the same rule.

Building a YOLOv6 model sets Conv.default_act = nn.ReLU() on the CLASS for the rest of the process (tasks.py:956-957): every build here
puts nn.SiLU() back in a `finally`, so that nothing built later in the same process inherits ReLU.
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
from ultralytics.nn.modules.conv import Conv  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

NC = 12
SHAPES = [(1, 64, 64), (2, 96, 128)]
LIMIT = 1 << 20
SPPF = 9  # the yaml's SPPF layer
FACTORS = (1.0, 0.5, 0.25, 0.125, 0.0625)
DAMP = {"prefix": "model.28.cv", "suffix": ".2.weight"}
GRAPHS = [  # tag, scale, width multiple written into the scales entry (None: as shipped), SPPF form
    ("yolov6n", "n", None, "silu"),
    ("yolov6n_upstream", "n", None, "relu"),
    ("yolov6m", "m", 0.25, "silu"),
]


def parsed():
    return yaml.safe_load(open(MF.CFG / "v6" / "yolov6.yaml"))


def build(scale, width, nc=NC):
    d = parsed()
    d["nc"], d["scale"] = nc, scale
    if width is not None:
        d["scales"][scale][1] = width
    try:
        return DetectionModel(d, ch=3, nc=nc, verbose=False).eval()
    finally:
        Conv.default_act = torch.nn.SiLU()


def damped(name):
    return name.startswith(DAMP["prefix"]) and name.endswith(DAMP["suffix"])


def filled(scale, width, sppf_act, factor, seed=0):
    """(model fused and ready to run, recorded un-fused names, parameter count)"""
    m = build(scale, width)
    names = MF.fill(m, "", seed)
    with torch.no_grad():
        hit = [t.mul_(factor) for k, t in m.state_dict().items() if damped(k)]
    assert len(hit) == 6
    acts = {type(mod.act).__name__ for mod in m.modules() if isinstance(getattr(mod, "act", None), torch.nn.Module) and hasattr(mod, "conv")}
    assert isinstance(m.model[SPPF].cv1.act, torch.nn.SiLU) and isinstance(m.model[SPPF].cv2.act, torch.nn.SiLU) and acts == {"ReLU", "SiLU"}
    assert isinstance(m.model[0].act, torch.nn.ReLU) and isinstance(m.model[-1].cv2[0][0].act, torch.nn.ReLU)
    if sppf_act == "relu":
        m.model[SPPF].cv1.act = torch.nn.ReLU()
        m.model[SPPF].cv2.act = torch.nn.ReLU()
    nparam = sum(p.numel() for p in m.parameters())
    m.fuse(verbose=False)
    return m, names, nparam


def run(m, x):
    with torch.inference_mode():
        y, raw = m(x)
    return y, raw


def probe(scale, width, sppf_act, factor, xs):
    """(conditions hold, fp16-to-fp32 distance of the reference) for one damping factor."""
    m, _, _ = filled(scale, width, sppf_act, factor)
    peak = [0.0]
    hooks = [layer.register_forward_hook(lambda mod, inp, o: peak.__setitem__(0, max(peak[0], float(o.abs().max())))
                                         if isinstance(o, torch.Tensor) else None) for layer in list(m.model)[:-1]]
    outs32 = [run(m, x) for x in xs]
    for h in hooks:
        h.remove()
    ok = peak[0] < 256.0 and all(bool(torch.isfinite(o[0]).all()) for o in outs32)
    dist = {"score": float("nan"), "box": float("nan"), "raw": float("nan"), "layer_max": peak[0]}
    if ok:
        mh = m.half()
        outs16 = [run(mh, x.half()) for x in xs]
        ds = max(float((a[0][:, 4:4 + NC].float() - b[0][:, 4:4 + NC]).abs().max()) for a, b in zip(outs16, outs32))
        db = max(float((a[0][:, :4].float() - b[0][:, :4]).abs().max()) for a, b in zip(outs16, outs32))
        dr = max(float((ra.float() - rb_).abs().max() / rb_.abs().max()) for a, b in zip(outs16, outs32) for ra, rb_ in zip(a[1], b[1]))
        dist.update(score=ds, box=db, raw=dr)
        ok = all(bool(torch.isfinite(o[0]).all()) for o in outs16) and ds < 5e-3 and db < 0.5 and dr < 5e-3
    return ok, dist


def graph_fixture(tag, scale, width, sppf_act, seed=0):
    xs, xmeta = [], []
    for si, (b, h, w) in enumerate(SHAPES):
        x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + si))
        xs.append(x)
        xmeta.append({"sum": float(x.double().sum()), "first": x.flatten()[:8].tolist()})
    for factor in FACTORS:
        ok, dist = probe(scale, width, sppf_act, factor, xs)
        print(tag, "factor", factor, "ok" if ok else "no", dist)
        if ok:
            break
    assert ok, (tag, "no damping factor meets the conditions")
    m, names, nparam = filled(scale, width, sppf_act, factor, seed)
    out, ys, raws = {}, [], {}
    for si, x in enumerate(xs):
        y, raw = run(m, x)
        assert len(raw) == len(m.stride)
        out[f"y{si}"] = y.numpy()
        ys.append(y)
        for li, r in enumerate(raw):
            raws[f"raw{si}_{li}"] = r.numpy()
    for conf in (0.25, 0.1, 0.01, 0.001):
        with torch.inference_mode():
            dets = [rops.non_max_suppression(y.clone(), conf, 0.7, nc=NC) for y in ys]
        if sum(len(r) for dd in dets for r in dd) > 0:
            break
    for si, dd in enumerate(dets):
        for bi, r in enumerate(dd):
            out[f"nms{si}_{bi}"] = r.numpy()
        print(tag, si, tuple(ys[si].shape), "conf", conf, "detections", [len(r) for r in dd], "max score", float(ys[si][:, 4:4 + NC].max()))
    d = parsed()
    meta = {"family": "yolov6", "scale": scale, "width_multiple": width, "depth_multiple": d["scales"][scale][0], "task": "detect", "nc": NC,
            "seed": seed, "names": names, "nparam": nparam, "sppf_act": sppf_act, "stride": [float(s) for s in m.stride], "shapes": SHAPES,
            "x": xmeta, "nms_conf": conf, "nms_iou": 0.7, "raw_shapes": [0, 1], "damp": dict(DAMP, factor=factor), "ref_fp16": dist, "yaml": d}
    path = HERE / f"graph_{tag}.npz"
    np.savez_compressed(path, **out, **raws, meta=json.dumps(meta))
    assert path.stat().st_size < LIMIT, (tag, path.stat().st_size)
    print(tag, path.stat().st_size, "bytes,", nparam, "parameters")
    return ys


if __name__ == "__main__":
    torch.set_num_threads(8)
    ys = {g[0]: graph_fixture(*g) for g in GRAPHS}
    # what makes the sppf_act tests meaningful: the two forms of the same weights differ by far more than the fp16 bounds
    for si, (a, b) in enumerate(zip(ys["yolov6n"], ys["yolov6n_upstream"])):
        print("fork vs upstream form, shape", si, "score", float((a[:, 4:] - b[:, 4:]).abs().max()), "box", float((a[:, :4] - b[:, :4]).abs().max()))
    assert isinstance(Conv.default_act, torch.nn.SiLU)
