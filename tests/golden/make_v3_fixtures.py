#!/usr/bin/env python3
"""Generate the YOLOv3 graph fixtures by RUNNING THE REFERENCE (build container only; never on the GPU box).

    python tests/golden/make_v3_fixtures.py

The reference is imported in-process with make_fixtures.py's stand-ins (this script imports it for them and for `fill`); nothing of
the reference is modified or copied.
  graph_yolov3_tiny.npz  DetectionModel of cfg/models/v3/yolov3-tiny.yaml, full width           (two levels: strides 16 and 32)
  graph_yolov3.npz       DetectionModel of cfg/models/v3/yolov3.yaml, width_multiple = 0.5      (every width a multiple of 16)
  graph_yolov3_spp.npz   DetectionModel of cfg/models/v3/yolov3-spp.yaml, width_multiple = 0.5
all with nc = 12, parameters written by fill() (oracle.yolo_ref.synth_param, names stored), inputs (1, 64, 64) and (2, 96, 128) from
seeds 100 + si (checksums stored).  Per shape: y, the raw level maps, and non_max_suppression(y, conf, 0.7, nc=12) per image at the
largest conf of 0.25 / 0.1 / 0.01 / 0.001 that keeps a detection (meta["nms_conf"]).  meta["yaml"] is the yaml file as parsed (settings
only: nc = 80, both multiples 1.0), so that a test can compare graphs.stock_cfg with it where the reference is absent.

Damping (meta["damp"] = {"layers": [...], "suffix": ".cv2.conv.weight", "factor": f}), make_v9_fixtures.py / make_ghost_fixtures.py's
rule.  Darknet-53 chains 23 shortcut Bottlenecks (x + cv2(cv1(x))), whose gain under the synthetic fill may exceed 1.  After fill() the
cv2 conv weight of EVERY top-level Bottleneck (a tensor named model.<i>.cv2.conv.weight or model.<i>.<j>.cv2.conv.weight with <i> one of
"layers", the yaml's Bottleneck lines) is multiplied by ONE factor, the largest of 1, 1/2, 1/4, 1/8, 1/16 for which, on both shapes,
(1) every top-level layer's output stays below 256 in magnitude in the reference's fp32 run and (2) the reference's own .half() run is
finite and within HALF of the project's fp16 bounds of its fp32 run (score 5e-3, box 0.5 px, raw maps 1e-2 of the map's maximum).  A
test that regenerates the state dict from synth_param applies the same rule.  meta["ref_fp16"] records that distance of the reference's
own fp16 run.  yolov3-tiny has no Bottleneck: its factor is 1 and the conditions are checked all the same.

meta["ref_conv_gflops_640"][family]: 2 * MAC of every convolution the (fused) reference model runs at 1 x 640 x 640 with nc = 80 at FULL
width, counted from the convs' output shapes (DFL excluded, as in the plan's count).
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
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

NC = 12
SHAPES = [(1, 64, 64), (2, 96, 128)]
LIMIT = 1 << 20
FACTORS = (1.0, 0.5, 0.25, 0.125, 0.0625)
SUFFIX = ".cv2.conv.weight"
YAMLS = {"yolov3": "v3/yolov3.yaml", "yolov3-spp": "v3/yolov3-spp.yaml", "yolov3-tiny": "v3/yolov3-tiny.yaml"}
GRAPHS = [  # tag, family, width_multiple
    ("yolov3_tiny", "yolov3-tiny", 1.0),
    ("yolov3", "yolov3", 0.5),
    ("yolov3_spp", "yolov3-spp", 0.5),
]


def parsed(family):
    return yaml.safe_load(open(MF.CFG / YAMLS[family]))


def build(family, width, nc=NC):
    d = parsed(family)
    d["nc"], d["width_multiple"] = nc, width
    return DetectionModel(d, ch=3, nc=nc, verbose=False).eval()


def bottleneck_layers(family):
    d = parsed(family)
    return [i for i, l in enumerate(d["backbone"] + d["head"]) if l[2] == "Bottleneck"]


def damped(name, layers):
    parts = name.split(".")
    return name.endswith(SUFFIX) and parts[0] == "model" and int(parts[1]) in layers


def filled(family, width, factor, seed=0):
    """(model fused and ready to run, recorded un-fused names, parameter count)"""
    m = build(family, width)
    names = MF.fill(m, "", seed)
    layers = bottleneck_layers(family)
    with torch.no_grad():
        for k, t in m.state_dict().items():
            if damped(k, layers):
                t.mul_(factor)
    nparam = sum(p.numel() for p in m.parameters())
    m.fuse(verbose=False)
    return m, names, nparam


def run(m, x):
    with torch.inference_mode():
        y, raw = m(x)
    return y, raw


def probe(family, width, factor, xs):
    """(conditions hold, fp16-to-fp32 distance of the reference) for one damping factor."""
    m, _, _ = filled(family, width, factor)
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
        ok = all(bool(torch.isfinite(o[0]).all()) for o in outs16) and ds < 5e-3 and db < 0.5 and dr < 1e-2
    return ok, dist


def conv_gflops_640(family):
    """2 * MAC of every conv of the fused full-width reference model at 1 x 640 x 640, nc = 80: counted at 64 x 64 from the output
    shapes and scaled by 100 (every map is even down to the last stride, so the counts scale with the area)."""
    m = build(family, 1.0, nc=80)
    m.fuse(verbose=False)
    total = [0]

    def conv_hook(mod, inp, out):
        total[0] += 2 * out.numel() * mod.in_channels // mod.groups * mod.kernel_size[0] * mod.kernel_size[1]

    for name, mod in m.named_modules():
        if ".dfl" not in name and isinstance(mod, torch.nn.Conv2d):
            mod.register_forward_hook(conv_hook)
    with torch.inference_mode():
        m(torch.zeros(1, 3, 64, 64))
    return total[0] * 100 / 1e9


def graph_fixture(tag, family, width, gflops, seed=0):
    xs, xmeta = [], []
    for si, (b, h, w) in enumerate(SHAPES):
        x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + si))
        xs.append(x)
        xmeta.append({"sum": float(x.double().sum()), "first": x.flatten()[:8].tolist()})
    layers = bottleneck_layers(family)
    for factor in FACTORS if layers else FACTORS[:1]:
        ok, dist = probe(family, width, factor, xs)
        print(tag, "factor", factor, "ok" if ok else "no", dist)
        if ok:
            break
    assert ok, (tag, "no damping factor meets the conditions")
    m, names, nparam = filled(family, width, factor, seed)
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
    meta = {"family": family, "scale": None, "width_multiple": width, "task": "detect", "nc": NC, "seed": seed, "names": names, "nparam": nparam,
            "stride": [float(s) for s in m.stride], "shapes": SHAPES, "x": xmeta, "nms_conf": conf, "nms_iou": 0.7, "raw_shapes": [0, 1],
            "damp": {"layers": layers, "suffix": SUFFIX, "factor": factor}, "ref_fp16": dist, "ref_conv_gflops_640": gflops,
            "yaml": parsed(family)}
    path = HERE / f"graph_{tag}.npz"
    np.savez_compressed(path, **out, **raws, meta=json.dumps(meta))
    assert path.stat().st_size < LIMIT, (tag, path.stat().st_size)
    print(tag, path.stat().st_size, "bytes,", nparam, "parameters")


if __name__ == "__main__":
    torch.set_num_threads(8)
    gflops = {fam: round(conv_gflops_640(fam), 4) for fam in YAMLS}
    print("reference conv GFLOPs at 640 x 640, nc = 80:", gflops)
    for g in GRAPHS:
        graph_fixture(*g, gflops)
