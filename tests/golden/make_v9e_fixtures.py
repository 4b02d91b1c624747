#!/usr/bin/env python3
"""Generate the YOLOv9e graph fixtures by RUNNING THE REFERENCE (build container only; never on the GPU box).

    python tests/golden/make_v9e_fixtures.py

The reference is imported in-process with make_fixtures.py's stand-ins, through make_v9_fixtures.py, whose fill, damping rule and run()
this script reuses; nothing of the reference is modified or copied.
  graph_yolov9e.npz      DetectionModel of cfg/models/v9/yolov9e.yaml at (1, 64, 64) and (2, 96, 128)
  graph_yolov9e_seg.npz  SegmentationModel of cfg/models/v9/yolov9e-seg.yaml at (1, 64, 64)
  graph_yolov9e_q.npz    yolov9e.yaml with every literal width divided by 4 (quarter(): 16 ... 256, CBLinear groups [16, 32, ...]), handed
                         to the reference as a dict, at both shapes: the three-precision sweep runs on it
all with nc = 12, parameters written by fill() (oracle.yolo_ref.synth_param; names and shapes stored, never the values), inputs from seeds
100 + si (checksums stored).  Per shape si: y, the three raw level maps, mc and proto for Segment, and the outputs of layers 16, 18, 21, 24
and 27 -- the five CBFuse maps -- as fuse{si}_{layer}, (B, C, H, W).  The second shape gives a 3 x 4 P5 map and non-square taps of every
shift 0 .. 4.  To keep a file under the repository's size limit the CBFuse maps of a shape are stored at every meta["fuse_step"][si]-th
channel, the smallest ODD step for which that shape's five maps take at most 256 KiB: an odd step visits every position inside the 8-
and 4-channel pieces a lane owns (a power of two would look at channel 0 of a piece only); the test slices what it reads back alike.

Damping (meta["damp"]): make_v9_fixtures.py's rule -- the tensors that feed the residual gain of the RepBottlenecks times ONE factor, the
largest of 1, 1/2, ... 1/16 for which every layer's output stays below 256 and the reference's own .half() run is within HALF of the
project's fp16 bounds of its fp32 run (score 5e-3, box 0.5 px, raw maps 1e-2 of the map's maximum: 2x to spare); the same is asserted for
the five CBFuse maps (1e-2 of each map's maximum).  CBFuse sums up to six maps, so activations grow, and for the FULL-WIDTH DETECT graph
that rule alone is not enough: its reference's own fp16 run stays 2 px and 1e-2 in score away from its fp32 run at every first factor (the
raw maps reach magnitudes of 50).  So there is a second factor, meta["damp"]["cblinear"]: the weight and bias of every CBLinear conv
(model.10 .. 14.conv.*) times the largest of 1, 1/2, 1/4, 1/8 for which some first factor meets the conditions.  What the fixtures hold:
yolov9e first factor 1/4 and cblinear 1/2; yolov9e_seg and yolov9e_q first factor 1/8 and cblinear 1 (the first rule alone).
meta["ref_fp16"] records the distances of the reference's own fp16 run, the CBFuse maps' as "fuse".

meta["ref_conv_gflops_640"]: 2 * MAC of every convolution of the fused reference model at 1 x 640 x 640, nc = 80 (make_v9_fixtures.py
conv_gflops_640; CBLinear's nn.Conv2d is counted like any other).  The yaml header says 193.0.
"""
import copy
import json
import re
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_v9_fixtures as V9  # noqa: E402  (stand-ins + the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402
from ultralytics.nn.tasks import DetectionModel, SegmentationModel  # noqa: E402

MF, NC, SHAPES, LIMIT = V9.MF, V9.NC, V9.SHAPES, V9.LIMIT
FUSE_LAYERS = (16, 18, 21, 24, 27)
FUSE_BYTES = 256 << 10
CBL_FACTORS = (1.0, 0.5, 0.25, 0.125)
CBL_KEY = re.compile(r"model\.\d+\.conv\.(weight|bias)")  # a CBLinear's nn.Conv2d: the one module whose conv sits directly under model.i
GRAPHS = [  # tag, yaml, task, width divisor, shapes
    ("yolov9e", "v9/yolov9e.yaml", "detect", 1, SHAPES),
    ("yolov9e_seg", "v9/yolov9e-seg.yaml", "segment", 1, SHAPES[:1]),
    ("yolov9e_q", "v9/yolov9e.yaml", "detect", 4, SHAPES),
]
WIDTH_ARGS = {"Conv": 1, "ADown": 1, "RepNCSPELAN4": 3, "SPPELAN": 2}  # how many leading arguments of a module are channel counts


def quarter(d: dict, div: int) -> dict:
    """The graph with every literal width divided by `div`: the leading channel arguments of WIDTH_ARGS' modules and CBLinear's groups."""
    d = copy.deepcopy(d)
    for layer in d["backbone"] + d["head"]:
        m, args = layer[2], layer[3]
        if m == "CBLinear":
            args[0] = [c // div for c in args[0]]
        for j in range(WIDTH_ARGS.get(m, 0)):
            args[j] //= div
    return d


def build(cfg, task, div, nc=NC):
    d = quarter(yaml.safe_load(open(MF.CFG / cfg)), div)
    d["nc"] = nc
    return (DetectionModel if task == "detect" else SegmentationModel)(d, ch=3, nc=nc, verbose=False).eval()


def filled(cfg, task, div, factor, cbl, seed=0):
    m = build(cfg, task, div)
    names = MF.fill(m, "", seed)
    with torch.no_grad():
        for k, t in m.state_dict().items():
            if V9.damped(k, V9.SUFFIXES["refconv"]):
                t.mul_(factor)
            if CBL_KEY.fullmatch(k) and type(m.model[int(k.split(".")[1])]).__name__ == "CBLinear":
                t.mul_(cbl)
    nparam = sum(p.numel() for p in m.parameters())
    m.fuse(verbose=False)
    return m, names, nparam


def run(m, x, task):
    """V9.run's outputs and the five CBFuse maps."""
    got = {}
    hooks = [m.model[i].register_forward_hook(lambda mod, inp, o, i=i: got.__setitem__(i, o.detach().float().clone())) for i in FUSE_LAYERS]
    res = V9.run(m, x, task)
    for h in hooks:
        h.remove()
    return res + ([got[i] for i in FUSE_LAYERS],)


def probe(cfg, task, div, factor, cbl, xs):
    m, _, _ = filled(cfg, task, div, factor, cbl)
    peak = [0.0]
    hooks = [layer.register_forward_hook(lambda mod, inp, o: peak.__setitem__(0, max(peak[0], float(o.abs().max())))
                                         if isinstance(o, torch.Tensor) else None) for layer in list(m.model)[:-1]]
    outs32 = [run(m, x, task) for x in xs]
    for h in hooks:
        h.remove()
    ok = peak[0] < 256.0 and all(bool(torch.isfinite(o[0]).all()) for o in outs32)
    dist = {"score": float("nan"), "box": float("nan"), "raw": float("nan"), "fuse": float("nan"), "layer_max": peak[0]}
    if ok:
        mh = m.half()
        outs16 = [run(mh, x.half(), task) for x in xs]
        ds = max(float((a[0][:, 4:4 + NC].float() - b[0][:, 4:4 + NC]).abs().max()) for a, b in zip(outs16, outs32))
        db = max(float((a[0][:, :4].float() - b[0][:, :4]).abs().max()) for a, b in zip(outs16, outs32))
        dr = max(float((ra.float() - rb_).abs().max() / rb_.abs().max()) for a, b in zip(outs16, outs32) for ra, rb_ in zip(a[1], b[1]))
        df = max(float((fa - fb).abs().max() / fb.abs().max()) for a, b in zip(outs16, outs32) for fa, fb in zip(a[4], b[4]))
        dist.update(score=ds, box=db, raw=dr, fuse=df)
        ok = all(bool(torch.isfinite(o[0]).all()) for o in outs16) and ds < 5e-3 and db < 0.5 and dr < 1e-2 and df < 1e-2
    return ok, dist


def conv_gflops_640(cfg):
    """V9.conv_gflops_640 on this script's build()."""
    keep = V9.build
    V9.build = lambda c, task, form, nc=NC: build(c, task, 1, nc)
    try:
        return V9.conv_gflops_640(cfg, "detect")
    finally:
        V9.build = keep


def graph_fixture(tag, cfg, task, div, shapes, gflops, seed=0):
    xs, xmeta = [], []
    for si, (b, h, w) in enumerate(shapes):
        x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + si))
        xs.append(x)
        xmeta.append({"sum": float(x.double().sum()), "first": x.flatten()[:8].tolist()})
    for cbl, factor in ((c, f) for c in CBL_FACTORS for f in V9.FACTORS):
        ok, dist = probe(cfg, task, div, factor, cbl, xs)
        print(tag, "factors", factor, cbl, "ok" if ok else "no", dist)
        if ok:
            break
    assert ok, (tag, "no damping factors keep the reference's own fp16 run within half the fp16 bounds")
    m, names, nparam = filled(cfg, task, div, factor, cbl, seed)
    out, ys, steps = {}, [], []
    for si, x in enumerate(xs):
        y, raw, mc, proto, fuse = run(m, x, task)
        if task == "segment":
            assert torch.equal(y[:, 4 + NC:], mc)
            out[f"mc{si}"], out[f"proto{si}"] = mc.numpy(), proto.numpy()
        assert len(raw) == 3
        out[f"y{si}"] = y.numpy()
        ys.append(y)
        for li, r in enumerate(raw):
            out[f"raw{si}_{li}"] = r.numpy()
        step = 1
        while sum(f[:, ::step].numel() for f in fuse) * 4 > FUSE_BYTES:
            step += 2
        steps.append(step)
        for i, f in zip(FUSE_LAYERS, fuse):
            out[f"fuse{si}_{i}"] = f[:, ::step].contiguous().numpy()
    for si, y in enumerate(ys):
        print(tag, si, tuple(y.shape), "max score", float(y[:, 4:4 + NC].max()))
    meta = {"family": "yolov9e", "scale": None, "task": task, "nc": NC, "seed": seed, "names": names, "nparam": nparam, "repconv": "refconv",
            "div": div, "stride": [float(s) for s in m.stride], "shapes": shapes, "x": xmeta,
            "fuse_layers": list(FUSE_LAYERS), "fuse_step": steps, "damp": {"suffixes": V9.SUFFIXES["refconv"], "factor": factor, "cblinear": cbl},
            "ref_fp16": dist, "ref_conv_gflops_640": gflops, "header_gflops_640": 193.0}
    path = HERE / f"graph_{tag}.npz"
    np.savez_compressed(path, **out, meta=json.dumps(meta))
    assert path.stat().st_size < LIMIT, (tag, path.stat().st_size)
    print(tag, path.stat().st_size, "bytes, CBFuse maps at channel steps", steps)


if __name__ == "__main__":
    torch.set_num_threads(8)
    gflops = round(conv_gflops_640("v9/yolov9e.yaml"), 4)
    print("reference conv GFLOPs at 640 x 640, nc = 80:", gflops, "(yaml header: 193.0)")
    for g in GRAPHS:
        graph_fixture(*g, gflops)
