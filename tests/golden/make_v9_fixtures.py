#!/usr/bin/env python3
"""Generate the YOLOv9 (GELAN) graph fixtures by RUNNING THE REFERENCE (build container only; never on the GPU box).

    python tests/golden/make_v9_fixtures.py

The reference is imported in-process with make_fixtures.py's stand-ins (this script imports it for them and for `fill`); nothing of
the reference is modified or copied.
  graph_yolov9c.npz         DetectionModel of cfg/models/v9/yolov9c.yaml        (ADown, n = 1, the fork's own RepConv: "refconv")
  graph_yolov9c_seg.npz     SegmentationModel of cfg/models/v9/yolov9c-seg.yaml
  graph_yolov9m.npz         DetectionModel of cfg/models/v9/yolov9m.yaml        (AConv on 184 channels, chunks of 180, hidden widths 60 / 90)
  graph_yolov9t.npz         DetectionModel of cfg/models/v9/yolov9t.yaml        (ELAN1, AConv, n = 3, hidden widths 16 / 24 / 32; "refconv")
  graph_yolov9t_repvgg.npz  the same graph with every RepBottleneck.cv1 replaced, before fill(), by upstream's
                            ultralytics.nn.modules.conv.RepConv(ci, co, 3, 1) -- what an upstream-pickled checkpoint unpickles in
                            that place; un-fused when the names are recorded, fused (BaseModel.fuse) when it is run
all with nc = 12, parameters written by fill() (oracle.yolo_ref.synth_param, names stored), inputs (1, 64, 64) and (2, 96, 128) from
seeds 100 + si (checksums stored).  Per shape: y, the three raw level maps, for Segment mc and proto, and
non_max_suppression(y, conf, 0.7, nc=12) per image at the largest conf of 0.25 / 0.1 / 0.01 / 0.001 that keeps a detection
(meta["nms_conf"]; synthetic head scores are low, the raw maps carry the class information).

Damping (meta["damp"] = {"suffixes": [...], "factor": f}).  Under the synthetic fill the chained residual RepBottlenecks of the narrow
graphs have a gain above 1 (per-layer maxima of 1e9 in fp32 on yolov9t, NaN in fp16): an artefact of the fill, not of the graph.  After
fill() every tensor that feeds that gain -- names under a `.m.<i>.` that end in one of the suffixes -- is multiplied by ONE factor, the
largest of 1, 1/2, 1/4, 1/8, 1/16 for which, on both shapes, (1) every top-level layer's output stays below 256 in magnitude in the
reference's fp32 run (2^8 of headroom under fp16's largest value) and (2) the reference's own .half() run is finite and within HALF of
the project's fp16 bounds of its fp32 run (score 5e-3, box 0.5 px, raw maps 1e-2 of the map's maximum).  A test that regenerates the
state dict from synth_param applies the same rule.  meta["ref_fp16"] records that distance of the reference's own fp16 run.

meta["ref_conv_gflops_640"]: 2 * MAC of every convolution the (fused) reference model of each size runs at 1 x 640 x 640 with nc = 80,
counted here from the convs' output shapes (DFL excluded, as in the plan's count) -- what Plan's own count is compared with (the
yaml headers' 7.7 / 26.4 / 102.1 GFLOPs come from another counter; the c graph agrees with its header to 0.5 %).
"""
import json
import re
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_fixtures as MF  # noqa: E402  (stand-ins + the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402
from ultralytics.nn.modules import block as rb, conv as rc  # noqa: E402
from ultralytics.nn.tasks import DetectionModel, SegmentationModel  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

NC = 12
SHAPES = [(1, 64, 64), (2, 96, 128)]
LIMIT = 1 << 20
FACTORS = (1.0, 0.5, 0.25, 0.125, 0.0625)
SUFFIXES = {"refconv": [".cv1.weight", ".cv1.convmap.weight"], "repvgg": [".cv1.conv1.conv.weight", ".cv1.conv2.conv.weight"]}
GRAPHS = [  # tag, yaml, scale, task, repconv form
    ("yolov9c", "v9/yolov9c.yaml", "c", "detect", "refconv"),
    ("yolov9c_seg", "v9/yolov9c-seg.yaml", "c", "segment", "refconv"),
    ("yolov9m", "v9/yolov9m.yaml", "m", "detect", "refconv"),
    ("yolov9t", "v9/yolov9t.yaml", "t", "detect", "refconv"),
    ("yolov9t_repvgg", "v9/yolov9t.yaml", "t", "detect", "repvgg"),
]


def build(cfg, task, form, nc=NC):
    d = yaml.safe_load(open(MF.CFG / cfg))
    d["nc"] = nc
    m = (DetectionModel if task == "detect" else SegmentationModel)(d, ch=3, nc=nc, verbose=False).eval()
    if form == "repvgg":
        for mod in m.modules():
            if isinstance(mod, rb.RepBottleneck):
                co, ci = mod.cv1.weight.shape[:2]
                mod.cv1 = rc.RepConv(ci, co, 3, 1)
        MF.initialize_weights(m)  # as the model's constructor does upstream: every BatchNorm, the new ones included, at eps 1e-3
        m.eval()
    return m


def damped(name, suffixes):
    return re.search(r"\.m\.\d+\.", name) is not None and any(name.endswith(s) for s in suffixes)


def filled(cfg, task, form, factor, seed=0):
    """(model fused and ready to run, recorded un-fused names, parameter count)"""
    m = build(cfg, task, form)
    names = MF.fill(m, "", seed)
    with torch.no_grad():
        for k, t in m.state_dict().items():
            if damped(k, SUFFIXES[form]):
                t.mul_(factor)
    nparam = sum(p.numel() for p in m.parameters())
    m.fuse(verbose=False)
    return m, names, nparam


def run(m, x, task):
    with torch.inference_mode():
        res = m(x)
    if task == "detect":
        y, raw = res
        return y, raw, None, None
    y, (raw, mc, proto) = res
    return y, raw, mc, proto


def probe(cfg, task, form, factor, xs):
    """(conditions hold, fp16-to-fp32 distance of the reference) for one damping factor."""
    m, _, _ = filled(cfg, task, form, factor)
    peak = [0.0]
    hooks = [layer.register_forward_hook(lambda mod, inp, o: peak.__setitem__(0, max(peak[0], float(o.abs().max())))
                                         if isinstance(o, torch.Tensor) else None) for layer in list(m.model)[:-1]]
    outs32 = [run(m, x, task) for x in xs]
    for h in hooks:
        h.remove()
    ok = peak[0] < 256.0 and all(bool(torch.isfinite(o[0]).all()) for o in outs32)
    dist = {"score": float("nan"), "box": float("nan"), "raw": float("nan"), "layer_max": peak[0]}
    if ok:
        mh = m.half()
        outs16 = [run(mh, x.half(), task) for x in xs]
        ds = max(float((a[0][:, 4:4 + NC].float() - b[0][:, 4:4 + NC]).abs().max()) for a, b in zip(outs16, outs32))
        db = max(float((a[0][:, :4].float() - b[0][:, :4]).abs().max()) for a, b in zip(outs16, outs32))
        dr = max(float((ra.float() - rb_).abs().max() / rb_.abs().max()) for a, b in zip(outs16, outs32) for ra, rb_ in zip(a[1], b[1]))
        dist.update(score=ds, box=db, raw=dr)
        ok = all(bool(torch.isfinite(o[0]).all()) for o in outs16) and ds < 5e-3 and db < 0.5 and dr < 1e-2
    return ok, dist


def conv_gflops_640(cfg, task):
    """2 * MAC of every conv of the fused reference model at 1 x 640 x 640, nc = 80: counted at 64 x 64 from the output shapes and
    scaled by 100 (every map is even down to stride 32, so the counts scale with the area)."""
    m = build(cfg, task, "refconv", nc=80)
    m.fuse(verbose=False)
    total = [0]

    def conv_hook(mod, inp, out):
        total[0] += 2 * out.numel() * mod.in_channels // mod.groups * mod.kernel_size[0] * mod.kernel_size[1]

    def deconv_hook(mod, inp, out):  # ConvTranspose2d(c, c, 2, 2): one tap per output pixel
        total[0] += 2 * out.numel() * mod.in_channels

    def rep_hook(mod, inp, out):  # the fork's RepConv runs F.conv2d with its own kernel
        co, ci, kh, kw = mod.origin_kernel_shape
        total[0] += 2 * out.numel() * ci * kh * kw

    for name, mod in m.named_modules():
        if ".dfl" in name or name.endswith(".convmap"):
            continue
        if isinstance(mod, torch.nn.Conv2d):
            mod.register_forward_hook(conv_hook)
        elif isinstance(mod, torch.nn.ConvTranspose2d):
            mod.register_forward_hook(deconv_hook)
        elif isinstance(mod, rb.RepConv):
            mod.register_forward_hook(rep_hook)
    with torch.inference_mode():
        m(torch.zeros(1, 3, 64, 64))
    return total[0] * 100 / 1e9


def graph_fixture(tag, cfg, scale, task, form, gflops, seed=0):
    xs, xmeta = [], []
    for si, (b, h, w) in enumerate(SHAPES):
        x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + si))
        xs.append(x)
        xmeta.append({"sum": float(x.double().sum()), "first": x.flatten()[:8].tolist()})
    for factor in FACTORS:
        ok, dist = probe(cfg, task, form, factor, xs)
        print(tag, "factor", factor, "ok" if ok else "no", dist)
        if ok:
            break
    assert ok, (tag, "no damping factor meets the conditions")
    m, names, nparam = filled(cfg, task, form, factor, seed)
    out, ys, raws = {}, [], {}
    for si, x in enumerate(xs):
        y, raw, mc, proto = run(m, x, task)
        if task == "segment":
            assert torch.equal(y[:, 4 + NC:], mc)
            out[f"mc{si}"], out[f"proto{si}"] = mc.numpy(), proto.numpy()
        assert len(raw) == 3
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
    meta = {"family": "yolov9", "scale": scale, "task": task, "nc": NC, "seed": seed, "names": names, "nparam": nparam, "repconv": form,
            "stride": [float(s) for s in m.stride], "shapes": SHAPES, "x": xmeta, "nms_conf": conf, "nms_iou": 0.7, "raw_shapes": [0, 1],
            "damp": {"suffixes": SUFFIXES[form], "factor": factor}, "ref_fp16": dist, "ref_conv_gflops_640": gflops}
    path = HERE / f"graph_{tag}.npz"
    np.savez_compressed(path, **out, **raws, meta=json.dumps(meta))
    if path.stat().st_size >= LIMIT:  # keep the file under the size the other goldens keep: raw maps of shape 0 only
        meta["raw_shapes"] = [0]
        np.savez_compressed(path, **out, **{k: v for k, v in raws.items() if k.startswith("raw0_")}, meta=json.dumps(meta))
    assert path.stat().st_size < LIMIT, (tag, path.stat().st_size)
    print(tag, path.stat().st_size, "bytes, raw maps of shapes", meta["raw_shapes"])


if __name__ == "__main__":
    torch.set_num_threads(8)
    gflops = {s: round(conv_gflops_640(f"v9/yolov9{s}.yaml", "detect"), 4) for s in "tsmc"}
    print("reference conv GFLOPs at 640 x 640, nc = 80:", gflops)
    for g in GRAPHS:
        graph_fixture(*g, gflops)
