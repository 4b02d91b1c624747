#!/usr/bin/env python3
"""Generate the YOLOv10 GRAPH fixtures by RUNNING THE REFERENCE (build container only; never on the GPU box).

    python tests/golden/make_v10_graph_fixtures.py

(make_v10_fixtures.py, beside this file, makes the fixtures of the top-k operator alone and is left as it is.)  The reference is
imported in-process with make_fixtures.py's stand-ins; nothing of it is modified or copied.
  graph_yolov10n.npz  DetectionModel of cfg/models/v10/yolov10n.yaml  (C2fCIB with lk = True, the RepVGGDW 7x7, at P5 of the neck)
  graph_yolov10s.npz  DetectionModel of cfg/models/v10/yolov10s.yaml  (the same block in the backbone too)
  graph_yolov10b.npz  DetectionModel of cfg/models/v10/yolov10b.yaml  (lk = False, C2fCIB at 40 x 40 and in the neck, n > 1)
all with nc = 12, parameters written by fill() (oracle.yolo_ref.synth_param, names stored), inputs (1, 64, 64) and (2, 96, 128) from
seeds 100 + si (checksums stored).

Two rules condition the synthetic fill (meta["one2one"], meta["damp"]); a test that regenerates the state dict applies both.

one2one.  synth_param's head rules key on ".cv2." / ".cv3.", which "model.23.one2one_cv3.0.2.bias" contains neither of: filled as it
is, the one2one scores saturate and the reference's own .half() run is 1.8e-2 in score and 2.6 px off its fp32 run.  After fill(), every
tensor of one2one_cv2.* / one2one_cv3.* is overwritten with synth_param(name.replace(".one2one_cv", ".cv"), shape, seed + 1): the
one2many head's conditioning from other draws.  Asserted: the one2one and one2many raw maps differ, so a swapped branch is noticed.

Damping, make_v9_fixtures.py's rule.  The shortcuts -- PSA's b + attn(b) and b + ffn(b), CIB's x + cv1(x), C2f's Bottlenecks -- have a
gain above 1 under the fill (b undamped: a layer peak of 8535, the .half() run NaN).  Every tensor whose name ends in
".attn.proj.conv.weight" or ".ffn.1.conv.weight", or, under any ".m.<i>.", in ".cv1.4.conv.weight" (CIB's last depthwise conv) or
".cv2.conv.weight" (Bottleneck.cv2), is multiplied by ONE factor: the largest of 1, 1/2, ..., 1/16 for which, on both shapes, (1) every
top-level layer's output stays below 256 in magnitude in the reference's fp32 run and (2) the reference's own .half() run is finite and
within HALF of the project's fp16 bounds of its fp32 run: score 5e-3 and box 0.5 px on the pre-top-k tensor, raw maps of BOTH heads 1e-2
of the map's maximum.  The factor is searched and asserted, never written down; meta["ref_fp16"] records the distance it leaves.

Per graph and shape si: rows300_si / rows20_si, the model's own output rows (B, min(max_det, A), 6) with max_det = 300 (K = A = 84 / 252:
the first stage selects everything) and 20 (set on the head instance; both stages select); pre_si = head._inference(one2one), the
pre-top-k tensor (B, 4 + nc, A) with xyxy boxes; o2o{si}_{l} / o2m{si}_{l}, the raw maps of the two heads (meta["raw_shapes"]: both shapes
where the file stays under 1 MiB, else shape 0).  Asserted for every max_det = 20 case and image: at least half of the 20 rows have a
score more than 2e-4 above the 20th, so a test may demand that the clear winners are found.

meta["yamls"][scale] = {"scales", "backbone", "head"}: the parsed layer lists of all six yamls ('None' read as None, which is what
parse_model's eval makes of it).  meta["ref_conv_gflops_640"][scale]: 2 * MAC of every convolution the (fused) reference model runs at
1 x 640 x 640 with nc = 80, both heads' branches included, counted as make_ghost_fixtures.py counts it.
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
from oracle.yolo_ref import synth_param  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402

NC = 12
SHAPES = [(1, 64, 64), (2, 96, 128)]
LIMIT = 1 << 20
FACTORS = (1.0, 0.5, 0.25, 0.125, 0.0625)
SUFFIXES = [".attn.proj.conv.weight", ".ffn.1.conv.weight"]           # anywhere
SUFFIXES_M = [".cv1.4.conv.weight", ".cv2.conv.weight"]              # under a ".m.<i>." only
SCALES = "nsmblx"
GRAPHS = ["n", "s", "b"]
MAX_DETS = (300, 20)
GAP = 2e-4


def load_yaml(scale):
    return yaml.safe_load(open(MF.CFG / "v10" / f"yolov10{scale}.yaml"))


def build(scale, nc=NC):
    d = load_yaml(scale)
    d["nc"] = nc
    return DetectionModel(d, ch=3, nc=nc, verbose=False).eval()


def damped(name):
    return any(name.endswith(s) for s in SUFFIXES) or (re.search(r"\.m\.\d+\.", name) is not None and any(name.endswith(s) for s in SUFFIXES_M))


def filled(scale, factor, seed=0):
    """(model fused and ready to run, recorded un-fused names, parameter count)"""
    m = build(scale)
    names = MF.fill(m, "", seed)
    with torch.no_grad():
        for k, t in m.state_dict().items():
            if k.endswith("num_batches_tracked"):
                continue
            if ".one2one_cv" in k:
                t.copy_(synth_param(k.replace(".one2one_cv", ".cv"), t.shape, seed + 1))
            if damped(k):
                t.mul_(factor)
    nparam = sum(p.numel() for p in m.parameters())
    m.fuse(verbose=False)
    return m, names, nparam


def run(m, x, max_det):
    """(rows, pre-top-k tensor, one2one maps, one2many maps)"""
    head = m.model[-1]
    head.max_det = max_det
    head.shape = None  # the anchors are made anew, in the dtype of this run
    with torch.inference_mode():
        y, raw = m(x)
        pre = head._inference([t.clone() for t in raw["one2one"]])
    return y, pre, raw["one2one"], raw["one2many"]


def probe(scale, factor, xs):
    """(conditions hold, fp16-to-fp32 distance of the reference) for one damping factor."""
    m, _, _ = filled(scale, factor)
    peak = [0.0]
    hooks = [layer.register_forward_hook(lambda mod, inp, o: peak.__setitem__(0, max(peak[0], float(o.abs().max())))
                                         if isinstance(o, torch.Tensor) else None) for layer in list(m.model)[:-1]]
    outs32 = [run(m, x, 300) for x in xs]
    for h in hooks:
        h.remove()
    finite = lambda outs: all(bool(torch.isfinite(o[1]).all()) for o in outs)  # noqa: E731
    ok = peak[0] < 256.0 and finite(outs32)
    dist = {"score": float("nan"), "box": float("nan"), "raw": float("nan"), "layer_max": peak[0]}
    if ok:
        mh = m.half()
        outs16 = [run(mh, x.half(), 300) for x in xs]
        ds = max(float((a[1][:, 4:].float() - b[1][:, 4:]).abs().max()) for a, b in zip(outs16, outs32))
        db = max(float((a[1][:, :4].float() - b[1][:, :4]).abs().max()) for a, b in zip(outs16, outs32))
        dr = max(float((ra.float() - rb_).abs().max() / rb_.abs().max()) for a, b in zip(outs16, outs32) for k in (2, 3) for ra, rb_ in zip(a[k], b[k]))
        dist.update(score=ds, box=db, raw=dr)
        ok = finite(outs16) and ds < 5e-3 and db < 0.5 and dr < 1e-2
    return ok, dist


def conv_gflops_640(scale):
    m = build(scale, nc=80)
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


def parsed_yaml(scale):
    d = load_yaml(scale)
    fix = lambda layers: [[f, n, m, [None if a == "None" else a for a in args]] for f, n, m, args in layers]  # noqa: E731
    return {"scales": d["scales"], "backbone": fix(d["backbone"]), "head": fix(d["head"])}


def graph_fixture(scale, gflops, yamls, seed=0):
    tag = f"yolov10{scale}"
    xs, xmeta = [], []
    for si, (b, h, w) in enumerate(SHAPES):
        x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + si))
        xs.append(x)
        xmeta.append({"sum": float(x.double().sum()), "first": x.flatten()[:8].tolist()})
    for factor in FACTORS:
        ok, dist = probe(scale, factor, xs)
        print(tag, "factor", factor, "ok" if ok else "no", dist, flush=True)
        if ok:
            break
    assert ok, (tag, "no damping factor meets the conditions")
    m, names, nparam = filled(scale, factor, seed)
    out, raws, clear = {}, {}, []
    for si, x in enumerate(xs):
        for md in MAX_DETS:
            y, pre, o2o, o2m = run(m, x, md)
            A = pre.shape[2]
            assert tuple(y.shape) == (x.shape[0], min(md, A), 6) and tuple(pre.shape) == (x.shape[0], 4 + NC, A)
            out[f"rows{md}_{si}"] = y.numpy()
            if md == 20:
                n_clear = [(y[bi, :, 4] > y[bi, -1, 4] + GAP).sum().item() for bi in range(x.shape[0])]
                srt = pre[:, 4:].flatten(1).sort(1, descending=True)[0]
                ties = int((srt[:, :md] == srt[:, 1:md + 1]).sum())
                print(tag, si, "max_det 20: rows more than", GAP, "above the 20th:", n_clear, "exact ties among the first 21 scores:", ties)
                assert min(n_clear) >= 10, (tag, si, n_clear)
                clear.append(n_clear)
        out[f"pre_{si}"] = pre.numpy()
        assert not any(torch.equal(a, b) for a, b in zip(o2o, o2m)), "one2one and one2many maps must differ"
        assert len(o2o) == len(o2m) == len(m.stride)
        for li, (a, b) in enumerate(zip(o2o, o2m)):
            raws[f"o2o{si}_{li}"], raws[f"o2m{si}_{li}"] = a.numpy(), b.numpy()
        print(tag, si, tuple(pre.shape), "top score", float(pre[:, 4:].max()))
    meta = {"family": "yolov10", "scale": scale, "task": "detect", "nc": NC, "seed": seed, "names": names, "nparam": nparam,
            "stride": [float(s) for s in m.stride], "shapes": SHAPES, "x": xmeta, "raw_shapes": [0, 1], "max_dets": list(MAX_DETS),
            "one2one": {"rule": "synth_param(name.replace('.one2one_cv', '.cv'), shape, seed + 1)", "seed_offset": 1},
            "damp": {"suffixes": SUFFIXES, "suffixes_m": SUFFIXES_M, "factor": factor}, "ref_fp16": dist, "clear_rows20": clear, "gap": GAP,
            "ref_conv_gflops_640": gflops, "yamls": yamls}
    path = HERE / f"graph_{tag}.npz"
    np.savez_compressed(path, **out, **raws, meta=json.dumps(meta))
    if path.stat().st_size >= LIMIT:
        meta["raw_shapes"] = [0]
        np.savez_compressed(path, **out, **{k: v for k, v in raws.items() if k[3] == "0"}, meta=json.dumps(meta))
    assert path.stat().st_size < LIMIT, (tag, path.stat().st_size)
    print(tag, path.stat().st_size, "bytes, raw maps of shapes", meta["raw_shapes"], flush=True)


if __name__ == "__main__":
    torch.set_num_threads(8)
    gflops = {s: round(conv_gflops_640(s), 4) for s in SCALES}
    print("reference conv GFLOPs at 640 x 640, nc = 80:", gflops, flush=True)
    yamls = {s: parsed_yaml(s) for s in SCALES}
    for g in GRAPHS:
        graph_fixture(g, gflops, yamls)
