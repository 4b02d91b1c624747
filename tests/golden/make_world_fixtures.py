#!/usr/bin/env python3
"""Generate the YOLO-World v2 graph fixtures by RUNNING THE REFERENCE (build container only; never on the GPU box).

    python tests/golden/make_world_fixtures.py

The reference is imported in-process with make_fixtures.py's stand-ins (this script imports it for them and for `fill`); nothing of
the reference is modified or copied.  Only .npz data is written.
  graph_yolov8n_worldv2.npz   WorldModel of cfg/models/v8/yolov8-worldv2.yaml at scale n (heads 2 / 1 / 2 / 4, one Bottleneck per block)
  graph_yolov8s_worldv2.npz   scale s (heads 4 / 2 / 4 / 8)
  graph_yolov8m_worldv2.npz   scale m at the width multiple shipped (heads 6 / 3 / 6 / 9, hidden widths 96 .. 288, two Bottlenecks per block)
all with nc = 12, parameters written by fill() (oracle.yolo_ref.synth_param; names and the seed stored, no weights), inputs (1, 64, 64) and
(2, 96, 128) from seeds 100 + si (checksums stored), text features txt = normalize(randn(1, 12, 512, generator=manual_seed(7))) and a second
set of 5 rows from seed 8 (checksums stored).  Per shape: y, the raw level maps, and non_max_suppression(y, conf, 0.7, nc=12) per image at
the largest conf of 0.25 / 0.1 / 0.01 / 0.001 that keeps a detection (meta["nms_conf"]).  Scale n also stores y and the raw maps under the
5-row text with head.nc = 5 -- what set_classes leaves behind (tasks.py:633-634) -- as y5_<si> / raw5_<si>_<l>.  meta["yaml"] is the yaml file as
parsed (nc = 80), so that a test can compare graphs.stock_cfg with it where the reference is absent.  meta["conv_flops"][si] is 2 x MAC of
every dense nn.Conv2d the reference ran on shape si (forward hooks), DFL's excepted and each cv3.l.2 counted as c3 -> nc: the class head
counted as the engine folds it.

Admission, checked here on the reference alone and recorded in meta:
 (1) make_v6_fixtures.py's two conditions: every top-level layer's output below 256 in the fp32 run, and the reference's own .half() run
     finite and within HALF of the project's fp16 bounds of its fp32 run (score 5e-3, box 0.5 px, raw maps 1.5e-2 of max(1, maximum));
     meta["ref_fp16"].
 (2) on every C2fAttn the gate aw -- the block's output over its proj_conv's output, both from forward hooks, where the latter is not tiny --
     has a minimum below 0.25 and a maximum above 0.75 over the pixels of both shapes WITHIN ONE HEAD; meta["gate"] is that head's range
     (the widest head's).  A head's bias is one number, so a spread inside a head comes from the maximum over the classes alone: a fill
     under which the gate is constant, or differs between heads only by their biases, would hide a wrong max.  And the classes must
     matter: at some pixel of that block the largest class logit of a head exceeds the smallest by 2 or more (the guide's bias adds the same
     to every class, so a spread may come from it alone); meta["class_spread"].
 (3) on each shape some class score exceeds 0.25 and some is below 0.01; meta["score_range"].
Damping (meta["damp"] = a list of {"contains", "suffix", "factor"}: every tensor whose name contains the one and ends with the other is
multiplied by the factor after fill(); a test regenerates the state dict by the same rule).  Fixed lists, searched in order, the FIRST
candidate that meets the condition taken.  Per C2fAttn block, in graph order (a block's gate depends on the blocks before it), for (2):
   model.<i>.attn.gl.weight x 1, 2, 4, ... 512 (powers of 2) (the guide's gain: synth_param draws the Linear with a fan-in of 512, so the
                                                              class-dependent part of the dot products is small and every gate sits near sigmoid(0))
   model.<i>.attn.bias      x 1, 16, -16, 32, -32, 64, -64   (U(-0.2, 0.2) per head after fill: the maximum over the classes is rarely negative,
                                                              so a gate below 0.25 needs a head whose bias is well below zero, and a block with
                                                              ONE head needs the sign that makes it so)
the gain the outer loop.  Then, for (1) and (3) with the blocks' factors fixed:
   model.22.cv<2|3>.<l>.2.weight x 1, 1/2, ... 1/32       (make_v6_fixtures.py's rule: a box is stride x the DFL expectation of 16 logits, so the
                                                              reference's own fp16 distance scales with the gain of the branches' last convs;
                                                              scale m, two Bottlenecks per block, moves a box by 5 px under the plain fill)
   *.cv4.<l>.logit_scale         x 1, 0.5, 0                 (synth_param draws it N(0, 2): exp() of it multiplies the class logits)
the head factor the outer loop.
"""
import itertools
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_fixtures as MF  # noqa: E402  (stand-ins + the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402
from ultralytics.nn.tasks import WorldModel  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

NC, NC2, E = 12, 5, 512
SHAPES = [(1, 64, 64), (2, 96, 128)]
LIMIT = 1 << 20
HEAD = 22
ATTN = (12, 15, 18, 21)
HEADS = (1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125)
GAINS, BIASES, SCALES = (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0, 512.0), (1.0, 16.0, -16.0, 32.0, -32.0, 64.0, -64.0), (1.0, 0.5, 0.0)
GRAPHS = [("yolov8n_worldv2", "n"), ("yolov8s_worldv2", "s"), ("yolov8m_worldv2", "m")]


def parsed():
    return yaml.safe_load(open(MF.CFG / "v8" / "yolov8-worldv2.yaml"))


def texts():
    t1 = torch.nn.functional.normalize(torch.randn(1, NC, E, generator=torch.Generator().manual_seed(7)), dim=-1)
    t2 = torch.nn.functional.normalize(torch.randn(1, NC2, E, generator=torch.Generator().manual_seed(8)), dim=-1)
    return t1, t2


def hit(name, rule):
    return rule["contains"] in name and name.endswith(rule["suffix"]) and not name.endswith("norm.bias")


def filled(scale, damp, seed=0):
    """(model fused and ready to run under the 12-row text, recorded un-fused names, parameter count)"""
    d = parsed()
    d["nc"], d["scale"] = NC, scale
    m = WorldModel(d, ch=3, nc=NC, verbose=False).eval()
    names = MF.fill(m, "", seed)
    with torch.no_grad():
        for rule in damp:
            n = [t.mul_(rule["factor"]) for k, t in m.state_dict().items() if hit(k, rule)]
            assert len(n) == {".cv4.": 3, f"model.{HEAD}.cv": 6}.get(rule["contains"], 1), (rule, len(n))  # per level / per branch and level / the block's own
    nparam = sum(p.numel() for p in m.parameters())
    m.fuse(verbose=False)
    m.txt_feats = texts()[0]
    return m, names, nparam


def run(m, x):
    with torch.inference_mode():
        y, raw = m(x)
    return y, raw


def probe(scale, damp, xs, block=None):
    """(conditions hold, what was measured) for one damping candidate; block: condition (2) on that C2fAttn alone, nothing else."""
    m, _, _ = filled(scale, damp)
    peak, keep, gates, spread = [0.0], {}, {i: [0.5, 0.5] for i in ATTN}, {i: 0.0 for i in ATTN}
    hooks = [layer.register_forward_hook(lambda mod, inp, o: peak.__setitem__(0, max(peak[0], float(o.abs().max())))
                                         if isinstance(o, torch.Tensor) else None) for layer in list(m.model)[:-1]]
    for i in ATTN:
        hooks.append(m.model[i].attn.proj_conv.register_forward_hook(lambda mod, inp, o, i=i: keep.__setitem__(i, o)))

        def gate(mod, inp, o, i=i):
            p, nh = keep[i], mod.nh
            for hp, ho in zip(p.chunk(nh, 1), o.chunk(nh, 1)):  # per head: the widest range inside one head, over the calls so far
                aw = (ho / hp)[hp.abs() > 1e-3]
                lo, hi = float(aw.min()), float(aw.max())
                if min(0.5 - lo, hi - 0.5) > min(0.5 - gates[i][0], gates[i][1] - 0.5):
                    gates[i] = [lo, hi]
            x, txt = inp
            dots = torch.einsum("bmchw,bnmc->bmhwn", x.view(x.shape[0], nh, -1, *x.shape[2:]), mod.gl(txt).view(x.shape[0], -1, nh, mod.hc)) / mod.hc ** 0.5
            spread[i] = max(spread[i], float((dots.max(-1)[0] - dots.min(-1)[0]).max()))
        hooks.append(m.model[i].attn.register_forward_hook(gate))
    outs32 = [run(m, x) for x in xs]
    for h in hooks:
        h.remove()
    rng = [[float(o[0][:, 4:].min()), float(o[0][:, 4:].max())] for o in outs32]
    info = {"layer_max": peak[0], "gate": {str(i): g for i, g in gates.items()}, "score_range": rng, "class_spread": {str(i): v for i, v in spread.items()}}
    if block is not None:
        return gates[block][0] < 0.25 and gates[block][1] > 0.75 and spread[block] >= 2.0, info
    ok = (peak[0] < 256.0 and all(bool(torch.isfinite(o[0]).all()) for o in outs32) and all(g[0] < 0.25 and g[1] > 0.75 for g in gates.values()) and min(spread.values()) >= 2.0
          and all(lo < 0.01 and hi > 0.25 for lo, hi in rng))
    if ok:
        mh = m.half()
        outs16 = [run(mh, x.half()) for x in xs]
        ds = max(float((a[0][:, 4:].float() - b[0][:, 4:]).abs().max()) for a, b in zip(outs16, outs32))
        db = max(float((a[0][:, :4].float() - b[0][:, :4]).abs().max()) for a, b in zip(outs16, outs32))
        dr = max(float((ra.float() - rb_).abs().max() / max(1.0, float(rb_.abs().max()))) for a, b in zip(outs16, outs32) for ra, rb_ in zip(a[1], b[1]))
        info.update(score=ds, box=db, raw=dr)
        ok = all(bool(torch.isfinite(o[0]).all()) for o in outs16) and ds < 5e-3 and db < 0.5 and dr < 1.5e-2
    return ok, info


def conv_flops(m, x, nc):
    """2 x MAC of the dense nn.Conv2d modules in one forward: DFL's excepted, each cv3.l.2 (c3 -> E, then the contrastive head) as c3 -> nc."""
    total, hooks = [0], []
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.Conv2d) and mod.groups == 1 and not name.endswith("dfl.conv"):
            folded = f"model.{HEAD}.cv3." in name and name.endswith(".2")

            def count(mod, inp, o, folded=folded):
                co = nc if folded else o.shape[1]
                total[0] += 2 * o.shape[0] * o.shape[2] * o.shape[3] * co * mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1]
            hooks.append(mod.register_forward_hook(count))
    run(m, x)
    for h in hooks:
        h.remove()
    return total[0]


def graph_fixture(tag, scale, seed=0):
    xs, xmeta = [], []
    for si, (b, h, w) in enumerate(SHAPES):
        x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + si))
        xs.append(x)
        xmeta.append({"sum": float(x.double().sum()), "first": x.flatten()[:8].tolist()})
    blocks = []
    for i in ATTN:
        for g, b in itertools.product(GAINS, BIASES):
            cand = blocks + [{"contains": f"model.{i}.attn.", "suffix": "gl.weight", "factor": g}, {"contains": f"model.{i}.attn.", "suffix": "attn.bias", "factor": b}]
            ok, info = probe(scale, cand, xs, block=i)
            if ok:
                break
        assert ok, (tag, i, "no gain / bias factor spreads the gate")
        print(tag, "block", i, "gain", g, "bias", b, "gate", info["gate"][str(i)], "class spread", info["class_spread"][str(i)], flush=True)
        blocks = cand
    for hf, f in itertools.product(HEADS, SCALES):
        damp = blocks + [{"contains": f"model.{HEAD}.cv", "suffix": ".2.weight", "factor": hf}, {"contains": ".cv4.", "suffix": "logit_scale", "factor": f}]
        ok, info = probe(scale, damp, xs)
        print(tag, "head factor", hf, "logit_scale factor", f, "ok" if ok else "no", info, flush=True)
        if ok:
            break
    assert ok, (tag, "no damping candidate meets the conditions")
    m, names, nparam = filled(scale, damp, seed)
    t1, t2 = texts()
    out, ys, raws = {}, [], {}
    flops = [conv_flops(m, x, NC) for x in xs]
    for si, x in enumerate(xs):
        y, raw = run(m, x)
        assert len(raw) == len(m.stride) and y.shape[1] == 4 + NC and all(r.shape[1] == 64 + NC for r in raw)
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
        print(tag, si, tuple(ys[si].shape), "conf", conf, "detections", [len(r) for r in dd], "max score", float(ys[si][:, 4:].max()))
    if scale == "n":  # what set_classes leaves behind: new text rows and head.nc (tasks.py:633-634); c3 stays what nc = 12 made it
        m.txt_feats, m.model[-1].nc = t2, NC2
        for si, x in enumerate(xs):
            y, raw = run(m, x)
            assert y.shape[1] == 4 + NC2 and all(r.shape[1] == 64 + NC2 for r in raw)
            out[f"y5_{si}"] = y.numpy()
            for li, r in enumerate(raw):
                raws[f"raw5_{si}_{li}"] = r.numpy()
        m.txt_feats, m.model[-1].nc = t1, NC
    d = parsed()
    head = m.model[-1]
    meta = {"family": "yolov8-worldv2", "scale": scale, "task": "detect", "nc": NC, "nc2": NC2, "embed": E, "seed": seed, "names": names,
            "nparam": nparam, "stride": [float(s) for s in m.stride], "shapes": SHAPES, "x": xmeta, "nms_conf": conf, "nms_iou": 0.7,
            "damp": damp, "ref_fp16": {k: info[k] for k in ("score", "box", "raw", "layer_max")}, "gate": info["gate"], "class_spread": info["class_spread"],
            "score_range": info["score_range"], "yaml": d, "conv_flops": flops,
            "txt": [{"sum": float(t.double().sum()), "first": t.flatten()[:8].tolist()} for t in (t1, t2)],
            "heads": [m.model[i].attn.nh for i in ATTN], "hc": [m.model[i].attn.hc for i in ATTN], "n": [len(m.model[i].m) for i in ATTN],
            "c3": head.cv3[0][0].conv.out_channels, "bn_eps": float(head.cv4[0].norm.eps)}
    assert all(m.model[i].attn.ec is None and m.model[i].attn.scale == 1.0 for i in ATTN)
    path = HERE / f"graph_{tag}.npz"
    np.savez_compressed(path, **out, **raws, meta=json.dumps(meta))
    assert path.stat().st_size < LIMIT, (tag, path.stat().st_size)
    print(tag, path.stat().st_size, "bytes,", nparam, "parameters", "heads", meta["heads"], "n", meta["n"], "flops", flops)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for g in GRAPHS:
        graph_fixture(*g)
