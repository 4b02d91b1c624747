"""Shared pieces of the graph-family tests (test_ghost.py, test_yolov3.py, test_yolov6.py, test_yolov9.py, test_yolov9e.py, test_yolov10.py,
test_world.py, test_p2p6.py; fixture / x_of / state_dict also test_pose_graph.py, test_classify.py, test_obb.py): the fixtures of
tests/golden/graph_<tag>.npz, the reference's state dict regenerated from them, an engine on both, the parity checkers, the NMS comparison,
the bit-equality loop of the on / off tests and the stand-in for the reference's model.  Not a test module, and no family's knowledge: every
bound is an argument, which each family file passes from one module-level constant (test_graph_helpers.py runs the checkers on both sides
of each of them)."""
import json
from collections import namedtuple

import numpy as np
import torch

from conftest import GOLDEN
from op_plan_helpers import DEV

# check_y.  fp16: score < score16 (and its 99.9th percentile < p999_16 unless None), box < box16 px -- with strides and lvl given that is
# the bound at stride 32, restated per level as box16 * max(1, stride / 32); without them it holds over the whole map.  fp32 / fp32x:
# score <= score32, box <= box32 * imgsz.
YBounds = namedtuple("YBounds", "score16 p999_16 box16 score32 box32")
# check_raw, e the largest error and mx the reference's largest magnitude.  fp16: e < or <= (strict16) rel16 * mx, mx floored at 1 where
# floor16; fp32 / fp32x: e <= rel32 * max(1, mx).
RawBounds = namedtuple("RawBounds", "rel16 strict16 floor16 rel32")

_FIXTURES, _STATE_DICTS = {}, {}


def fixture(tag):
    """(arrays, meta) of tests/golden/graph_<tag>.npz, loaded once."""
    if tag not in _FIXTURES:
        z = np.load(GOLDEN / f"graph_{tag}.npz")
        _FIXTURES[tag] = ({k: z[k] for k in z.files if k != "meta"}, json.loads(str(z["meta"])))
    return _FIXTURES[tag]


def x_of(meta, si):
    """The fixture's input of shape `si`, regenerated from its seed and checked against the checksum the generator stored."""
    b, h, w = meta["shapes"][si]
    x = torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(100 + si))
    assert abs(float(x.double().sum()) - meta["x"][si]["sum"]) < 1e-6 * x.numel() and x.flatten()[:8].tolist() == meta["x"][si]["first"]
    return x


def state_dict(tag, damp):
    """The reference's un-fused state dict (names as the fixture recorded them), values regenerated from synth_param and multiplied by
    damp(name, meta) -- the rule of the family's make_*_fixtures.py; None: no rule.  Made once per tag and shared: a caller that changes
    it takes a copy (RefModel clones every tensor)."""
    if tag not in _STATE_DICTS:
        from oracle.yolo_ref import synth_param
        meta = fixture(tag)[1]
        sd = {n: synth_param(n, s, meta["seed"]) for n, s in meta["names"]}
        if damp is not None:
            for n in sd:
                f = damp(n, meta)
                if f != 1.0:
                    sd[n] = sd[n] * f
        _STATE_DICTS[tag] = sd
    return _STATE_DICTS[tag]


def cfg_of(meta, **overrides):
    from bs_yolo_amd.graphs import stock_cfg
    return dict(stock_cfg(meta["family"], meta["scale"], meta["nc"], meta["task"]), **overrides)


def engine(tag, precision, damp, cfg=None, **kw):
    """A YoloEngine on the fixture's graph (cfg_of its meta unless the family builds `cfg` another way) and state dict."""
    from bs_yolo_amd.engine import YoloEngine
    return YoloEngine(cfg_of(fixture(tag)[1]) if cfg is None else cfg, state_dict(tag, damp), precision=precision, **kw)


def kinds(plan, kind):
    return [o for o in plan.ops if o["kind"] == kind]


def level_of_anchor(levels):
    return np.concatenate([np.full(h * w, l) for l, (h, w) in enumerate(levels)])


def check_y(y, yref, strides, lvl, imgsz, precision, what, nc, bounds):
    """The decoded map (B, 4 + nc [+ ...], A) against the reference's under `bounds` (YBounds); `lvl` the level of every anchor, or None
    (with strides None) for one box bound over the whole map.  Every figure is printed first."""
    ds = np.abs(y[:, 4:4 + nc] - yref[:, 4:4 + nc])
    es = float(ds.max())
    eb = np.abs(y[:, :4] - yref[:, :4]).max(axis=(0, 1))  # per anchor
    score = f"score {es:.2e}"
    if bounds.p999_16 is not None:
        e999 = float(np.quantile(ds, 0.999))
        score = f"score max {es:.2e} p99.9 {e999:.2e}"
    if lvl is None:
        per_level, limit = float(eb.max()), bounds.box16
        print(what, precision, f"{score} box {per_level:.2e}")
    else:
        per_level = [float(eb[lvl == l].max()) for l in range(len(strides)) if (lvl == l).any()]
        limit = np.array([bounds.box16 * max(1.0, s / 32.0) for s in strides])[lvl]
        print(what, precision, f"{score} box per level {['%.2e' % e for e in per_level]}")
    if precision == "fp16":
        assert es < bounds.score16, (what, "score", es)
        assert bounds.p999_16 is None or e999 < bounds.p999_16, (what, "score p99.9", e999)
        assert (eb < limit).all(), (what, "box", per_level)
    else:
        assert es <= bounds.score32, (what, "score", es)
        assert eb.max() <= bounds.box32 * imgsz, (what, "box", per_level)


def check_raw(got, ref, precision, what, bounds):
    """A raw level map, mask coefficients, prototypes or an inner layer against the reference's under `bounds` (RawBounds)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e, mx = np.abs(got - ref).max(), np.abs(ref).max()
    print(what, precision, f"err {e:.2e} of max {mx:.3f}")
    if precision == "fp16":
        limit = bounds.rel16 * (max(1.0, mx) if bounds.floor16 else mx)
        assert e < limit if bounds.strict16 else e <= limit, (what, e, mx)
    else:
        assert e <= bounds.rel32 * max(1.0, mx), (what, e, mx)


def check_nms(z, meta, si, y, b, h, w, precision, nc, ykey="y%d", seg=False, what=""):
    """NMS at the fixture's conf, three ways: on the fixture's own y the device NMS returns the stored rows at 1e-5; on the engine's `y` it
    is the oracle's NMS of that y bit for bit; in the fp32-storage modes the rows it keeps are the stored ones (count, classes, boxes
    within 1e-3 * imgsz, confidences -- and with `seg` the mask coefficients -- within 1e-3).  In fp16 the last is not asked: a score within
    1e-2 of the threshold may fall on either side.  -> the number of stored rows."""
    from bs_yolo_amd import nms as HN
    from oracle import postproc_ref as PP
    conf, iou = meta["nms_conf"], meta["nms_iou"]
    pinned = HN.non_max_suppression(torch.from_numpy(z[ykey % si]).to(DEV), conf, iou, nc=nc)
    mine = HN.non_max_suppression(y.float().clone(), conf, iou, nc=nc)  # (both convert xywh in place)
    oracle = PP.non_max_suppression(y.float().cpu().clone(), conf, iou, nc=nc)
    kept = 0
    for bi in range(b):
        want = z[f"nms{si}_{bi}"]
        assert tuple(pinned[bi].shape) == want.shape and np.allclose(pinned[bi].cpu().numpy(), want, atol=1e-5, rtol=0), (what, si, bi)
        assert torch.equal(mine[bi].cpu(), oracle[bi]), (what, si, bi)
        if precision != "fp16":
            g = mine[bi].cpu().numpy()
            assert g.shape == want.shape, (what, precision, si, bi, g.shape, want.shape)
            if len(g):
                print(what, precision, si, bi, f"nms rows {len(g)} box {np.abs(g[:, :4] - want[:, :4]).max():.2e} conf {np.abs(g[:, 4] - want[:, 4]).max():.2e}")
                assert np.abs(g[:, :4] - want[:, :4]).max() <= 1e-3 * max(h, w) and np.abs(g[:, 4] - want[:, 4]).max() <= 1e-3
                assert np.array_equal(g[:, 5], want[:, 5]) and (not seg or np.abs(g[:, 6:] - want[:, 6:]).max() <= 1e-3 * max(1.0, np.abs(want[:, 6:]).max()))
        kept += len(want)
    return kept


def outputs(eng, meta, dtype):
    """[y, raw map of every level] of every shape of the fixture, cloned."""
    outs = []
    for si in range(len(meta["shapes"])):
        y, raws = eng(x_of(meta, si).to(dtype).to(DEV))
        torch.cuda.synchronize()
        outs.append([y.clone()] + [r.clone() for r in raws])
    return outs


def all_equal(a, b, what):
    """Two outputs() hold the same bits (torch.equal).  Every figure is printed before the caller asserts anything."""
    same = True
    for si, (u, v) in enumerate(zip(a, b)):
        for k, (s, t) in enumerate(zip(u, v)):
            d = (s.float() - t.float()).abs()
            print(what, "shape", si, "y" if k == 0 else f"raw{k - 1}", f"differing {int((d > 0).sum())} of {d.numel()}, max {float(d.max()):.3e}")
            same = same and torch.equal(s, t)
    return same


class RefModel(torch.nn.Module):
    """Stand-in for the reference's DetectionModel: `.yaml`, the reference's parameter names with the fixture's values (cloned) on a tree
    of `module_cls` -- buffers where the leaf is a BatchNorm statistic or buffer(name, leaf, sd) says so --, and an original forward that
    only counts its calls."""

    def __init__(self, cfg, sd, module_cls=torch.nn.Module, buffer=lambda name, leaf, sd: False):
        super().__init__()
        self.yaml = cfg
        for name, t in sd.items():
            mod = self
            *path, leaf = name.split(".")
            for p in path:
                if not hasattr(mod, p):
                    mod.add_module(p, module_cls())
                mod = getattr(mod, p)
            if leaf in ("running_mean", "running_var", "num_batches_tracked") or buffer(name, leaf, sd):
                mod.register_buffer(leaf, t.clone())
            else:
                mod.register_parameter(leaf, torch.nn.Parameter(t.clone(), requires_grad=False))
        self.calls = 0
        self.eval()

    def forward(self, x, *args, **kwargs):
        self.calls += 1
        return "original"
