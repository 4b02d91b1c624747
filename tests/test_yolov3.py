"""YOLOv3 graphs on the engine (cfg/models/v3/yolov3.yaml, yolov3-spp.yaml, yolov3-tiny.yaml): the graph families, the plan lowering of the
stride-1 image conv, top-level Bottleneck (chains), SPP, nn.MaxPool2d / nn.ZeroPad2d and the 3x3 conv over an upsampled Concat operand in
all three precisions; BSY_OP_MAXPOOL (csrc/maxpool.hip), BSY_OP_CONV_FIRST with stride 1 and BSY_OP_FIRST_POOL (csrc/conv_first.hip) ALONE as
one-op plans on poisoned views; the three graphs against fixtures made by running the reference (tests/golden/make_v3_fixtures.py), the
BSY_FUSE_FIRST_POOL switch and plugin.accelerate.

MAXPOOL cases.  One lane per 16-byte piece of an output pixel, 256 lanes per workgroup, blockIdx.y the image.  Maps 2 x 2 (one window; in
mode 1 every window but the first touches the padding), 2 x 6 and 6 x 4; C = 8 and 24 at a channel offset of a wider row; batch 3; 6 x 4 x 24
channels in mode 1 is more than one workgroup in f32.  Payloads: all-negative (mode 1's border windows must return 0, the padding value),
and a random one holding a NaN and both infinities.  Bit for bit F.max_pool2d on the CPU (F.pad first in mode 1); NaN positions compared as
positions.

CONV_FIRST stride 1 / FIRST_POOL cases.  The kernel's tile is 4 x 64 outputs (2 x 32 pooled), one accumulator set per 32 couts (NT = 1 .. 4).
Images 2 x 2 (smaller than the halo), 6 x 10 (W no multiple of 4: the element-wise load path), 8 x 136 (a second tile along H and along W,
a 4-pixel group across the tile edge) and 6 x 12 at 2 elements past a 128-byte boundary (a misaligned base: the element-wise path again);
Cout 8, 16, 40, 128 (NT 1, 1, 2, 4; 8 and 40: a partial 32-cout tile); f16 and f32 images.  The kernel has no grid cap (one workgroup per
tile); FIRST_POOL also runs 3 x 64 x 1280 = 960 workgroups.
  (a) integer payload (image and bias in eighths, weights in {-1, 0, 1}), act = 0: the fp64 result bit for bit.
  (b) SiLU payload: within op_plan_helpers._bound of fp64, test_fp16_block_ops.py's per-element bound (K = 27).
  (c) the same layers in fp32 / fp32x: integers bit for bit, the SiLU payload under test_fp32_matrix_ops._reference's b1 / b2.
  (d) FIRST_POOL: bit for bit its chain CONV_FIRST stride 1 -> MAXPOOL mode 0 run as one plan on the same blob.

Graph bounds, the project's (test_ghost.py, test_p2p6.py): fp16 score < 1e-2, box < max(1, stride / 32) px per level, raw maps 3e-2 of
max(1, maximum); fp32 / fp32x 1e-3 and 1e-3 * imgsz.

Run on the MI355X box with ``pytest -m gpu``; everything else runs anywhere."""
import ctypes as C
import re
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from bs_yolo_amd import lib as L
from bs_yolo_amd.graphs import stock_cfg
from bs_yolo_amd.plan import Plan
from bs_yolo_amd.weights import pack_plan_weights, synth_state_dict
from graph_helpers import (RawBounds, RefModel, YBounds, all_equal, cfg_of, check_nms, check_raw, check_y, engine, fixture, kinds, level_of_anchor,
                           outputs, state_dict, x_of)
from op_plan_helpers import (DEV, NAN, POISON16, POISON32, _bound, _worst, assert_poison_intact, bits, conv16_op, conv16_records, conv32_op,
                             conv32_record, conv_first16_op, nchw, nhwc, new_op, poisoned, poisoned_blob, poisoned_image, run_ops, view)

gpu = pytest.mark.gpu
NC = 12
F16, F32, F64 = torch.float16, torch.float32, torch.float64
FAMILIES = {"yolov3_tiny": "yolov3-tiny", "yolov3": "yolov3", "yolov3_spp": "yolov3-spp"}
STRIDES = {"yolov3-tiny": (16, 32), "yolov3": (8, 16, 32), "yolov3-spp": (8, 16, 32)}
GRAPHS = list(FAMILIES)
PRECISIONS = ["fp16", "fp32x", "fp32"]
Y_BOUNDS = YBounds(score16=1e-2, p999_16=None, box16=1.0, score32=1e-3, box32=1e-3)  # the graph bounds of the module docstring
RAW_BOUNDS = RawBounds(rel16=3e-2, strict16=False, floor16=True, rel32=1e-3)


def _damped(name, d):
    parts = name.split(".")
    return name.endswith(d["suffix"]) and parts[0] == "model" and int(parts[1]) in d["layers"]


def _damp(name, meta):
    """The rule the generator wrote into meta["damp"] (make_v3_fixtures.py)."""
    return meta["damp"]["factor"] if _damped(name, meta["damp"]) else 1.0


def _sd_of(tag):
    return state_dict(tag, _damp)


def _cfg(meta):
    return cfg_of(meta, width_multiple=meta["width_multiple"])


def _evaluated(d):
    """The parsed yaml with every string argument that is a Python literal evaluated, as parse_model does before it builds a layer
    (nn/tasks.py:967-970): the yaml's `None` (a string to a YAML parser) becomes None, names such as nc or nearest stay."""
    import ast

    def ev(a):
        if isinstance(a, str):
            try:
                return ast.literal_eval(a)
            except (ValueError, SyntaxError):
                return a
        return a

    out = dict(d)
    for part in ("backbone", "head"):
        out[part] = [[f, n, m, [ev(a) for a in args]] for f, n, m, args in d[part]]
    return out


# ---- host side (no GPU) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", GRAPHS)
def test_stock_cfg_is_the_reference_yaml(tag):
    meta = fixture(tag)[1]
    fam = meta["family"]
    assert fam == FAMILIES[tag] and meta["scale"] is None
    for scale in (None, ""):
        cfg = stock_cfg(fam, scale, 80)
        assert cfg == _evaluated(meta["yaml"]) and "scales" not in cfg and cfg["depth_multiple"] == cfg["width_multiple"] == 1.0
    for bad in (dict(scale="n"), dict(scale="s"), dict(scale=None, task="segment"), dict(scale=None, task="obb"), dict(scale=None, task="classify")):
        with pytest.raises(ValueError):
            stock_cfg(fam, bad["scale"], 80, bad.get("task", "detect"))
    with pytest.raises(ValueError):
        stock_cfg(fam, None, 1, "pose", kpt_shape=(17, 3))
    cfg = stock_cfg(fam, None, 80)
    cfg["head"][0][3][0] = 7  # a deep copy: the table is not the caller's to change
    assert stock_cfg(fam, None, 80) == _evaluated(meta["yaml"])
    assert [l[3] for l in meta["yaml"]["head"] if l[2] == "nn.Upsample"][0] == ["None", 2, "nearest"]  # (what _evaluated is for)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", GRAPHS)
def test_v3_plans(tag, precision, monkeypatch):
    """Every family in every precision plans at 64 x 64 and 640 x 640; the matrix-pipe flops at 640 x 640, nc = 80, full width are the
    reference's own conv count within 1 % (test_ghost.py's and test_yolov9.py's margin for zero-padded pieces; these graphs have none);
    the weight records read exactly the parameter names the reference's model holds."""
    monkeypatch.delenv("BSY_FUSE_FIRST_POOL", raising=False)
    meta = fixture(tag)[1]
    fam, strides = meta["family"], STRIDES[meta["family"]]
    assert meta["stride"] == [float(s) for s in strides]
    for h in (64, 640):
        plan = Plan(stock_cfg(fam, None, 80), 1, h, h, precision=precision)
        m = plan.meta
        assert m["strides"] == [float(s) for s in strides] and m["levels"] == [(h // s, h // s) for s in strides]
        assert m["A"] == sum((h // s) ** 2 for s in strides) and m["legacy"] and m["nm"] == 0 and m["scale"] is None
    ref = meta["ref_conv_gflops_640"][fam]
    got = sum(o.get("mfma_flops", 0) for o in plan.ops) / 1e9
    print(fam, precision, f"plan {got:.4f} reference convs {ref:.4f}")
    assert abs(got - ref) <= 0.01 * ref and plan.flops / 1e9 == got
    # the fixture's graph (nc = 12, the fixture's width): what the records consume
    sd = _sd_of(tag)
    seen = set()

    class Recording(dict):
        def __getitem__(self, k):
            seen.add(k)
            return dict.__getitem__(self, k)

    plan = Plan(_cfg(meta), 1, 64, 64, precision=precision)
    assert {r.kind for r in plan.wrecs.values()} == {"conv", "first", "plain"}  # nothing new in weights.py
    pack_plan_weights(plan, Recording(sd))
    skip = lambda n: n.endswith(".dfl.conv.weight") or n.endswith("num_batches_tracked")  # noqa: E731
    assert seen == {n for n in sd if not skip(n)} == set(synth_state_dict(plan))
    assert len(plan.c_ops()) == len(plan.ops)
    if tag != "yolov3_tiny":  # parse_model's nn.Sequential of n > 1 Bottlenecks: model.<i>.<j>.cv1
        chains = {4: 2, 6: 8, 8: 8, 10: 4, 27: 2}
        for i, n in chains.items():
            assert [f"model.{i}.{j}.cv{c}" in plan.wrecs for j in range(n) for c in (1, 2)] == [True] * (2 * n) and f"model.{i}.{n}.cv1" not in plan.wrecs
        assert "model.2.cv1" in plan.wrecs and "model.11.cv2" in plan.wrecs
        d = meta["damp"]
        assert d["factor"] == 0.25 and d["layers"] == [2, 4, 6, 8, 10, 11, 19, 20, 26, 27]
        assert sum(_damped(n, d) for n in sd) == 1 + 2 + 8 + 8 + 4 + 1 + 1 + 1 + 1 + 2
    else:
        assert meta["damp"]["factor"] == 1.0 and not meta["damp"]["layers"] and not any(_damped(n, meta["damp"]) for n in sd)
    r = meta["ref_fp16"]  # the conditions the generator checked: what makes the fp16 comparison meaningful
    assert r["score"] < 5e-3 and r["box"] < 0.5 and r["raw"] < 1e-2 and r["layer_max"] < 256


def test_tiny_op_counts(monkeypatch):
    cfg = stock_cfg("yolov3-tiny", None, NC)

    def census(plan):
        pools = kinds(plan, L.OP_MAXPOOL)
        return (len(kinds(plan, L.OP_FIRST_POOL)), len(kinds(plan, L.OP_CONV_FIRST)), sum(o["level"] == 0 for o in pools),
                sum(o["level"] == 1 for o in pools))

    monkeypatch.delenv("BSY_FUSE_FIRST_POOL", raising=False)
    on = Plan(cfg, 1, 64, 64)
    assert on.fuse_first_pool and census(on) == (1, 0, 4, 1)
    fp = on.ops[0]
    assert fp["kind"] == L.OP_FIRST_POOL and fp["name"] == "model.0+1" and (fp["H"], fp["W"], fp["OH"], fp["OW"]) == (64, 64, 32, 32)
    assert (fp["ksize"], fp["stride"], fp["pad"], fp["act"], fp["dst"].C) == (3, 1, 1, 1, 16) and on.layer_out[0] is None and on.layer_out[11] is None
    assert on.wrecs[fp["wkey"]].kind == "first" and L.lib.bsy_first_pool_supported(16, 64, 64) == 1
    assert on.meta["strides"] == [16.0, 32.0] and on.meta["A"] == 20 and on.meta["levels"] == [(4, 4), (2, 2)]
    monkeypatch.setenv("BSY_FUSE_FIRST_POOL", "0")
    off = Plan(cfg, 1, 64, 64)
    assert not off.fuse_first_pool and census(off) == (0, 1, 5, 1)
    assert (off.ops[0]["kind"], off.ops[0]["stride"], off.ops[1]["kind"], off.ops[1]["level"]) == (L.OP_CONV_FIRST, 1, L.OP_MAXPOOL, 0)
    assert len(off.ops) == len(on.ops) + 1 and off.flops == on.flops and list(off.wrecs) == list(on.wrecs)
    assert [o["name"] for o in off.ops[2:]] == [o["name"] for o in on.ops[1:]]
    monkeypatch.setenv("BSY_FUSE_FIRST_POOL", "1")
    assert census(Plan(cfg, 1, 64, 64)) == (1, 0, 4, 1)
    for precision in ("fp32", "fp32x"):
        p = Plan(cfg, 1, 64, 64, precision=precision)
        assert not p.fuse_first_pool and census(p) == (0, 1, 5, 1) and p.ops[0]["stride"] == 1 and p.meta["A"] == 20
    with pytest.raises(TypeError):  # a plan attribute read from the environment like fuse_ghost, not a keyword of SWITCHES
        Plan(cfg, 1, 64, 64, fuse_first_pool=False)
    # the mode-1 pool reads layer 10's map and keeps its size; layer 19: one COPY through up0, then a two-source 3x3 conv
    last = next(o for o in on.ops if o["kind"] == L.OP_MAXPOOL and o["level"] == 1)
    assert last["name"] == "model.12" and (last["H"], last["W"], last["OH"], last["OW"]) == (2, 2, 2, 2) and last["src0"].C == 512
    copies = kinds(on, L.OP_COPY)
    c19 = next(o for o in on.ops if o["name"] == "model.19")
    assert len(copies) == 1 and copies[0]["src0"].up and not copies[0]["dst"].up and copies[0]["name"] == "model.19.up0"
    assert c19["ksize"] == 3 and c19["src0"] is copies[0]["dst"] and not c19["src0"].up and not c19["src1"].up and (c19["src0"].C, c19["src1"].C) == (128, 256)
    pack_plan_weights(on, synth_state_dict(on))
    ops = on.c_ops()
    assert [o.level for o in ops if o.kind == L.OP_MAXPOOL] == [0, 0, 0, 0, 1] and ops[0].kind == L.OP_FIRST_POOL and ops[0].stride == 1
    assert [o.up0 for o in ops if o.kind == L.OP_COPY] == [1]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_spp_op_counts(precision):
    spp = Plan(stock_cfg("yolov3-spp", None, NC), 1, 64, 64, precision=precision)
    v3 = Plan(stock_cfg("yolov3", None, NC), 1, 64, 64, precision=precision)
    assert len(kinds(spp, L.OP_SPPF_POOL)) == 1 and not kinds(v3, L.OP_SPPF_POOL)
    pool = kinds(spp, L.OP_SPPF_POOL)[0]
    assert pool["name"] == "model.12.m" and pool["src0"].C == 512 and {"model.12.cv1", "model.12.cv2"} <= set(spp.wrecs)
    assert (spp.wrecs["model.12.cv1"].cin, spp.wrecs["model.12.cv2"].cin, spp.wrecs["model.12.cv2"].cout) == (1024, 2048, 512)
    for plan in (spp, v3):  # one COPY with up0 per head Concat (layers 18 and 25), in front of cv1 of the Bottleneck that reads it
        copies = kinds(plan, L.OP_COPY)
        assert [o["name"] for o in copies] == ["model.19.cv1.up0", "model.26.cv1.up0"] and all(o["src0"].up for o in copies)
        for c, name in zip(copies, ("model.19.cv1", "model.26.cv1")):
            cv1 = next(o for o in plan.ops if o["name"] == name)
            assert cv1["ksize"] == 3 and cv1["src0"] is c["dst"] and cv1["src1"] is not None and not cv1["src1"].up
        assert not any(o["kind"] == L.OP_CONV and o["ksize"] == 3 and (o["src0"].up or (o.get("src1") is not None and o["src1"].up)) for o in plan.ops)
        assert len(kinds(plan, L.OP_BNECK)) == (1 if precision == "fp16" else 0)  # model.2 (64 -> 32 -> 64); the rest are too wide
        assert plan.ops[0]["kind"] == L.OP_CONV_FIRST and plan.ops[0]["stride"] == 1 and not kinds(plan, L.OP_STEM)


def test_what_is_refused():
    from bs_yolo_amd.plugin import graph_support, max_stride
    tiny = lambda: stock_cfg("yolov3-tiny", None, NC)  # noqa: E731
    layers = lambda cfg: cfg["backbone"] + cfg["head"]  # noqa: E731
    for precision in PRECISIONS:
        cases = []
        c = tiny(); c["backbone"][3] = [-1, 1, "nn.MaxPool2d", [3, 2, 1]]; cases.append((c, r"model\.3: nn\.MaxPool2d \[3, 2, 1\]"))
        c = tiny(); c["backbone"][3] = [-1, 1, "nn.MaxPool2d", [2, 1, 0]]; cases.append((c, r"model\.3: nn\.MaxPool2d \[2, 1, 0\]"))  # no pad in front
        c = tiny(); c["backbone"][11] = [-1, 1, "nn.ZeroPad2d", [[1, 1, 1, 1]]]; cases.append((c, r"model\.11: nn\.ZeroPad2d \[\[1, 1, 1, 1\]\]"))
        c = tiny(); c["backbone"][11] = [-1, 1, "nn.ZeroPad2d", [1]]; cases.append((c, r"model\.11: nn\.ZeroPad2d \[1\]"))
        c = tiny(); c["backbone"][12] = [-1, 1, "nn.MaxPool2d", [2, 2, 0]]; cases.append((c, r"model\.11: nn\.ZeroPad2d is accelerated only in front of"))
        c = tiny(); c["backbone"][12] = [-1, 1, "Conv", [512, 3, 1]]; cases.append((c, r"model\.11: nn\.ZeroPad2d is accelerated only in front of"))
        c = tiny(); c["head"][0] = [11, 1, "Conv", [1024, 3, 1]]; cases.append((c, r"model\.11: the output of nn\.ZeroPad2d is read by model\.13 as well"))
        c = tiny(); c["backbone"][0] = [-1, 1, "Conv", [16, 3, 1, 0]]; cases.append((c, r"image conv k=3 s=1 p=0"))
        c = tiny(); c["backbone"][0] = [-1, 1, "Conv", [16, 5, 1]]; cases.append((c, r"image conv k=5 s=1 p=2"))
        c = stock_cfg("yolov3-spp", None, NC); c["head"][1] = [-1, 1, "SPP", [512, [3, 5, 7]]]; cases.append((c, r"model\.12: SPP with k = \[3, 5, 7\]"))
        c = stock_cfg("yolov3", None, NC); c["backbone"][2] = [-1, 1, "Bottleneck", [64, True, 2]]; cases.append((c, r"model\.2: Bottleneck with g = 2"))
        c = stock_cfg("yolov3", None, NC); c["backbone"][4] = [-1, 2, "Bottleneck", [256]]; cases.append((c, r"model\.4: 2 chained Bottlenecks need an input of their own width"))
        for cfg, msg in cases:
            with pytest.raises(NotImplementedError, match=msg):
                Plan(cfg, 1, 64, 64, precision=precision)
        with pytest.raises(NotImplementedError, match=r"model\.9: MaxPool2d\(2, 2, 0\) on an odd 3 x 3 map"):
            Plan(tiny(), 1, 48, 48, precision=precision)  # 48 / 16 = 3: the fifth pool meets an odd map
        assert Plan(tiny(), 1, 96, 128, precision=precision).meta["A"] == 6 * 8 + 3 * 4
    for fam in FAMILIES.values():
        cfg = stock_cfg(fam, None, NC)
        assert graph_support(cfg) == {"fp16": True, "fp32": True} and max_stride(cfg) == 32
        assert len(layers(cfg)) == (21 if fam == "yolov3-tiny" else 29)


def test_abi():
    header = (ROOT / "include" / "bsyolo.h").read_text()
    assert re.search(r"BSY_OP_MAXPOOL\s*=\s*27\b", header) and re.search(r"BSY_OP_FIRST_POOL\s*=\s*28\b", header)
    assert re.search(r"int\s+bsy_maxpool2d\s*\(", header) and re.search(r"int\s+bsy_first_pool_supported\s*\(", header)
    assert (L.OP_MAXPOOL, L.OP_FIRST_POOL, L.OP_E2E_TOPK, L.OP_CONV_FIRST) == (27, 28, 26, 0)
    assert {"bsy_maxpool2d", "bsy_first_pool_supported"} <= set(L.SYMBOLS) and hasattr(L.lib, "bsy_maxpool2d")
    assert L.lib.bsy_sizeof_op() == C.sizeof(L.Op) == 624
    assert re.search(r'PLAN_ENV = .*"BSY_FUSE_FIRST_POOL"', (ROOT / "tools" / "plan_snapshot.py").read_text())  # the snapshots unset it too
    from bs_yolo_amd.plan import LANE_KINDS, SWITCHES
    assert "fuse_first_pool" not in SWITCHES and L.OP_FIRST_POOL not in LANE_KINDS and L.OP_MAXPOOL not in LANE_KINDS
    f = L.lib.bsy_first_pool_supported
    assert all(f(c, h, w) == 1 for c in range(8, 129, 8) for h, w in ((2, 2), (64, 64), (6, 10), (640, 640)))
    assert not any(f(c, h, w) for c, h, w in ((0, 64, 64), (12, 64, 64), (136, 64, 64), (16, 63, 64), (16, 64, 63), (16, 0, 0), (-8, 64, 64)))


# ------------------------------------------------------------------------------------------------------------
# BSY_OP_MAXPOOL alone
# ------------------------------------------------------------------------------------------------------------
POOL_MAPS = [(2, 2), (2, 6), (6, 4)]
POOL_B = 3


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 15485863 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _pool_ref(x, mode):
    """x (B, H, W, C) -> F.max_pool2d on the CPU in x's dtype (through f32, exact for a max), F.pad with zeros first in mode 1."""
    t = nchw(x.float())
    y = F.max_pool2d(F.pad(t, (0, 1, 0, 1)), 2, 1, 0) if mode else F.max_pool2d(t, 2, 2, 0)
    return nhwc(y).to(x.dtype)


def _same_bits(got, want):
    """Bit for bit outside NaN, NaN exactly where the reference has NaN (a NaN's payload is not part of ATen's contract)."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool((gn == wn).all()) and bool((bits(got) == bits(want))[~wn].all())


def _pool_payloads(H, W, Cc, dtype, mode):
    g = _gen(H, W, Cc, dtype == F16, mode)
    neg = (-torch.rand(POOL_B, H, W, Cc, generator=g) - 0.5).to(dtype)  # all negative: mode 1's border windows return the padding's 0
    mix = (torch.randn(POOL_B, H, W, Cc, generator=g) * 3).to(dtype)
    mix[0, 0, 0, 0], mix[1, H - 1, W - 1, Cc - 1], mix[2, 0, W - 1, 1] = NAN, float("inf"), float("-inf")
    mix[1, 0, 0, 2], mix[1, 0, 1, 2] = 0.0, -0.0  # of +0 / -0 the first one met stays
    return {"neg": neg, "mix": mix}


@gpu
@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("hw", POOL_MAPS, ids=lambda m: "%dx%d" % m)
@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
def test_maxpool_op(mode, dtype, hw, Cc):
    H, W = hw
    OH, OW = (H, W) if mode else (H // 2, W // 2)
    poison = POISON16 if dtype == F16 else POISON32
    lds, cs, ldd, cd = Cc + 24, 8, Cc + 40, 16
    for name, x in _pool_payloads(H, W, Cc, dtype, mode).items():
        want = _pool_ref(x, mode)
        if name == "neg" and mode:
            assert bool((want[:, -1] == 0).all()) and bool((want[:, :, -1] == 0).all()) and bool((want[:, :-1, :-1] < 0).all())
        if name == "mix":
            assert bool(torch.isnan(want[0, 0, 0, 0])) and bool(torch.isinf(want).any())
        src = poisoned((POOL_B, H, W, lds), cs, Cc, x, NAN)
        dst = poisoned((POOL_B, OH, OW, ldd), cd, Cc, None, poison, dtype=dtype)
        op = new_op(L.OP_MAXPOOL, 0 if dtype == F16 else 1, POOL_B, H, W)
        op.OH, op.OW, op.level, op.ksize, op.stride = OH, OW, mode, 2, 1 if mode else 2
        op.src0, op.dst = view(0, lds, cs, Cc), view(1, ldd, cd, Cc)
        before = src.cpu()
        run_ops([op], [src, dst])
        assert_poison_intact(dst, cd, Cc, poison)
        assert torch.equal(bits(src), bits(before)), "a store reached the source buffer"
        got = dst[..., cd:cd + Cc].cpu()
        assert _same_bits(got, want), (name, mode, hw, Cc)
        # the stand-alone entry point: the same launch
        out = poisoned((POOL_B, OH, OW, ldd), cd, Cc, None, poison, dtype=dtype)
        L.check(L.lib.bsy_maxpool2d(src.data_ptr(), lds, cs, out.data_ptr(), ldd, cd, POOL_B, H, W, Cc, mode, L.dtype_code(dtype), L.stream_ptr(DEV)))
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(dst))


@gpu
def test_maxpool_refuses_bad_arguments():
    x = torch.zeros(1, 4, 4, 16, dtype=F16, device=DEV)
    y = torch.full((1, 4, 4, 16), POISON16, dtype=F16, device=DEV)
    f = lambda *a: L.lib.bsy_maxpool2d(x.data_ptr(), *a[:2], y.data_ptr(), *a[2:], L.stream_ptr(DEV))  # noqa: E731
    #          ldx xoff ldy yoff B  H  W  C  mode dtype
    bad = [f(16, 0, 16, 0, 1, 3, 4, 16, 0, L.BSY_F16), f(16, 0, 16, 0, 1, 4, 3, 16, 0, L.BSY_F16), f(16, 0, 16, 0, 1, 4, 4, 16, 2, L.BSY_F16),
           f(16, 0, 16, 0, 1, 4, 4, 12, 0, L.BSY_F16), f(16, 4, 16, 0, 1, 4, 4, 8, 0, L.BSY_F16), f(16, 8, 16, 0, 1, 4, 4, 16, 0, L.BSY_F16),
           f(16, 0, 16, 0, 1, 4, 4, 16, 0, L.BSY_U8), f(16, 0, 16, 0, 0, 4, 4, 16, 0, L.BSY_F16), f(16, 0, 16, 0, 1, 0, 4, 16, 1, L.BSY_F16)]
    assert bad == [-1] * len(bad) and b"maxpool" in L.lib.bsy_last_error()
    op = new_op(L.OP_MAXPOOL, 0, 1, 4, 4)  # a record whose extents disagree with its mode
    op.level, op.src0, op.dst = 0, view(0, 16, 0, 16), view(1, 16, 0, 16)
    with pytest.raises(L.BsyError, match="maxpool"):
        run_ops([op], [x, y])
    torch.cuda.synchronize()
    assert bool((y.cpu() == POISON16).all())  # nothing was launched


# ------------------------------------------------------------------------------------------------------------
# BSY_OP_CONV_FIRST with stride 1, BSY_OP_FIRST_POOL
# ------------------------------------------------------------------------------------------------------------
FIRST_B = 2
FIRST_MAPS = [(2, 2, 0), (6, 10, 0), (8, 136, 0), (6, 12, 2)]  # H, W, elements past a 128-byte boundary
FIRST_COUTS = [8, 16, 40, 128]
FIRST_IDS = ["%dx%d%s" % (h, w, "-mis" if mis else "") for h, w, mis in FIRST_MAPS]
LDX = 24  # a destination view: channels [8, 8 + C) of rows of C + 24 elements


def _stage(x, w, b, act):
    """The stride-1 image conv in fp64 as test_fp16_block_ops._stage states a conv: v, a = act(v), S = |b| + sum |x||w|, K = 27."""
    x, w, b = x.to(F64), w.to(F64), b.to(F64)
    v = nhwc(F.conv2d(x, w, b, 1, 1))
    a = F.silu(v) if act else v
    S = nhwc(F.conv2d(x.abs(), w.abs(), b.abs(), 1, 1))
    return SimpleNamespace(v=v, a=a, ref=a, S=S, act=act, res=None, K=27, nsl=1, out_f32=False)


@lru_cache(maxsize=None)
def _first_payload(B, H, W, cout, exact):
    g = _gen(B, H, W, cout, exact, 3)
    if not exact:
        w = (torch.randn(cout, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5).to(F16).to(F32)
        return SimpleNamespace(x=torch.rand(B, 3, H, W, generator=g), convs=[(w, torch.randn(cout, generator=g) * 0.2)])
    draw = lambda shp, lim: torch.randint(-lim, lim + 1, shp, generator=g).float()  # noqa: E731
    x = draw((B, 3, H, W), 8) / 8
    edge = torch.zeros_like(x, dtype=torch.bool)
    edge[:, :, [0, -1]] = True
    edge[:, :, :, [0, -1]] = True
    x[edge & (x == 0)] = 0.375  # no tap hides behind a zero edge
    return SimpleNamespace(x=x, convs=[(draw((cout, 3, 3, 3), 1), draw((cout,), 8) / 8)])


def _run_first16(B, H, W, cout, idt, mis, p, act, form):
    """form "conv": CONV_FIRST stride 1 -> (B, H, W, cout); "pool": FIRST_POOL; "chain": CONV_FIRST stride 1 into slot 2, MAXPOOL mode 0
    -> (B, H / 2, W / 2, cout).  The image inside a NaN allocation, destinations in 777, the blob with NaN between its records."""
    keep, img = poisoned_image(p.x, idt, mis)
    blob, recs = conv16_records(p.convs)
    code, ld = L.dtype_code(idt), cout + LDX
    oh, ow = (H, W) if form == "conv" else (H // 2, W // 2)
    dst = poisoned((B, oh, ow, ld), 8, cout, None, POISON16, dtype=F16)
    dv, ext, mid = view(1, ld, 8, cout), [img, dst], None
    if form == "chain":
        mid = poisoned((B, H, W, ld), 8, cout, None, POISON16, dtype=F16)
        mv = view(2, ld, 8, cout)
        pool = new_op(L.OP_MAXPOOL, 0, B, H, W)
        pool.OH, pool.OW, pool.level, pool.ksize, pool.stride, pool.src0, pool.dst = oh, ow, 0, 2, 2, mv, dv
        ops, ext = [conv_first16_op(B, H, W, mv, *recs[0], code, act, stride=1), pool], ext + [mid]
    else:
        op = conv_first16_op(B, H, W, dv, *recs[0], code, act, stride=1)
        if form == "pool":
            op.kind, op.OH, op.OW = L.OP_FIRST_POOL, oh, ow
        ops = [op]
    before = keep.clone()
    run_ops(ops, ext, blob)
    assert torch.equal(bits(keep), bits(before)), "a store reached the image's allocation"
    assert_poison_intact(dst, 8, cout, POISON16)
    if mid is not None:
        assert_poison_intact(mid, 8, cout, POISON16)
    return dst[..., 8:8 + cout].cpu()


def test_first_cases_reach_every_path():
    assert any(h < 4 and w < 4 for h, w, _ in FIRST_MAPS) and any(w % 4 for _, w, _ in FIRST_MAPS) and any(m for _, _, m in FIRST_MAPS)
    assert any(h > 4 and w > 64 and w % 4 == 0 and w % 64 for h, w, _ in FIRST_MAPS) and all(not h % 2 and not w % 2 for h, w, _ in FIRST_MAPS)
    assert {(c + 31) // 32 for c in FIRST_COUTS} >= {1, 2, 4} and any(c % 32 for c in FIRST_COUTS) and max(FIRST_COUTS) == 128
    for h, w, _ in FIRST_MAPS:
        for cout in FIRST_COUTS:
            p = _first_payload(FIRST_B, h, w, cout, True)
            st = _stage(p.x, *p.convs[0], 0)
            ok = lambda v: bool((v * 8 == (v * 8).round()).all()) and float(v.abs().max()) < 64  # noqa: E731
            assert ok(p.x) and ok(st.v) and float(st.S.max()) * 8 < 2 ** 24 and float(st.v.abs().max()) > 1


@gpu
@pytest.mark.parametrize("idt", [F16, F32], ids=["img16", "img32"])
@pytest.mark.parametrize("cout", FIRST_COUTS)
@pytest.mark.parametrize("hw", FIRST_MAPS, ids=FIRST_IDS)
def test_conv_first_stride1_op(hw, cout, idt):
    H, W, mis = hw
    p = _first_payload(FIRST_B, H, W, cout, True)
    got = _run_first16(FIRST_B, H, W, cout, idt, mis, p, 0, "conv")
    want = (_stage(p.x, *p.convs[0], 0).ref + 0.0).to(F16)
    print("first s1 exact", hw, cout, f"differing {int((bits(got) != bits(want)).sum())} of {got.numel()}")
    assert torch.equal(bits(got), bits(want))
    p = _first_payload(FIRST_B, H, W, cout, False)
    got = _run_first16(FIRST_B, H, W, cout, idt, mis, p, 1, "conv")
    st = _stage(p.x.to(F16), *p.convs[0], 1)  # the values the kernel multiplies: it parks the image as f16 whatever its dtype
    r = _worst(got, st.ref, sum(_bound(st, st, False)))
    print("first s1 silu", hw, cout, f"worst error / bound = {r:.3f}")
    assert r <= 1.0
    if mis:
        assert torch.equal(bits(got), bits(_run_first16(FIRST_B, H, W, cout, idt, 0, p, 1, "conv")))


@gpu
@pytest.mark.parametrize("idt", [F16, F32], ids=["img16", "img32"])
@pytest.mark.parametrize("cout", [16, 40, 128])
@pytest.mark.parametrize("hw", FIRST_MAPS, ids=FIRST_IDS)
def test_first_pool_op_is_its_chain(hw, cout, idt):
    H, W, mis = hw
    assert L.lib.bsy_first_pool_supported(cout, H, W) == 1
    p = _first_payload(FIRST_B, H, W, cout, False)
    fused = _run_first16(FIRST_B, H, W, cout, idt, mis, p, 1, "pool")
    chain = _run_first16(FIRST_B, H, W, cout, idt, mis, p, 1, "chain")
    nd = int((bits(fused) != bits(chain)).sum())
    print("first_pool", hw, cout, f"differing {nd} of {fused.numel()}")
    assert bool(torch.isfinite(fused.float()).all()) and nd == 0
    # and the chain is the pooled conv: MAXPOOL of the map CONV_FIRST wrote, bit for bit F.max_pool2d of it
    full = _run_first16(FIRST_B, H, W, cout, idt, mis, p, 1, "conv")
    assert torch.equal(bits(chain), bits(_pool_ref(full, 0)))


@gpu
def test_first_pool_op_on_many_tiles():
    """3 x 16 x 20 = 960 workgroups (the launcher has no grid cap: one workgroup per 4 x 64 tile), against the chain."""
    B, H, W, cout = 3, 64, 1280, 16
    p = _first_payload(B, H, W, cout, False)
    fused = _run_first16(B, H, W, cout, F16, 0, p, 1, "pool")
    chain = _run_first16(B, H, W, cout, F16, 0, p, 1, "chain")
    assert bool(torch.isfinite(fused.float()).all()) and torch.equal(bits(fused), bits(chain))


@gpu
def test_first_pool_refuses_what_it_does_not_take():
    p = _first_payload(1, 6, 10, 16, False)
    for H, W, stride in ((5, 10, 1), (6, 9, 1), (6, 10, 2)):
        keep, img = poisoned_image(torch.rand(1, 3, H, W), F16)
        blob, recs = conv16_records(p.convs)
        dst = poisoned((1, H // 2, W // 2, 16), 0, 16, None, POISON16, dtype=F16)
        op = conv_first16_op(1, H, W, view(1, 16, 0, 16), *recs[0], L.BSY_F16, 1, stride=stride)
        op.kind, op.OH, op.OW = L.OP_FIRST_POOL, H // 2, W // 2
        with pytest.raises(L.BsyError, match="first_pool"):
            run_ops([op], [img, dst], blob)
        torch.cuda.synchronize()
        assert bool((dst.cpu() == POISON16).all())
        op.prec = 1
        with pytest.raises(L.BsyError, match="fp32"):  # no fp32 form: the planner never emits it there
            run_ops([op], [img, dst], blob)


@gpu
@pytest.mark.parametrize("idt", [F16, F32], ids=["img16", "img32"])
@pytest.mark.parametrize("cout", FIRST_COUTS)
@pytest.mark.parametrize("hw", FIRST_MAPS[:3], ids=FIRST_IDS[:3])
@pytest.mark.parametrize("prec", [1, 2], ids=["fp32", "fp32x"])
def test_conv_first_stride1_fp32_modes(prec, hw, cout, idt):
    """The same layers through Conv32Args (stride 1 needed no change there): integers bit for bit, the SiLU payload under the bounds
    test_fp32_matrix_ops.py derives for these modes (its _reference: b1 exact mode, b2 the split-f16 image kernel)."""
    from test_fp32_matrix_ops import _reference
    H, W, _ = hw
    B, ldd, cd = FIRST_B, cout + 16, 8
    lin = lambda xs, w_, b_: nhwc(F.conv2d(xs[0], w_, b_, 1, 1))  # noqa: E731
    for kind in ("int", "rand"):
        g = _gen(H, W, cout, idt == F16, kind == "int", prec)
        if kind == "int":
            x = torch.randint(0, 256, (B, 3, H, W), generator=g).to(idt)
            w, b = torch.randint(-2, 3, (cout, 3, 3, 3), generator=g).float(), torch.randint(-8, 9, (cout,), generator=g).float()
        else:
            x = torch.rand(B, 3, H, W, generator=g).to(idt)
            w, b = torch.randn(cout, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5, torch.randn(cout, generator=g) * 0.5
        c = _reference(lin, (x,), w, b, None, kind != "int", 27)
        keep, img = poisoned_image(x, idt)
        dst = poisoned((B, H, W, ldd), cd, cout, None, POISON32, dtype=F32)
        blob, offs = poisoned_blob(conv32_record(w, b, prec))
        op = conv32_op(prec, B, H, W, 3, 1, 1, view(0, 3, 0, 3), view(1, ldd, cd, cout), offs[0], offs[1], act=int(c.act), in_dtype=L.dtype_code(idt),
                       first=True)
        run_ops([op], [img, dst], blob)
        assert_poison_intact(dst, cd, cout, POISON32)
        got = dst[..., cd:cd + cout].cpu()
        if kind == "int":
            assert torch.equal(bits(got), bits(c.ref.to(F32)))
        else:
            r = _worst(got, c.ref, c.b2 if prec == 2 else c.b1)
            print("first s1 prec %d %s cout %d: worst error / bound = %.3f" % (prec, hw, cout, r))
            assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------
# a 3x3 conv over a Concat whose first operand is an upsampled map: COPY through up0, then two ordinary sources
# ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("prec", [0, 1, 2], ids=["fp16", "fp32", "fp32x"])
def test_two_source_3x3_after_materialised_upsample(prec):
    """The plan's form (COPY with up0 into a full-size map, then CONV 3x3 over [map | other]) against the same CONV with the first
    source upsampled by torch: the same bits, and the copied map is F.interpolate(nearest) of the small one."""
    B, H, W, C0, C1, cout = 2, 6, 10, 16, 24, 32
    dt = F16 if prec == 0 else F32
    poison = POISON16 if prec == 0 else POISON32
    g = _gen(prec, 19)
    small = torch.randn(B, H // 2, W // 2, C0, generator=g).to(dt)
    other = torch.randn(B, H, W, C1, generator=g).to(dt)
    w = (torch.randn(cout, C0 + C1, 3, 3, generator=g) * (2.0 / (9 * (C0 + C1))) ** 0.5).to(F16).to(F32)
    b = torch.randn(cout, generator=g) * 0.2
    big = nhwc(F.interpolate(nchw(small.float()), scale_factor=2.0, mode="nearest")).to(dt)
    if prec == 0:
        blob, recs = conv16_records([(w, b)])
        conv = lambda s0, s1, d: conv16_op(B, H, W, 3, 1, 1, s0, d, *recs[0], src1=s1, act=1)  # noqa: E731
    else:
        blob, offs = poisoned_blob(conv32_record(w, b, prec))
        conv = lambda s0, s1, d: conv32_op(prec, B, H, W, 3, 1, 1, s0, d, offs[0], offs[1], src1=s1, act=1)  # noqa: E731
    ld0, ld1, ldd = C0 + 8, C1 + 16, cout + 24
    outs = []
    for form in ("copy", "torch"):
        dst = poisoned((B, H, W, ldd), 8, cout, None, poison, dtype=dt)
        src1 = poisoned((B, H, W, ld1), 8, C1, other, NAN)
        if form == "copy":
            s = poisoned((B, H // 2, W // 2, ld0), 8, C0, small, NAN)
            mid = poisoned((B, H, W, ld0), 0, C0, None, poison, dtype=dt)
            cp = new_op(L.OP_COPY, prec, B, H, W)
            cp.src0, cp.up0, cp.dst = view(0, ld0, 8, C0), 1, view(3, ld0, 0, C0)
            run_ops([cp, conv(view(3, ld0, 0, C0), view(1, ld1, 8, C1), view(2, ldd, 8, cout))], [s, src1, dst, mid], blob)
            assert_poison_intact(mid, 0, C0, poison)
            assert torch.equal(bits(mid[..., :C0]), bits(big))
        else:
            s = poisoned((B, H, W, ld0), 8, C0, big, NAN)
            run_ops([conv(view(0, ld0, 8, C0), view(1, ld1, 8, C1), view(2, ldd, 8, cout))], [s, src1, dst], blob)
        assert_poison_intact(dst, 8, cout, poison)
        outs.append(dst[..., 8:8 + cout].cpu())
    assert bool(torch.isfinite(outs[0].float()).all()) and torch.equal(bits(outs[0]), bits(outs[1]))
    ref = nhwc(F.silu(F.conv2d(torch.cat([nchw(big.double()), nchw(other.double())], 1), w.double(), b.double(), 1, 1)))
    assert float((outs[0].double() - ref).abs().max()) < (2e-2 if prec == 0 else 1e-4)  # (the conv ops' own tests hold the derived bounds)


# ------------------------------------------------------------------------------------------------------------
# the graphs
# ------------------------------------------------------------------------------------------------------------
def _engine(tag, precision, **kw):
    return engine(tag, precision, _damp, cfg=_cfg(fixture(tag)[1]), **kw)


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", GRAPHS)
def test_v3_graph_matches_reference(tag, precision, monkeypatch):
    """ONE engine over both shapes: y, the raw maps of every level and NMS at the fixture's conf, as test_ghost.py compares them: on the
    fixture's own y the device NMS returns the fixture's rows; on the engine's y it is the oracle's NMS of that y bit for bit; in the
    fp32-storage modes the rows it keeps are the fixture's within the modes' bounds."""
    monkeypatch.delenv("BSY_FUSE_FIRST_POOL", raising=False)
    z, meta = fixture(tag)
    eng = _engine(tag, precision)
    kept = 0
    for si, (b, h, w) in enumerate(meta["shapes"]):
        x = x_of(meta, si)
        y, raws = eng((x.half() if precision == "fp16" else x).to(DEV))
        torch.cuda.synchronize()
        plan = eng.plan_for(b, h, w, *(2 * [F16 if precision == "fp16" else F32]))[0]
        assert bool(kinds(plan, L.OP_FIRST_POOL)) == (precision == "fp16" and tag == "yolov3_tiny")
        assert bool(kinds(plan, L.OP_MAXPOOL)) == (tag == "yolov3_tiny") and bool(kinds(plan, L.OP_SPPF_POOL)) == (tag == "yolov3_spp")
        assert kinds(plan, L.OP_COPY) and (tag == "yolov3_tiny" or plan.ops[0]["stride"] == 1)
        levels = [(h // int(s), w // int(s)) for s in meta["stride"]]
        assert tuple(y.shape) == (b, 4 + NC, sum(lh * lw for lh, lw in levels)) and len(raws) == len(levels)
        assert [tuple(r.shape) for r in raws] == [(b, 64 + NC, lh, lw) for lh, lw in levels]
        yr = y.float().cpu().numpy()
        assert np.isfinite(yr).all()
        check_y(yr, z[f"y{si}"], meta["stride"], level_of_anchor(levels), max(h, w), precision, f"{tag} shape {si}", NC, Y_BOUNDS)
        assert si in meta["raw_shapes"]
        for l, r in enumerate(raws):
            check_raw(r.float().cpu().numpy(), z[f"raw{si}_{l}"], precision, f"{tag} shape {si} raw {l}", RAW_BOUNDS)
        kept += check_nms(z, meta, si, y, b, h, w, precision, NC, what=tag)
    assert kept > 0
    eng.close()


@gpu
def test_fusion_is_not_a_different_answer(monkeypatch):
    """BSY_FUSE_FIRST_POOL = 0 and = 1 on the fp16 path of yolov3-tiny: y and the raw maps are the same bits (torch.equal)."""
    tag = "yolov3_tiny"
    _, meta = fixture(tag)
    outs = {}
    for env in ("0", "1"):
        monkeypatch.setenv("BSY_FUSE_FIRST_POOL", env)
        eng = _engine(tag, "fp16")
        outs[env] = outputs(eng, meta, F16)
        for b, h, w in meta["shapes"]:
            plan = eng.plan_for(b, h, w, F16, F16)[0]
            assert bool(kinds(plan, L.OP_FIRST_POOL)) == (env == "1") and bool(kinds(plan, L.OP_CONV_FIRST)) == (env == "0")
        eng.close()
    assert all_equal(outs["0"], outs["1"], tag), tag


@gpu
def test_accelerate_a_yolov3_tiny_model(monkeypatch):
    from bs_yolo_amd import plugin
    monkeypatch.delenv("BSY_FUSE_FIRST_POOL", raising=False)
    tag = "yolov3_tiny"
    z, meta = fixture(tag)
    m = RefModel(_cfg(meta), _sd_of(tag)).to(DEV)
    plugin.accelerate(m)
    x = x_of(meta, 1)
    b, h, w = meta["shapes"][1]
    lvl = level_of_anchor([(h // int(s), w // int(s)) for s in meta["stride"]])
    y, raws = m(x.to(DEV))  # fp32 input: the fp32x engine
    st = m._bsy_state
    assert m.calls == 0 and len(raws) == 2 and st["fp32_calls"] == 1 and st["support"] == {"fp16": True, "fp32": True}
    check_y(y.cpu().numpy(), z["y1"], meta["stride"], lvl, max(h, w), "fp32x", f"accelerate {tag}", NC, Y_BOUNDS)
    y16, raws16 = m(x.half().to(DEV))  # fp16 input: the product path, which is the engine's own output
    assert st["engine_calls"] == 1 and m.calls == 0
    eng = _engine(tag, "fp16")
    ye, re_ = eng(x.half().to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(y16, ye) and all(torch.equal(a, c) for a, c in zip(raws16, re_))
    assert kinds(st["engine"].plan_for(b, h, w, F16, F16)[0], L.OP_FIRST_POOL)
    check_y(y16.float().cpu().numpy(), z["y1"], meta["stride"], lvl, max(h, w), "fp16", f"accelerate {tag}", NC, Y_BOUNDS)
    for l, r in enumerate(raws16):
        check_raw(r.float().cpu().numpy(), z[f"raw1_{l}"], "fp16", f"accelerate {tag} raw {l}", RAW_BOUNDS)
    eng.close()
    plugin.restore(m)
