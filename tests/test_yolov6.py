"""YOLOv6 graphs on the engine (cfg/models/v6/yolov6.yaml) and ReLU, activation id 2, as a conv epilogue.

Host side (anywhere): graphs.stock_cfg("yolov6", ...) against the parsed yaml the fixtures carry; the plans of every scale in every precision
-- the chains of repeated Convs (parse_model's nn.Sequential, model.<i>.<j>), the top-level nn.ConvTranspose2d as four dst_scale = 2 phases,
and `act` per op: 2 (ReLU) on every activated conv, SPPF's two convs by Plan's sppf_act (1 by default: what a model of this fork holds, 2
for an upstream-pickled one), 0 on the decoding convs and the deconv phases --; what is refused; the weight records against the
reference's parameter names.

Ops alone (``pytest -m gpu``): BSY_OP_CONV with act = 2 as one-op plans on poisoned views, through the case tables and runners of
test_fp16_conv_ops.py / test_fp32_matrix_ops.py / test_fp16_block_ops.py (imported, not copied): one layer per fp16 kernel family with its
configuration preset and confirmed by bsy_plan_check_tuning -- implicit GEMM (LDS and direct epilogues), persistent 1x1, weights-resident
1x1, patch 3x3, split-K through splitk_reduce_kernel --, a shortcut (ReLU before the add), two sources, misaligned destinations, a
ConvTranspose2d's phases with bias (act = 0), CONV_FIRST at stride 2 and 1, STEM against its chain; every tile form of the fp32x and fp32
kernels and the scalar fall-through.  Integer (dyadic) payloads: ReLU is exact, so the output is the fp64 reference value for value (zeros
compared by value: the sign of a zero result is not specified), and all configurations of a layer agree bit for bit.  In every case
the fp64 pre-activation is negative for 25 % .. 75 % of the elements (asserted), so ReLU differs from identity and from SiLU there.

Graphs (``pytest -m gpu``): the three fixtures of tests/golden/make_v6_fixtures.py x fp16 / fp32x / fp32.  Bounds: fp16 score max 1e-2 and
p99.9 5e-3, box 1 px, raw maps 1e-2 of the map's maximum; fp32 / fp32x 1e-3 and 1e-3 * imgsz (raw maps 1e-3 of max(1, maximum)).  The
reference's own fp16 run is within half of the fp16 bounds (meta["ref_fp16"], checked by the generator).  The two SPPF forms of the same
weights differ by 6.2e-2 in a score and 14 px in a box on the larger shape (printed by the generator), so a plan with the wrong
sppf_act must MISS the bounds there.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_fp16_block_ops as TB
import test_fp16_conv_ops as T16
import test_fp32_matrix_ops as T32
from bs_yolo_amd import lib as L
from bs_yolo_amd.graphs import stock_cfg
from bs_yolo_amd.plan import Plan
from bs_yolo_amd.weights import pack_plan_weights, synth_state_dict
from graph_helpers import (RawBounds, RefModel, YBounds, all_equal, cfg_of, check_nms, check_raw, check_y, engine, fixture, kinds, level_of_anchor,
                           outputs, state_dict, x_of)
from op_plan_helpers import (DEV, POISON16, bits, bneck_op, conv16_records, conv_first16_op, new_op, poisoned, poisoned_image, run_ops, view)

gpu = pytest.mark.gpu
NC = 12
F16, F32, F64 = torch.float16, torch.float32, torch.float64
GRAPHS = ["yolov6n", "yolov6n_upstream", "yolov6m"]
SCALES = ["n", "s", "m", "l", "x"]
PRECISIONS = ["fp16", "fp32x", "fp32"]
REPEATS = {2: 6, 4: 12, 6: 18, 8: 6, 14: 9, 19: 9, 23: 9, 27: 9}  # the yaml's repeated Convs: layer -> repeats before depth scaling
DEPTH = {"n": 0.33, "s": 0.33, "m": 0.67, "l": 1.0, "x": 1.0}
ACT_KINDS = (L.OP_CONV_FIRST, L.OP_FIRST_POOL, L.OP_STEM, L.OP_CONV)
# the graph bounds of the module docstring (the box bound of 1 px is max(1, stride / 32) of every level here)
Y_BOUNDS = YBounds(score16=1e-2, p999_16=5e-3, box16=1.0, score32=1e-3, box32=1e-3)
RAW_BOUNDS = RawBounds(rel16=1e-2, strict16=False, floor16=False, rel32=1e-3)


def _damped(name, d):
    return name.startswith(d["prefix"]) and name.endswith(d["suffix"])


def _damp(name, meta):
    """The rule the generator wrote into meta["damp"] (make_v6_fixtures.py).  The two yolov6n fixtures hold the same weights."""
    return meta["damp"]["factor"] if _damped(name, meta["damp"]) else 1.0


def _sd_of(tag):
    return state_dict(tag, _damp)


def _cfg(meta):
    cfg = cfg_of(meta)
    if meta["width_multiple"] is not None:
        cfg["scales"][meta["scale"]][1] = meta["width_multiple"]
    return cfg


def _chain_len(i, scale):
    return max(round(REPEATS[i] * DEPTH[scale]), 1)


def _want_act(name, sppf):
    """The activation id the plan must give an op of an activation-carrying kind, by its name."""
    if "@" in name:  # a ConvTranspose2d phase
        return 0
    if name.startswith("model.9."):
        return sppf
    if name.startswith("model.28.") and name.endswith(".2"):  # the decoding 1x1 convs (the fused box tail is named "...1+2")
        return 0
    return 2


# ---- host side (no GPU) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_stock_cfg_is_the_reference_yaml(scale):
    for tag in GRAPHS:
        meta = fixture(tag)[1]
        want = dict(meta["yaml"])
        assert want["activation"] == "nn.ReLU()" and want["nc"] == 80 and "scale" not in want
        cfg = stock_cfg("yolov6", scale, 80)
        assert cfg.pop("scale") == scale and cfg == want
    for bad in (dict(scale="t"), dict(scale=None), dict(scale="n", task="segment"), dict(scale="n", task="classify"), dict(scale="n", task="obb")):
        with pytest.raises(ValueError):
            stock_cfg("yolov6", bad["scale"], 80, bad.get("task", "detect"))
    with pytest.raises(ValueError):
        stock_cfg("yolov6", "n", 1, "pose", kpt_shape=(17, 3))
    cfg = stock_cfg("yolov6", scale, 80)
    cfg["head"][0][3][0] = 7  # a deep copy: the table is not the caller's to change
    assert stock_cfg("yolov6", scale, 80)["head"][0][3][0] == 256


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("scale", SCALES)
def test_v6_plans(scale, precision):
    """Every scale plans in every precision at 64 x 64 and 640 x 640 (graph_support says so, max_stride is 32): the op kinds, the chains'
    names and lengths after depth scaling, the four phases of each ConvTranspose2d, and `act` per op under both SPPF forms."""
    from bs_yolo_amd.plugin import graph_support, max_stride
    cfg = stock_cfg("yolov6", scale, 80)
    assert graph_support(cfg) == {"fp16": True, "fp32": True} and max_stride(cfg) == 32
    for h in (64, 640):
        for form, sppf in (("silu", 1), ("relu", 2)):
            plan = Plan(cfg, 1, h, h, precision=precision, sppf_act=form)
            m = plan.meta
            assert m["strides"] == [8.0, 16.0, 32.0] and m["levels"] == [(h // s, h // s) for s in (8, 16, 32)] and m["legacy"] and m["scale"] == scale
            glue = {L.OP_SPPF_POOL, L.OP_DECODE, L.OP_RAW_NCHW}
            assert {o["kind"] for o in plan.ops} <= set(ACT_KINDS) | glue and len(kinds(plan, L.OP_SPPF_POOL)) == 1
            acts = [(o["name"], o["act"]) for o in plan.ops if o["kind"] in ACT_KINDS]
            assert acts and all(a == _want_act(n, sppf) for n, a in acts), [(n, a) for n, a in acts if a != _want_act(n, sppf)]
            assert [a for n, a in acts if n.startswith("model.9.")] == [sppf, sppf]
            assert sum(a == 0 for _, a in acts) == 8 + (6 if precision != "fp16" else 3)  # 2 x 4 phases; cv2.l.2 + cv3.l.2, the box tail fused in fp16
    plan = Plan(cfg, 1, 64, 64, precision=precision)
    assert plan.sppf_act == "silu"  # the default: what a model this fork builds from the yaml holds
    names = [o["name"] for o in plan.ops]
    for i in REPEATS:
        n = _chain_len(i, scale)
        assert [f"model.{i}.{j}" in plan.wrecs for j in range(n)] == [True] * n and f"model.{i}.{n}" not in plan.wrecs and f"model.{i}" not in plan.wrecs
        at = [names.index(f"model.{i}.{j}") for j in range(n)]
        assert at == list(range(at[0], at[0] + n))  # in order, nothing in between
        ops = plan.ops[at[0]:at[0] + n]
        assert all(o["ksize"] == 3 and o["stride"] == 1 and o["src0"].C == o["dst"].C and o.get("src1") is None for o in ops)
        assert all(b["src0"] is a["dst"] for a, b in zip(ops, ops[1:]))
    assert [_chain_len(i, "m") for i in REPEATS] == [4, 8, 12, 4, 6, 6, 6, 6]
    for i in (11, 16):
        ph = [o for o in plan.ops if o["name"].startswith(f"model.{i}@")]
        assert [(o["dst_scale"], o["dst_dy"], o["dst_dx"], o["ksize"], o["act"]) for o in ph] == [(2, dy, dx, 1, 0) for dy in (0, 1) for dx in (0, 1)]
        src = plan.layer_out[i - 1]
        assert all(o["src0"] is src and o["dst"].buf == plan.layer_out[i].buf and (o["dst"].H, o["dst"].W) == (src.H, src.W) for o in ph)
        assert (plan.layer_out[i].H, plan.layer_out[i].W) == (2 * src.H, 2 * src.W)
        for o in ph:
            r = plan.wrecs[o["wkey"]]
            assert (r.kind, r.name, r.cout, r.cin, r.tap) == ("deconv", f"model.{i}", plan.layer_out[i].C, src.C, (o["dst_dy"], o["dst_dx"]))
    width, max_ch = cfg["scales"][scale][1:]
    assert plan.layer_out[11].C == -(-min(256, max_ch) * width // 8) * 8 and plan.layer_out[9].C == -(-min(1024, max_ch) * width // 8) * 8
    pack_plan_weights(plan, synth_state_dict(plan))
    assert [o.act for o in plan.c_ops()] == [o.get("act", 0) for o in plan.ops]


def test_fixture_plans_and_weight_names():
    """The fixtures' graphs (nc = 12): the weight records read exactly the parameter names the reference's model holds, through the
    kinds weights.py already had."""
    for tag in GRAPHS:
        meta = fixture(tag)[1]
        sd = _sd_of(tag)
        assert meta["sppf_act"] == ("relu" if tag.endswith("upstream") else "silu") and meta["stride"] == [8.0, 16.0, 32.0]
        for precision in PRECISIONS:
            seen = set()

            class Recording(dict):
                def __getitem__(self, k):
                    seen.add(k)
                    return dict.__getitem__(self, k)

            plan = Plan(_cfg(meta), 1, 64, 64, precision=precision, sppf_act=meta["sppf_act"])
            assert {r.kind for r in plan.wrecs.values()} == {"conv", "first", "plain", "deconv"}
            pack_plan_weights(plan, Recording(sd))
            skip = lambda n: n.endswith(".dfl.conv.weight") or n.endswith("num_batches_tracked")  # noqa: E731
            assert seen == {n for n in sd if not skip(n)} == set(synth_state_dict(plan))
            assert len(plan.c_ops()) == len(plan.ops)
            if tag == "yolov6m":
                assert all(t.C % 16 == 0 for t in plan.layer_out if t is not None and not isinstance(t, list))
                assert plan.layer_out[8].C == 192 and "model.6.11" in plan.wrecs and "model.6.12" not in plan.wrecs  # max_channels 768 x 0.25
        d = meta["damp"]
        assert d["factor"] == 0.5 and sum(_damped(n, d) for n in sd) == 6
        r = meta["ref_fp16"]  # the conditions the generator checked: half of the fp16 bounds below
        assert r["score"] < 5e-3 and r["box"] < 0.5 and r["raw"] < 5e-3 and r["layer_max"] < 256
    a, b = _sd_of("yolov6n"), _sd_of("yolov6n_upstream")
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_activation_key():
    v8 = stock_cfg("yolov8", "n", NC)
    for precision in PRECISIONS:
        with pytest.raises(NotImplementedError, match=r"model\.2: C2f under activation nn\.ReLU\(\)"):
            Plan(dict(v8, activation="nn.ReLU()"), 1, 64, 64, precision=precision)
        with pytest.raises(NotImplementedError, match=r"nn\.Hardswish\(\)"):
            Plan(dict(v8, activation="nn.Hardswish()"), 1, 64, 64, precision=precision)
        with pytest.raises(NotImplementedError, match=r"nn\.LeakyReLU\(0\.1\)"):
            Plan(dict(stock_cfg("yolov6", "n", NC), activation="nn.LeakyReLU(0.1)"), 1, 64, 64, precision=precision)
        plain, silu = Plan(v8, 1, 64, 64, precision=precision), Plan(dict(v8, activation="nn.SiLU()"), 1, 64, 64, precision=precision)
        for p in (plain, silu):
            pack_plan_weights(p, synth_state_dict(p))
        assert bytes(plain.c_ops()) == bytes(silu.c_ops()) and plain.buf_bytes == silu.buf_bytes and list(plain.wrecs) == list(silu.wrecs)
        assert Plan(v8, 1, 64, 64, precision=precision, sppf_act="relu").ops == plain.ops  # read under a ReLU graph alone
    with pytest.raises(NotImplementedError, match=r"model\.2: C3k2 under activation"):
        Plan(dict(stock_cfg("yolo11", "n", NC), activation="nn.ReLU()"), 1, 64, 64)
    for fam, first in (("yolov8-ghost", r"model\.1: GhostConv"), ("yolov10", r"model\.2: C2f"), ("yolov3", r"model\.2: Bottleneck")):
        with pytest.raises(NotImplementedError, match=first + " under activation"):
            Plan(dict(stock_cfg(fam, "n" if fam != "yolov3" else None, NC), activation="nn.ReLU()"), 1, 64, 64)
    with pytest.raises(NotImplementedError, match=r"Segment under activation"):
        c = stock_cfg("yolov6", "n", NC)
        c["head"][-1] = [[19, 23, 27], 1, "Segment", ["nc", 32, 256]]
        Plan(c, 1, 64, 64)
    with pytest.raises(ValueError, match="sppf_act"):
        Plan(stock_cfg("yolov6", "n", NC), 1, 64, 64, sppf_act="gelu")
    # yolov3-tiny is Conv / pool / Concat / Detect only: under ReLU it plans, with the first-pool fusion carrying the id
    tiny = Plan(dict(stock_cfg("yolov3-tiny", None, NC), activation="nn.ReLU()"), 1, 64, 64)
    assert tiny.ops[0]["kind"] == L.OP_FIRST_POOL and tiny.ops[0]["act"] == 2
    assert all(o["act"] == (0 if o["name"].startswith("model.20.") and o["name"].endswith(".2") else 2) for o in tiny.ops if o["kind"] in ACT_KINDS)


def test_chain_and_deconv_refusals():
    v6 = lambda: stock_cfg("yolov6", "s", NC)  # noqa: E731
    for precision in PRECISIONS:
        cases = []
        c = v6(); c["backbone"][2] = [-1, 6, "Conv", [256, 3, 1]]; cases.append((c, r"model\.2: 2 chained Convs need an input of their own width \(128 channels\)"))
        c = v6(); c["backbone"][0] = [-1, 6, "Conv", [64, 3, 2]]; cases.append((c, r"model\.0: an image conv repeated 2 times"))
        c = v6(); c["head"][3] = [-1, 9, "Conv", [256, 3, 1]]; cases.append((c, r"model\.13: 3 chained Convs need an input of their own width"))  # reads a Concat
        for args in ([256, 3, 2, 0], [256, 2, 1, 0], [256, 2, 2, 1], [256, 2, 2, 0, 1], [256, 2, 2, 0, 0, 2], [256, 2, 2, 0, 0, 1, False], [256, 4, 2, 1]):
            c = v6(); c["head"][1] = [-1, 1, "nn.ConvTranspose2d", args]
            cases.append((c, r"model\.11: nn\.ConvTranspose2d \[" + str(args[0])))
        c = v6(); c["head"][1] = [-1, 6, "nn.ConvTranspose2d", [256, 2, 2, 0]]; cases.append((c, r"model\.11: nn\.ConvTranspose2d"))  # n = 2 at depth 0.33
        c = v6(); c["head"][6] = [[-1, 4], 1, "nn.ConvTranspose2d", [128, 2, 2, 0]]; cases.append((c, r"model\.16: nn\.ConvTranspose2d on a Concat"))
        for cfg, msg in cases:
            with pytest.raises(NotImplementedError, match=msg):
                Plan(cfg, 1, 64, 64, precision=precision)
        c = v6(); c["head"][1] = [-1, 1, "nn.ConvTranspose2d", [256, 2, 2, 0, 0, 1, True, 1]]
        assert len(Plan(c, 1, 64, 64, precision=precision).ops) == len(Plan(v6(), 1, 64, 64, precision=precision).ops)
    # a repeated Conv outside YOLOv6: lowered n times now, not once
    p = Plan({"nc": NC, "backbone": [[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "Conv", [32, 3, 2]], [-1, 3, "Conv", [32, 3, 1]]],
              "head": [[-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [64, 3, 2]], [[2, 3, 4], 1, "Detect", ["nc"]]]}, 1, 64, 64,
             fuse_stem=False)
    assert [o["name"] for o in p.ops[:5]] == ["model.0", "model.1", "model.2.0", "model.2.1", "model.2.2"] and all(o["act"] == 1 for o in p.ops[:5])


def test_entry_points_check_the_range_of_act():
    """The stand-alone calls refuse an `act` outside their range before they look at anything else (null pointers here): 0 .. 2 for the
    conv, image-conv and stem calls, 0 / 1 for the kernels that read it as a SiLU switch -- where 2 would run SiLU and say nothing."""
    calls = {"bsy_conv2d": (13, 2), "bsy_conv2d_f32": (13, 2), "bsy_conv2d_f32x": (15, 2), "bsy_conv_first_f32": (12, 2), "bsy_conv_first": (12, 2),
             "bsy_stem_fused": (13, 2), "bsy_bottleneck_fused": (13, 1), "bsy_dwconv": (14, 1), "bsy_dwpw_fused": (13, 1), "bsy_dwconv3x3": (10, 1)}
    for name, (at, top) in calls.items():
        fn = getattr(L.lib, name)
        for act, refused in ((-1, True), (top + 1, True), (top, False), (0, False)):
            args = [None if t is C.c_void_p else 0 for t in fn.argtypes]
            args[at] = act
            assert fn(*args) != 0  # (null pointers: every call fails, the message says why)
            msg = L.lib.bsy_last_error().decode(errors="replace")
            assert (f"act = {act}" in msg) == refused, (name, act, msg)


# ------------------------------------------------------------------------------------------------------------
# ops alone: act = 2
# ------------------------------------------------------------------------------------------------------------
def _relu_ref(v, res=None):
    """fp64 ReLU(v) (+ res) and the condition that makes the case tell ReLU from identity and from SiLU."""
    neg = float((v < 0).double().mean())
    assert 0.25 <= neg <= 0.75, neg
    y = torch.where(v < 0, torch.zeros_like(v), v)
    return (y + res.to(F64) if res is not None else y), neg


def _same_values(got, ref):
    """Every element finite and equal to the fp64 reference's VALUE (-0 == +0), which for non-zero values of one format is bit for bit."""
    g = got.to(F64)
    return bool(torch.isfinite(g).all()) and bool((g == ref).all())


def _with_act(c, act):
    c2 = SimpleNamespace(**vars(c))
    c2.act = act
    return c2


RELU16 = [  # (layer of test_fp16_conv_ops.LAYERS, configuration ids to preset, the families they are)
    ("cat1x1-64up+32-48", (0x11, 0x22, 0x81, 0x92, 0xF1), {"gemm", "persist", "wres"}),      # two sources, one read through nearest x2
    ("cat1x1-64up+32-136", (0x21, 0x42, 0x82, 0xE1, 0xF2), {"gemm", "persist", "wres"}),
    ("gen1x1-40up+8-68", (0x00, 0x10, 0x30), {"gemm"}),                                      # Cout % 8: conv_epilogue's narrow stores
    ("gen3x3-24-s2", (0x00, 0x20), {"gemm"}),
    ("k3s1-64-72", (0x15, 0x46, 0xA1, 0xB1, 0xD2), {"gemm", "patch"}),
    ("k3s1-96-72-res", (0x15, 0x26, 0xB2, 0xC1), {"gemm", "patch"}),                         # a shortcut: ReLU before the add
    ("k3s2-64+64-256", (0x15, 0x47, 0x77), {"gemm"}),
    ("split2x3-k3s1-32+96-64", (0x15, 0x36), {"gemm"}),                                      # splitk_reduce_kernel, shortcut, two sources
    ("split8x1-1x1-512-72", (0x11, 0x23), {"gemm"}),
    ("m4-cat1x1-64up+32-48", (0x11, 0x22), {"gemm"}),                                        # misaligned destination: the direct epilogue
    ("ld4-k3s1-64-72-res", (0x15, 0x26), {"gemm"}),
]


def _layer16(name):
    return next(ly for ly in T16.LAYERS if ly.name == name)


def test_relu16_cases_are_valid_and_sign_balanced():
    """The ids listed are valid for their layers by test_fp16_conv_ops.cfg_valid, every fp16 family is there, and every payload of the
    op tests below meets the 25 % .. 75 % condition (the assertions of _relu_ref), checked here where no GPU is needed."""
    fams = set()
    for name, ids, want in RELU16:
        ly = _layer16(name)
        assert set(ids) <= set(ly.ids) and all(T16.cfg_valid(ly, i) for i in ids) and {T16.cfg_row(i).fam for i in ids} == want, name
        fams |= want | ({"split"} if ly.nsl > 1 else set()) | ({"res"} if ly.res else set()) | ({"two"} if ly.C1 else set()) | {ly.place}
        c = T16._case(ly.payload, "int")
        ref, _ = _relu_ref(c.v, c.res)
        assert float(ref.abs().max()) <= 2048 and bool((ref == ref.round()).all())
    assert fams >= {"gemm", "persist", "wres", "patch", "split", "res", "two", "m4", "ld4"}
    for prec, ly in RELU32:
        c = T32._conv_case(ly.payload, "int")
        _relu_ref(_v32(c), c.res)
    forms = {T32.route(p, ly) for p, ly in RELU32}
    assert forms >= {"scalar", "mfma-thin", "mfma-64", "mfma-128", "x-thin", "x-64", "x-128", "x-big128-bk16", "x-big128-bk32", "x-big256-bk16",
                     "x-big256-bk32", "patch"}, forms
    for cs in IMAGE_CASES:
        _image_ref(cs)


@gpu
@pytest.mark.parametrize("name,ids", [(n, i) for n, i, _ in RELU16], ids=[n for n, _, _ in RELU16])
def test_conv16_relu_exact(name, ids):
    ly = _layer16(name)
    c = T16._case(ly.payload, "int")
    ref, neg = _relu_ref(c.v, c.res)
    outs = T16._run(ly, _with_act(c, 2), ids=ids, refused=())
    assert set(outs) == set(ids)
    for cfg, got in outs.items():
        print("relu16 %s 0x%02x [%s]: %.0f %% of the pre-activations negative" % (name, cfg, T16.cfg_row(cfg).fam, 100 * neg))
        assert _same_values(got, ref), "%s under 0x%02x" % (name, cfg)
        assert torch.equal(bits(got), bits(outs[ids[0]])), "%s: 0x%02x and 0x%02x differ" % (name, cfg, ids[0])


@gpu
@pytest.mark.parametrize("name,cfg", [("k3s1-64-72", 0x15), ("k3s1-64-72", 0xB1), ("cat1x1-64up+32-48", 0x81), ("cat1x1-64up+32-48", 0xF1),
                                      ("gen1x1-40up+8-68", 0x00)])
def test_conv16_act_2_is_not_silu(name, cfg):
    """The same op under act = 1 and act = 2: different outputs, and nothing negative under ReLU.  (Before id 2 existed every epilogue
    tested `act` for truth: both ran SiLU and returned the same bits.)"""
    ly = _layer16(name)
    assert not ly.res
    c = T16._case(ly.payload, "int")
    silu = T16._run(ly, _with_act(c, 1), ids=(cfg,), refused=())[cfg]
    relu = T16._run(ly, _with_act(c, 2), ids=(cfg,), refused=())[cfg]
    assert bool(torch.isfinite(silu.float()).all()) and bool((silu.float() < 0).any())
    assert not torch.equal(bits(silu), bits(relu)) and float(relu.float().min()) >= 0.0 and bool(torch.isfinite(relu.float()).all())
    assert float((silu.double() - torch.nn.functional.silu(c.v)).abs().max()) < 1.0  # and act = 1 is still SiLU


@gpu
@pytest.mark.parametrize("name,ids", [("deconv-64-64", (0x11, 0x33, 0x63)), ("deconv-40-136", (0x00, 0x20))])
def test_deconv_phases_with_bias(name, ids):
    """The four dst_scale = 2 phases (act = 0, bias) that Plan.deconv emits for Proto.upsample and for YOLOv6's top-level upsamplers."""
    ly = _layer16(name)
    c = T16._case(ly.payload, "int")
    assert bool((c.b != 0).any()) and ly.deconv
    for cfg, got in T16._run(ly, _with_act(c, 0), ids=ids, refused=()).items():
        assert torch.equal(bits(got), bits(c.ref.to(F16))), hex(cfg)


IMAGE_CASES = [TB.Case("first", "first-s2-22x70-c72", 2, 22, 70, (72,)), TB.Case("first", "first-s2-9x37-c104-f32", 3, 9, 37, (104,), F32),
               TB.Case("first", "first-s1-6x10-c40", 2, 6, 10, (40,)), TB.Case("first", "first-s1-8x136-c128", 2, 8, 136, (128,)),
               TB.Case("stem", "stem-37x52-32-64", 2, 37, 52, (32, 64)), TB.Case("stem", "stem-16x132-16-32-f32", 2, 16, 132, (16, 32), F32)]


def _image_ref(cs):
    """fp64 ReLU chain of an image case on test_fp16_block_ops' dyadic payload -> (payload, reference); stride 1 for the "-s1-" cases."""
    p = TB._payload(cs.payload, True)
    s = 1 if "-s1-" in cs.name else 2
    ref, _ = _relu_ref(TB._stage(p.x, *p.convs[0], s, 0).v)
    if cs.kind == "stem":
        ref, _ = _relu_ref(TB._stage(TB.nchw(ref), *p.convs[1], 2, 0).v)
    assert bool((ref * 32 == (ref * 32).round()).all()) and float(ref.max()) < 64
    return p, ref


@gpu
@pytest.mark.parametrize("cs", IMAGE_CASES, ids=[cs.name for cs in IMAGE_CASES])
def test_image_ops_relu_exact(cs):
    """CONV_FIRST at stride 2 and 1 and STEM with act = 2; STEM returns the bits of its chain CONV_FIRST -> CONV, both with act = 2."""
    p, ref = _image_ref(cs)
    if "-s1-" in cs.name:
        B, H, W, co = cs.B, cs.H, cs.W, cs.widths[0]
        keep, img = poisoned_image(p.x, cs.idt, 0)
        dst, dv, drng = TB._dst(B, H, W, co)
        blob, recs = conv16_records(p.convs)
        run_ops([conv_first16_op(B, H, W, dv, *recs[0], L.dtype_code(cs.idt), act=2, ksize=3, stride=1, pad=1)], [img, dst], blob)
        got = TB._take(dst, drng)
    else:
        got, _ = TB._go_image(cs, p, 2)
    assert _same_values(got, ref)
    if cs.kind == "stem":
        chain, mids = TB._go_image(cs, p, 2, chain=True)
        assert torch.equal(bits(got), bits(chain)) and float(mids[0].float().min()) >= 0.0


RELU32_NAMES = ["cat1x1-64+32-up10-24", "cat1x1-64+32-up10-48", "cat1x1-64+32-up10-136", "cat3x3-s2", "big1-1x1-136", "big1-1x1-136-bk16", "big2-1x1-264",
                "big2-1x1-264-bk16", "big1-3x3-136", "res3x3-view", "res3x3-view-nopatch", "res1x1-self", "cat1x1-cout6", "off2-res1x1-self"]
RELU32 = [(p, ly) for ly in T32.LAYERS if ly.name in RELU32_NAMES for p in (1, 2)]


def _v32(c):
    d = lambda t: None if t is None else t.to(F64)  # noqa: E731
    return c.lin(tuple(d(x) for x in c.xs), d(c.w), d(c.b))


@gpu
@pytest.mark.parametrize("prec,ly", RELU32, ids=["prec%d-%s" % (p, ly.name) for p, ly in RELU32])
def test_conv32_relu_exact(prec, ly, monkeypatch):
    """Every tile form of conv32_mfma.hip / conv32x_mfma.hip and the scalar kernel of ref32.hip with act = 2, on integers."""
    c = T32._conv_case(ly.payload, "int")
    ref, neg = _relu_ref(_v32(c), c.res)
    got, _ = T32._run_conv(prec, ly, _with_act(c, 2), monkeypatch)
    print("relu32 prec %d %s [%s]: %.0f %% negative" % (prec, ly.name, T32.route(prec, ly), 100 * neg))
    assert got.dtype == F32 and _same_values(got, ref), T32.route(prec, ly)
    silu, _ = T32._run_conv(prec, ly, _with_act(c, 1), monkeypatch)
    assert not torch.equal(bits(silu), bits(got))


def _create(ops):
    """bsy_plan_create alone on a list of ops -> status (the plan, if any, is destroyed)."""
    blob = b"\0" * 256
    eng, plan = C.c_void_p(), C.c_void_p()
    L.check(L.lib.bsy_engine_create(0, C.byref(eng)))
    try:
        L.check(L.lib.bsy_engine_load_weights(eng, (C.c_char * len(blob)).from_buffer_copy(blob), len(blob)))
        rc = L.lib.bsy_plan_create(eng, (L.Op * len(ops))(*ops), len(ops), None, 0, C.byref(plan))
        msg = L.lib.bsy_last_error().decode(errors="replace") if rc else ""
    finally:
        if plan:
            L.lib.bsy_plan_destroy(plan)
        L.lib.bsy_engine_destroy(eng)
    return rc, msg


@gpu
def test_act_2_is_refused_where_act_is_a_switch():
    """A plan holding a BNECK -- or any kind that reads `act` as 0 / 1 -- with act = 2 is refused at creation, by name; the kinds that
    give the field another meaning keep theirs, and the four activation kinds take 0 .. 2."""
    conv = new_op(L.OP_CONV, 0, 1, 4, 4)
    bn = bneck_op(1, 4, 4, view(0, 32, 0, 32), view(1, 32, 0, 32), 16, (0, 0), (0, 0), act=2)
    rc, msg = _create([conv, bn])
    assert rc != 0 and "op 1 (BNECK) has act = 2" in msg, msg
    with pytest.raises(L.BsyError, match="BNECK"):
        run_ops([bn], [torch.zeros(1, 4, 4, 32, dtype=F16, device=DEV), torch.zeros(1, 4, 4, 32, dtype=F16, device=DEV)])
    names = {L.OP_DWCONV: "DWCONV", L.OP_DWPW: "DWPW", L.OP_C3K2: "C3K2", L.OP_GHOST: "GHOST", L.OP_PMSFA_TAIL: "PMSFA_TAIL", L.OP_COPY: "COPY",
             L.OP_MSCA_SPATIAL: "MSCA_SPATIAL", L.OP_SPPF_POOL: "SPPF_POOL"}
    for kind, name in names.items():
        op = new_op(kind, 0, 1, 4, 4)
        op.act = 2
        rc, msg = _create([op])
        assert rc != 0 and f"({name}) has act = 2" in msg, (name, msg)
        op.act = 1
        assert _create([op])[0] == 0, name
    for kind in ACT_KINDS:
        for act, ok in ((0, True), (1, True), (2, True), (3, False), (-1, False)):
            op = new_op(kind, 0, 1, 4, 4)
            op.act = act
            assert (_create([op])[0] == 0) == ok, (kind, act)
    for kind, act in ((L.OP_DWCONV_G, 40), (L.OP_DECODE, 3), (L.OP_ATTN, 1)):
        op = new_op(kind, 0, 1, 4, 4)
        op.act = act
        assert _create([op])[0] == 0, kind


# ------------------------------------------------------------------------------------------------------------
# the graphs
# ------------------------------------------------------------------------------------------------------------
def _engine(tag, precision, **kw):
    meta = fixture(tag)[1]
    kw.setdefault("sppf_act", meta["sppf_act"])
    return engine(tag, precision, _damp, cfg=_cfg(meta), **kw)


def _errors(y, yref):
    ds = np.abs(y[:, 4:4 + NC] - yref[:, 4:4 + NC])
    return float(ds.max()), float(np.quantile(ds, 0.999)), np.abs(y[:, :4] - yref[:, :4]).max(axis=(0, 1))


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", GRAPHS)
def test_v6_graph_matches_reference(tag, precision):
    """ONE engine over both shapes: y, the raw maps of every level and NMS at the fixture's conf, as test_yolov3.py compares them: on the
    fixture's own y the device NMS returns the stored rows in every precision; on the engine's y it is the oracle's NMS of that y bit for
    bit; and the rows it keeps of the engine's y are the stored rows (count, classes, boxes and confidences within the modes' bounds) in
    the fp32-storage modes.  In fp16 that last comparison is not made: a score within 1e-2 of the threshold may fall on either side."""
    z, meta = fixture(tag)
    eng = _engine(tag, precision)
    assert eng.sppf_act == meta["sppf_act"]
    kept = 0
    for si, (b, h, w) in enumerate(meta["shapes"]):
        x = x_of(meta, si)
        y, raws = eng((x.half() if precision == "fp16" else x).to(DEV))
        torch.cuda.synchronize()
        plan = eng.plan_for(b, h, w, *(2 * [F16 if precision == "fp16" else F32]))[0]
        assert bool(kinds(plan, L.OP_STEM)) == (precision == "fp16") and len([o for o in plan.ops if o.get("dst_scale") == 2]) == 8
        assert [o["act"] for o in plan.ops if o["name"] in ("model.9.cv1", "model.9.cv2")] == 2 * [2 if meta["sppf_act"] == "relu" else 1]
        levels = [(h // int(s), w // int(s)) for s in meta["stride"]]
        assert tuple(y.shape) == (b, 4 + NC, sum(lh * lw for lh, lw in levels)) and len(raws) == len(levels)
        assert [tuple(r.shape) for r in raws] == [(b, 64 + NC, lh, lw) for lh, lw in levels]
        yr = y.float().cpu().numpy()
        assert np.isfinite(yr).all()
        check_y(yr, z[f"y{si}"], meta["stride"], level_of_anchor(levels), max(h, w), precision, f"{tag} shape {si}", NC, Y_BOUNDS)
        for l, r in enumerate(raws):
            check_raw(r.float().cpu().numpy(), z[f"raw{si}_{l}"], precision, f"{tag} shape {si} raw {l}", RAW_BOUNDS)
        kept += check_nms(z, meta, si, y, b, h, w, precision, NC, what=tag)
    assert kept > 0
    eng.close()


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag,wrong", [("yolov6n_upstream", "silu"), ("yolov6n", "relu")])
def test_wrong_sppf_form_misses(tag, wrong, precision):
    """The flag does something: the upstream-form fixture under sppf_act = "silu", and the fork's under "relu", are outside the bounds
    on the larger shape (the two references differ by 6.2e-2 in a score and 14 px in a box there), in every precision."""
    z, meta = fixture(tag)
    assert meta["sppf_act"] != wrong
    eng = _engine(tag, precision, sppf_act=wrong)
    x = x_of(meta, 1)
    y, _ = eng((x.half() if precision == "fp16" else x).to(DEV))
    torch.cuda.synchronize()
    es, e999, eb = _errors(y.float().cpu().numpy(), z["y1"])
    print(tag, "under", wrong, precision, f"score max {es:.2e} box max {eb.max():.2e}")
    assert es > 1e-2 and eb.max() > 1.0
    eng.close()


@gpu
@pytest.mark.parametrize("switch", ["fuse_stem", "fuse_head"])
def test_fusion_is_not_a_different_answer(switch):
    """Stem and head fusion carry the ReLU id: on and off return the same bits on the fp16 path."""
    tag = "yolov6n"
    meta = fixture(tag)[1]
    outs = {}
    for on in (False, True):
        eng = _engine(tag, "fp16", **{switch: on})
        outs[on] = outputs(eng, meta, F16)
        plan = eng.plan_for(*meta["shapes"][1], F16, F16)[0]
        assert (bool(kinds(plan, L.OP_STEM)) == on) if switch == "fuse_stem" else (bool(kinds(plan, L.OP_DECODE)) != on)
        assert all(o["act"] == _want_act(o["name"], 1) for o in plan.ops if o["kind"] in ACT_KINDS)
        eng.close()
    assert all_equal(outs[False], outs[True], f"{tag} {switch}")


@gpu
def test_first_pool_fusion_under_relu(monkeypatch):
    """BSY_OP_FIRST_POOL with act = 2 (a yolov3-tiny graph with `activation: nn.ReLU()`): the bits of its unfused chain."""
    from bs_yolo_amd.engine import YoloEngine
    cfg = dict(stock_cfg("yolov3-tiny", None, NC), activation="nn.ReLU()")
    sd = synth_state_dict(Plan(cfg, 1, 64, 64))
    meta = fixture("yolov6n")[1]
    outs = {}
    for env in ("0", "1"):
        monkeypatch.setenv("BSY_FUSE_FIRST_POOL", env)
        eng = YoloEngine(cfg, sd)
        outs[env] = outputs(eng, meta, F16)
        plan = eng.plan_for(*meta["shapes"][1], F16, F16)[0]
        assert bool(kinds(plan, L.OP_FIRST_POOL)) == (env == "1") and plan.ops[0]["act"] == 2
        eng.close()
    assert all_equal(outs["0"], outs["1"], "yolov3-tiny under ReLU, first pool")
    assert float(outs["1"][1][0][:, 4:].float().max()) > 0 and bool(torch.isfinite(outs["1"][1][0].float()).all())


@gpu
@pytest.mark.parametrize("tag", ["yolov6n", "yolov6m"])
def test_tuned_equals_untuned(tag):
    meta = fixture(tag)[1]
    outs = {}
    for tune in (False, True):
        eng = _engine(tag, "fp16", autotune=tune)
        outs[tune] = outputs(eng, meta, F16)
        eng.close()
    assert all_equal(outs[False], outs[True], f"{tag} tuned / untuned")


class _Seq(torch.nn.Module):
    def __getitem__(self, i):
        return getattr(self, str(i))


class V6Model(RefModel):
    """RefModel for yolov6.yaml: an `act` on every Conv module (a module holding `conv` and `bn`) -- nn.ReLU(), SPPF's cv1 / cv2 nn.SiLU()
    unless sppf_act = "relu" --, and layers indexable as model.model[i]."""

    def __init__(self, cfg, sd, sppf_act="silu"):
        super().__init__(cfg, sd, module_cls=_Seq)
        for name, mod in list(self.named_modules()):
            if hasattr(mod, "conv") and hasattr(mod, "bn"):
                mod.act = torch.nn.SiLU() if name.startswith("model.9.") and sppf_act == "silu" else torch.nn.ReLU()
        self.eval()


@gpu
@pytest.mark.parametrize("tag", ["yolov6n", "yolov6n_upstream"])
def test_accelerate_a_yolov6_model(tag):
    from bs_yolo_amd import plugin
    z, meta = fixture(tag)
    form = meta["sppf_act"]
    m = V6Model(_cfg(meta), _sd_of(tag), form).to(DEV)
    assert isinstance(m.model[9].cv1.act, torch.nn.ReLU if form == "relu" else torch.nn.SiLU) and isinstance(m.model[0].act, torch.nn.ReLU)
    plugin.accelerate(m)
    st = m._bsy_state
    assert st["sppf_act"] == form and st["support"] == {"fp16": True, "fp32": True}
    x = x_of(meta, 1)
    b, h, w = meta["shapes"][1]
    lvl = level_of_anchor([(h // int(s), w // int(s)) for s in meta["stride"]])
    y, raws = m(x.to(DEV))  # fp32 input: the fp32x engine
    assert m.calls == 0 and len(raws) == 3 and st["fp32_calls"] == 1 and st["sppf_act"] == form and st["engine32"].sppf_act == form
    check_y(y.cpu().numpy(), z["y1"], meta["stride"], lvl, max(h, w), "fp32x", f"accelerate {tag}", NC, Y_BOUNDS)
    y16, raws16 = m(x.half().to(DEV))  # fp16 input: the product path
    assert st["engine_calls"] == 1 and m.calls == 0 and st["engine"].sppf_act == form
    check_y(y16.float().cpu().numpy(), z["y1"], meta["stride"], lvl, max(h, w), "fp16", f"accelerate {tag}", NC, Y_BOUNDS)
    for l, r in enumerate(raws16):
        check_raw(r.float().cpu().numpy(), z[f"raw1_{l}"], "fp16", f"accelerate {tag} raw {l}", RAW_BOUNDS)
    # an in-place weight change rebuilds the engine, and the new weights are the ones that run
    n = st["rebuilds"]
    with torch.no_grad():
        m.model[10].conv.weight.mul_(0.5)
    y2, _ = m(x.half().to(DEV))
    assert st["rebuilds"] == n + 1 and not torch.equal(y2, y16) and m.calls == 0
    plugin.restore(m)
    assert m(x.to(DEV)) == "original"


@gpu
def test_accelerate_refuses_a_swapped_activation():
    """One top-level Conv's act swapped to nn.SiLU(), or SPPF's two convs disagreeing: NotImplementedError before anything is rebound."""
    from bs_yolo_amd import plugin
    meta = fixture("yolov6n")[1]
    for where, msg in (("model.4.1", r"model\.4\.1: the module's activation is SiLU\(\), the plan runs act = 2"),
                       ("model.9.cv2", r"SPPF convs disagree on their activation"),
                       ("model.28.cv3.1.0", r"model\.28\.cv3\.1\.0: the module's activation is SiLU")):
        m = V6Model(_cfg(meta), _sd_of("yolov6n")).to(DEV)
        mod = m.get_submodule(where)
        mod.act = torch.nn.ReLU() if isinstance(mod.act, torch.nn.SiLU) else torch.nn.SiLU()
        fwd = m.forward
        with pytest.raises(NotImplementedError, match=msg):
            plugin.accelerate(m)
        assert not hasattr(m, "_bsy_state") and not hasattr(m, "_bsy_orig_forward") and m.forward == fwd
        assert m(x_of(meta, 0).to(DEV)) == "original" and m.calls == 1


@gpu
def test_a_swap_after_accelerate_is_caught_at_the_next_rebuild():
    """accelerate() checked the activations once; every engine build checks them again, so after a swap the next rebuild (here: an
    in-place weight change) sends the call to the reference forward instead of computing the yaml's function for another model."""
    from bs_yolo_amd import plugin
    meta = fixture("yolov6n")[1]
    m = V6Model(_cfg(meta), _sd_of("yolov6n")).to(DEV)
    plugin.accelerate(m)
    x = x_of(meta, 0).half().to(DEV)
    y, _ = m(x)
    st = m._bsy_state
    assert m.calls == 0 and st["engine_calls"] == 1
    m.get_submodule("model.4.1").act = torch.nn.SiLU()
    with torch.no_grad():
        m.model[10].conv.weight.mul_(0.5)
    assert m(x) == "original" and m.calls == 1 and st["fallbacks"] == 1 and st["engine_calls"] == 1 and "fp16" in st["failed"]
    plugin.restore(m)


def test_sppf_form_reads_both_convs():
    from bs_yolo_amd.engine import sppf_form
    meta = fixture("yolov6n")[1]
    cfg, sd = _cfg(meta), _sd_of("yolov6n")
    assert sppf_form(V6Model(cfg, sd, "silu"), cfg) == "silu" and sppf_form(V6Model(cfg, sd, "relu"), cfg) == "relu"
    m = V6Model(cfg, sd, "silu")
    m.model[9].cv1.act = torch.nn.ReLU()
    with pytest.raises(NotImplementedError, match="disagree"):
        sppf_form(m, cfg)
    m.model[9].cv1.act = torch.nn.Hardswish()
    with pytest.raises(NotImplementedError, match=r"model\.9\.cv1: SPPF's activation is Hardswish"):
        sppf_form(m, cfg)
    with pytest.raises(NotImplementedError, match="cannot read SPPF's activations"):
        sppf_form(torch.nn.Module(), cfg)
    assert sppf_form(torch.nn.Module(), stock_cfg("yolov8", "n", NC)) == "silu"  # read under a ReLU graph alone


@gpu
def test_engine_reads_the_sppf_form_off_a_model():
    from bs_yolo_amd.engine import YoloEngine
    meta = fixture("yolov6n_upstream")[1]
    cfg, sd = _cfg(meta), _sd_of("yolov6n_upstream")
    for form in ("relu", "silu"):
        eng = YoloEngine(cfg, V6Model(cfg, sd, form))
        assert eng.sppf_act == form
        eng.close()
    eng = YoloEngine(cfg, sd)  # a bare state dict does not say: "silu"
    assert eng.sppf_act == "silu"
    eng.close()
    eng = YoloEngine(cfg, V6Model(cfg, sd, "silu"), sppf_act="relu")  # the argument wins
    assert eng.sppf_act == "relu"
    eng.close()
