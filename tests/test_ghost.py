"""YOLOv8-ghost graphs on the engine (cfg/models/v8/yolov8-ghost.yaml, -p2, -p6): the graph families, the plan lowering of GhostConv /
GhostBottleneck / C3Ghost in all three precisions, BSY_OP_ADD (bsyolo_ops.hip add_kernel, ref32.hip add32_kernel) and BSY_OP_GHOST
(csrc/ghost_fused.hip) ALONE as one-op plans on poisoned views, the three graphs against fixtures made by running the reference
(tests/golden/make_ghost_fixtures.py), the BSY_FUSE_GHOST switch and plugin.accelerate.

BSY_OP_GHOST cases.  The kernel's output tile is 8 x 16 and its patch 12 x 20, it walks tiles persistently (grid cap 256 x workgroups per
CU, at most 1024) and holds one accumulator per 32 hidden channels.  Maps: 3 x 5 (smaller than the halo), 9 x 21 and 13 x 19 (partial tiles
both ways, a second tile along W / along H).  Widths (Cin, CH): (16, 8), (40, 24) -- Cin off a 32 boundary: a K-step half past Cin --,
(64, 72) -- CH no multiple of 32 --, (320, 160) -- the widest stock GhostConv shapes; cv1's weights no longer fit in LDS beside the patch.
act = 1 without a shortcut and act = 0 with one (the two forms a GhostBottleneck holds).  Source, destination and shortcut are channel
slices at non-zero offsets of wider buffers: the source and the shortcut in NaN, the destination in 777, the weight blob with NaN
between its records.
  (a) act = 0, dyadic payloads (x and the shortcut in eighths, cv1 weights in {-1, 0, 1} and a bias in eighths, cv2 weights in {-1/4, 0,
      1/4} and a bias in 1/32; asserted: every value a multiple of 2^-5 below 64 and every sum of magnitudes below 2^19, so exact in
      f32 in any order and exact in f16): the output is the fp64 result bit for bit.
  (b) random payloads: bit for bit the plain chain CONV 1x1 -> DWCONV_G 5x5 (-> ADD) run as one plan on the same blob and views.
  (c) that chain lies within op_plan_helpers._bound of fp64 stage by stage, every stage's input read back from the GPU (cv1: K = Cin;
      cv2: K = 25; both round f16(act(v)) once), and the ADD stage is exact: f16(a + b) of two f16 values through f32 is the correctly
      rounded sum (24 >= 2 * 11 + 2 bits).
  (d) the poison outside the destination view is intact, the source and shortcut buffers keep their bits.
  (e) one case with 2625 tiles (over 2.5 x the cap of 1024), all inside the map, against the chain.

Graph bounds, the project's (test_p2p6.py): fp16 score < 1e-2, box < max(1, stride / 32) px per level, raw maps 3e-2 of max(1, maximum);
fp32 / fp32x 1e-3 and 1e-3 * imgsz.

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
from bs_yolo_amd.plan import Plan, make_divisible
from bs_yolo_amd.weights import fold_conv_bn, pack_plan_weights, synth_state_dict
from graph_helpers import (RawBounds, RefModel, YBounds, all_equal, cfg_of, check_nms, check_raw, check_y, engine, fixture, kinds, level_of_anchor,
                           outputs, state_dict, x_of)
from op_plan_helpers import (DEV, NAN, POISON16, POISON32, _bound, _worst, assert_poison_intact, bits, conv1x1_op, dw_ref, dwg_op, new_op,
                             packed_1x1, poisoned, poisoned_blob, run_ops, view)

gpu = pytest.mark.gpu
NC = 12
F16, F32, F64 = torch.float16, torch.float32, torch.float64
FAMILIES = ["yolov8-ghost", "yolov8-ghost-p2", "yolov8-ghost-p6"]
STRIDES = {"yolov8-ghost": (8, 16, 32), "yolov8-ghost-p2": (4, 8, 16, 32), "yolov8-ghost-p6": (8, 16, 32, 64)}
SHAPES = {"yolov8-ghost": [(1, 64, 64), (2, 96, 128)], "yolov8-ghost-p2": [(1, 64, 64), (2, 96, 128)],
          "yolov8-ghost-p6": [(1, 64, 64), (2, 128, 192)]}  # the fixtures' shapes; p6 (no fixture) needs multiples of 64
GRAPHS = ["yolov8s_ghost", "yolov8n_ghost_p2", "yolov8x_ghost"]
Y_BOUNDS = YBounds(score16=1e-2, p999_16=None, box16=1.0, score32=1e-3, box32=1e-3)  # the graph bounds of the module docstring
RAW_BOUNDS = RawBounds(rel16=3e-2, strict16=False, floor16=True, rel32=1e-3)


def _damped(name, suffixes):
    return re.search(r"\.m\.\d+\.", name) is not None and any(name.endswith(s) for s in suffixes)


def _damp(name, meta):
    """The rule the generator wrote into meta["damp"] (make_ghost_fixtures.py)."""
    return meta["damp"]["factor"] if _damped(name, meta["damp"]["suffixes"]) else 1.0


def _sd_of(tag):
    return state_dict(tag, _damp)


# ---- host side (no GPU) ------------------------------------------------------------------------------------------------
def test_family_tables():
    want = {"yolov8-ghost": ([15, 18, 21], 10, 13, 4, 2, 8), "yolov8-ghost-p2": ([18, 21, 24, 27], 10, 19, 4, 3, 10),
            "yolov8-ghost-p6": ([20, 23, 26, 29], 12, 19, 5, 3, 11)}
    for fam, (frm, nb, nh, gb, gh, c3) in want.items():
        cfg = stock_cfg(fam, "s", NC)
        layers = cfg["backbone"] + cfg["head"]
        mods = [l[2] for l in layers]
        assert cfg["head"][-1] == [frm, 1, "Detect", ["nc"]] and len(cfg["backbone"]) == nb and len(cfg["head"]) == nh
        assert cfg["scales"] == stock_cfg("yolov8", "s", NC)["scales"] and mods[0] == "Conv" and mods.count("Conv") == 1
        assert [l[2] for l in cfg["backbone"]].count("GhostConv") == gb and [l[2] for l in cfg["head"]].count("GhostConv") == gh
        assert mods.count("C3Ghost") == c3 and "C2f" not in mods and "C2" not in mods and mods.count("SPPF") == 1
        assert all(l[3][1:] == [3, 2] for l in layers if l[2] == "GhostConv")
        assert all(l[3][1:] == [True] for l in cfg["backbone"] if l[2] == "C3Ghost") and all(len(l[3]) == 1 for l in cfg["head"] if l[2] == "C3Ghost")
    for task in ("segment", "obb"):  # fall out of the planner, not required: they must at least describe a graph
        assert stock_cfg("yolov8-ghost", "n", NC, task)["head"][-1][2] in ("Segment", "OBB")
    with pytest.raises(ValueError):
        stock_cfg("yolov8-ghost", "n", 1, "pose", kpt_shape=(17, 3))


@pytest.mark.parametrize("precision", ["fp16", "fp32x", "fp32"])
@pytest.mark.parametrize("scale", list("nsmlx"))
@pytest.mark.parametrize("family", FAMILIES)
def test_ghost_plans(family, scale, precision, monkeypatch):
    monkeypatch.delenv("BSY_FUSE_GHOST", raising=False)
    cfg = stock_cfg(family, scale, NC)
    depth, width, max_ch = cfg["scales"][scale]
    strides = STRIDES[family]
    for b, h, w in [(1, 64, 64)] + SHAPES[family][1:]:
        plan = Plan(cfg, b, h, w, precision=precision)
        m = plan.meta
        assert m["strides"] == [float(s) for s in strides] and m["levels"] == [(h // s, w // s) for s in strides]
        assert m["A"] == sum((h // s) * (w // s) for s in strides) and m["legacy"] and m["nm"] == 0
        nb = sum(max(round(l[1] * depth), 1) for l in cfg["backbone"] + cfg["head"] if l[2] == "C3Ghost")  # GhostBottlenecks
        ghosts, adds = kinds(plan, L.OP_GHOST), kinds(plan, L.OP_ADD)
        assert (len(ghosts), len(adds)) == ((2 * nb, 0) if precision == "fp16" else (0, nb))
        assert not kinds(plan, L.OP_BNECK) and len(kinds(plan, L.OP_SPPF_POOL)) == 1
        for o in ghosts:
            assert o["dst"].C == 2 * o["mid_c"] and not o["src0"].C % 8 and not o["mid_c"] % 8 and o["lane"] == 0
            assert (o["res"] is not None) == o["name"].endswith(".conv.2") and o["act"] == int(o["name"].endswith(".conv.0"))
            assert L.lib.bsy_ghost_fused_supported(o["src0"].C, o["mid_c"]) == 1
            assert plan.wrecs[o["wkey"]].kind == "conv" and plan.wrecs[o["wkey2"]].kind == "dwg" and plan.wrecs[o["wkey2"]].k == 5
        # the stride-2 downsamplers: a 3x3 stride-2 CONV into the first half and a depthwise 5x5 into the second, in every precision
        for l, layer in enumerate(cfg["backbone"] + cfg["head"]):
            if layer[2] == "GhostConv":
                cv1, cv2 = (next(o for o in plan.ops if o["name"] == f"model.{l}.{cv}") for cv in ("cv1", "cv2"))
                c2 = make_divisible(min(layer[3][0], max_ch) * width, 8)
                assert (cv1["kind"], cv1["ksize"], cv1["stride"], cv1["dst"].C, cv1["dst"].coff) == (L.OP_CONV, 3, 2, c2 // 2, 0)
                assert (cv2["kind"], cv2["ksize"], cv2["pad"], cv2["stride"], cv2["act"]) == (L.OP_DWCONV_G, 5, 5, 1, c2 // 2)
                assert cv2["src0"].view() == cv1["dst"].view() and cv2["dst"].buf == cv1["dst"].buf and cv2["dst"].coff == c2 // 2
    pack_plan_weights(plan, synth_state_dict(plan))
    ops = plan.c_ops()
    assert [o.mid_c for o in ops if o.kind == L.OP_GHOST] == [o["mid_c"] for o in ghosts]
    assert all(o.ksize == 5 and o.stride == 1 and o.pad == 2 and o.w2_off > o.w_off for o in ops if o.kind == L.OP_GHOST)


@pytest.mark.parametrize("family", FAMILIES)
def test_conv_flops_at_640(family):
    """Plan.flops (2 x MAC of every conv, the depthwise ones included) at 1 x 640 x 640, nc = 80, within 1 % of the count of the
    reference's own convs (make_ghost_fixtures.py conv_gflops_640, stored in every fixture's meta) -- test_yolov9.py's tolerance.  The
    fp16 plans of n, m and x carry their 4-, 12- and 20-channel pieces on 8, 16 and 24 and multiply 0.1 - 0.3 % more; the fp32 plans
    have no padding.  mfma_flops holds the dense part only, as for DWPW."""
    ref = fixture("yolov8s_ghost")[1]["ref_conv_gflops_640"][family]
    for scale in "nsmlx":
        for precision in ("fp16", "fp32"):
            plan = Plan(stock_cfg(family, scale, 80), 1, 640, 640, precision=precision)
            got = plan.flops / 1e9
            print(family, scale, precision, f"plan {got:.4f} reference convs {ref[scale]:.4f}")
            assert abs(got - ref[scale]) <= 0.01 * ref[scale]
            dw = sum(2 * o["OH"] * o["OW"] * o["src0"].C * 25 for o in kinds(plan, L.OP_DWCONV_G))
            dw += sum(2 * o["OH"] * o["OW"] * o["mid_c"] * 25 for o in kinds(plan, L.OP_GHOST))
            assert sum(o.get("mfma_flops", 0) for o in plan.ops) == plan.flops - dw
        if scale in "sl":
            assert abs(got - ref[scale]) <= 1e-4 * ref[scale]  # no padding anywhere: the same count


def test_fuse_ghost_switch(monkeypatch):
    cfg = stock_cfg("yolov8-ghost", "s", NC)
    monkeypatch.setenv("BSY_FUSE_GHOST", "0")
    off = Plan(cfg, 1, 64, 64)
    assert not off.fuse_ghost and not kinds(off, L.OP_GHOST) and len(kinds(off, L.OP_ADD)) == 10
    for env in (None, "1"):
        monkeypatch.delenv("BSY_FUSE_GHOST", raising=False)
        if env:
            monkeypatch.setenv("BSY_FUSE_GHOST", env)
        on = Plan(cfg, 1, 64, 64)
        assert on.fuse_ghost and len(kinds(on, L.OP_GHOST)) == 20 and not kinds(on, L.OP_ADD)
    assert not Plan(cfg, 1, 64, 64, precision="fp32").fuse_ghost and not Plan(cfg, 1, 64, 64, precision="fp32x").fuse_ghost
    with pytest.raises(TypeError):  # a plan attribute read from the environment like fuse_boxtail, not a keyword of SWITCHES
        Plan(cfg, 1, 64, 64, fuse_ghost=False)
    # every stride-1 GhostConv is ONE op and a bottleneck exactly two, where the unfused plan has five
    names = [o["name"] for o in on.ops]
    bnecks = sorted({n[:-len(".conv.0")] for n in names if n.endswith(".conv.0")})
    assert len(bnecks) == 10
    for bn in bnecks:
        i = names.index(bn + ".conv.0")
        assert names[i + 1] == bn + ".conv.2" and [n for n in names if n.startswith(bn + ".")] == names[i:i + 2]
        a, b = on.ops[i:i + 2]
        assert a["kind"] == b["kind"] == L.OP_GHOST and b["src0"].view() == a["dst"].view() and b["res"].view() == a["src0"].view()
        assert (a["act"], b["act"], 4 * a["mid_c"], 2 * b["mid_c"]) == (1, 0, b["dst"].C, b["dst"].C)
        chain = [o for o in off.ops if o["name"].startswith(bn + ".")]
        assert [o["kind"] for o in chain] == [L.OP_CONV, L.OP_DWCONV_G, L.OP_CONV, L.OP_DWCONV_G, L.OP_ADD]
        assert chain[4]["src0"].buf == chain[2]["dst"].buf == chain[3]["dst"].buf != chain[4]["dst"].buf and chain[4]["src1"].view() == chain[0]["src0"].view()
        assert chain[4]["dst"].view()[1:] == b["dst"].view()[1:] and chain[4]["src0"].C == chain[4]["dst"].C == 2 * b["mid_c"]
    assert len(off.ops) - len(on.ops) == 3 * 10 and off.flops == on.flops and list(off.wrecs) == list(on.wrecs)
    assert [(k, r.kind, r.cout, r.cin, r.k) for k, r in off.wrecs.items()] == [(k, r.kind, r.cout, r.cin, r.k) for k, r in on.wrecs.items()]


def test_what_is_refused():
    from bs_yolo_amd.plugin import graph_support
    # a width multiple of 0.375: C3Ghost(48) has c_ = 24 and a second GhostConv of hidden width 12
    odd = stock_cfg("yolov8-ghost", "s", NC)
    odd["scales"] = {"s": [0.33, 0.375, 1024]}
    with pytest.raises(NotImplementedError, match=r"hidden width of 12 channels"):
        Plan(odd, 1, 64, 64)
    for precision in ("fp32", "fp32x"):
        assert Plan(odd, 1, 64, 64, precision=precision).meta["A"] == 84
    assert graph_support(odd) == {"fp16": False, "fp32": True}
    # GhostBottleneck at top level: s = 1 builds (two GhostConvs, one launch each on fp16), s = 2 is in no shipped graph
    for precision in ("fp16", "fp32x", "fp32"):
        top = stock_cfg("yolov8-ghost", "s", NC)
        top["backbone"][2] = [-1, 1, "GhostBottleneck", [128, 3, 1]]
        plan = Plan(top, 1, 64, 64, precision=precision)
        assert [o["name"] for o in plan.ops if o["name"].startswith("model.2.")][0].startswith("model.2.conv.0")
        assert len([o for o in plan.ops if o["name"].startswith("model.2.")]) == (2 if precision == "fp16" else 5)
        top["backbone"][2] = [-1, 1, "GhostBottleneck", [128, 3, 2]]
        with pytest.raises(NotImplementedError, match="s = 2"):
            Plan(top, 1, 64, 64, precision=precision)
        top["backbone"][2] = [-1, 1, "GhostBottleneck", [256, 3, 1]]  # 64 -> 128 channels under an identity shortcut
        with pytest.raises(NotImplementedError):
            Plan(top, 1, 64, 64, precision=precision)
    for fam in FAMILIES:
        for scale in "nsmlx":
            assert graph_support(stock_cfg(fam, scale, NC)) == {"fp16": True, "fp32": True}


def _unpack16(blob, r, cout, cin):
    cp, kp = C.c_int(), C.c_int()
    L.check(L.lib.bsy_conv_packed_dims(cout, cin, r.k, C.byref(cp), C.byref(kp)))
    w = np.frombuffer(blob, np.float16, cp.value * kp.value, r.w_off).reshape(cp.value, kp.value)
    return w, np.frombuffer(blob, np.float32, cp.value, r.b_off)


@pytest.mark.parametrize("tag", GRAPHS)
def test_weights_pack_from_the_reference_state_dict(tag):
    _, meta = fixture(tag)
    sd = _sd_of(tag)
    assert meta["damp"]["factor"] == {"yolov8s_ghost": 0.5, "yolov8n_ghost_p2": 0.5, "yolov8x_ghost": 0.25}[tag]
    assert sum(_damped(n, meta["damp"]["suffixes"]) for n in sd) == 2 * sum(n.endswith(".conv.2.cv1.bn.weight") for n in sd) > 0
    seen = set()

    class Recording(dict):
        def __getitem__(self, k):
            seen.add(k)
            return dict.__getitem__(self, k)

    for precision in ("fp16", "fp32x"):
        plan = Plan(cfg_of(meta), 1, 64, 64, precision=precision)
        blob = pack_plan_weights(plan, Recording(sd))
        assert set(synth_state_dict(plan)) == {n for n in sd if not n.endswith(".dfl.conv.weight") and not n.endswith("num_batches_tracked")}
        if precision != "fp16":
            assert all(r.rows is None and r.cols is None for r in plan.wrecs.values())
            continue
        padded = 0
        for key, r in plan.wrecs.items():
            if ".m." not in key or r.kind not in ("conv", "dwg"):
                continue
            w, b = fold_conv_bn(sd, r.name)
            rows = r.rows if r.rows is not None else list(range(r.cout))
            real = [i for i, v in enumerate(rows) if v >= 0]
            assert [rows[i] for i in real] == list(range(w.shape[0])), key  # the module's output channels, in order, padding between
            if r.kind == "dwg":
                gw = np.frombuffer(blob, np.float32, 25 * r.cout, r.w_off).reshape(25, r.cout)
                gb = np.frombuffer(blob, np.float32, r.cout, r.b_off)
                assert np.array_equal(gw[:, real], w.reshape(w.shape[0], 25).t().numpy()) and np.array_equal(gb[real], b.numpy()), key
            else:
                gw, gb = _unpack16(blob, r, r.cout, r.cin)
                cols = r.cols if r.cols is not None else list(range(r.cin))
                creal = [j for j, v in enumerate(cols) if v >= 0]
                assert [cols[j] for j in creal] == list(range(w.shape[1])), key
                assert np.array_equal(gw[np.ix_(real, creal)], w[:, :, 0, 0].to(F16).numpy()) and np.array_equal(gb[real], b.numpy()), key
                zc = np.ones(gw.shape[1], bool)
                zc[creal] = False
                assert not gw[:, zc].any(), key  # zero columns: the padding channels it reads and the tail up to Kpad
            zr = np.ones(gw.shape[-2 if r.kind == "conv" else -1], bool)
            zr[real] = False
            assert not (gw[zr] if r.kind == "conv" else gw[:, zr]).any() and not gb[zr[:len(gb)]].any(), key
            padded += r.rows is not None or r.cols is not None
        assert (padded > 0) == (tag != "yolov8s_ghost")
        if tag == "yolov8n_ghost_p2":  # C3Ghost(32): c_ = 16, the first GhostConv's halves are 4 channels on 8
            a, d, c = (plan.wrecs[f"model.2.m.0.conv.{k}"] for k in ("0.cv1", "0.cv2", "2.cv1"))
            assert a.rows == d.rows == [0, 1, 2, 3, -1, -1, -1, -1] and a.cols == list(range(16)) and (a.cout, a.cin, d.cout) == (8, 16, 8)
            assert c.cols == [0, 1, 2, 3, -1, -1, -1, -1, 4, 5, 6, 7, -1, -1, -1, -1] and c.rows == list(range(8)) and (c.cout, c.cin) == (8, 16)
        if tag == "yolov8x_ghost":  # C3Ghost(160): c_ = 80, halves of 20 channels on 24; C3Ghost(640): GhostConvs of 320 -> 80 and 160 -> 160
            a = plan.wrecs["model.2.m.0.conv.0.cv1"]
            assert a.rows == list(range(20)) + [-1] * 4 and (a.cout, a.cin) == (24, 80)
            shapes = {(o["src0"].C, o["mid_c"]) for o in kinds(plan, L.OP_GHOST)}
            assert {(320, 80), (160, 160), (80, 24), (48, 40)} <= shapes
    assert {n for n in sd if n not in seen and not n.endswith("num_batches_tracked")} == {n for n in sd if n.endswith(".dfl.conv.weight")}
    gone = dict(sd)
    del gone[next(n for n in sd if _damped(n, meta["damp"]["suffixes"]))]
    with pytest.raises(KeyError):
        pack_plan_weights(Plan(cfg_of(meta), 1, 64, 64), gone)


def test_abi():
    header = (ROOT / "include" / "bsyolo.h").read_text()
    assert re.search(r"BSY_OP_GHOST\s*=\s*24\b", header) and re.search(r"BSY_OP_ADD\s*=\s*25\b", header)
    assert re.search(r"int\s+bsy_ghost_fused_supported\s*\(", header)
    assert (L.OP_GHOST, L.OP_ADD, L.OP_CLASSIFY_TAIL) == (24, 25, 23) and "bsy_ghost_fused_supported" in L.SYMBOLS
    assert L.lib.bsy_sizeof_op() == C.sizeof(L.Op) == 624
    assert re.search(r'PLAN_ENV = .*"BSY_FUSE_GHOST"', (ROOT / "tools" / "plan_snapshot.py").read_text())  # the snapshots unset it too
    from bs_yolo_amd.plan import LANE_KINDS, SWITCHES
    assert "fuse_ghost" not in SWITCHES and L.OP_GHOST not in LANE_KINDS


def test_ghost_fused_supported_widths():
    f = L.lib.bsy_ghost_fused_supported
    assert all(f(cin, ch) == 1 for cin in range(8, 321, 8) for ch in range(8, 161, 8))
    assert not any(f(cin, ch) for cin, ch in ((0, 8), (8, 0), (12, 8), (8, 12), (-8, 8), (8, -8), (4, 4), (1 << 20, 8), (8, 1 << 20)))


# ------------------------------------------------------------------------------------------------------------
# BSY_OP_ADD alone
# ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("alias", [False, True], ids=["sep", "alias"])
@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_add_op(dtype, Cc, alias):
    B, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(Cc * 10 + alias)
    a = (torch.randn(B, H, W, Cc, generator=g) * 4).to(dtype)
    b = (torch.randn(B, H, W, Cc, generator=g) * torch.tensor([1e-3, 1.0, 30.0, 1.0])[torch.arange(Cc) % 4]).to(dtype)  # far-apart exponents too
    a[0, 0, 0, 0], b[0, 0, 0, 0] = 60000.0, 60000.0  # f16: the sum overflows to inf, as the reference's add does
    want = (a.float() + b.float()).to(dtype)
    assert torch.equal(bits(want), bits((a.double() + b.double()).to(dtype)))  # one rounding: the correctly rounded sum
    poison = POISON16 if dtype == F16 else POISON32
    lda, ca, ldb, cb, ldd, cd = Cc + 24, 8, Cc + 8, 0, Cc + 40, 16
    ta, tb = poisoned((B, H, W, lda), ca, Cc, a, poison), poisoned((B, H, W, ldb), cb, Cc, b, poison)
    op = new_op(L.OP_ADD, 0 if dtype == F16 else 1, B, H, W)
    op.src0, op.src1 = view(0, lda, ca, Cc), view(1, ldb, cb, Cc)
    if alias:
        op.dst, td, ldd, cd = view(0, lda, ca, Cc), ta, lda, ca
    else:
        td = poisoned((B, H, W, ldd), cd, Cc, None, poison, dtype=dtype)
        op.dst = view(2, ldd, cd, Cc)
    before_b, before_a = tb.cpu(), ta.cpu()
    run_ops([op], [ta, tb, None if alias else td])
    assert_poison_intact(td, cd, Cc, poison)
    assert torch.equal(bits(td[..., cd:cd + Cc]), bits(want))
    assert torch.equal(bits(tb), bits(before_b)) and (alias or torch.equal(bits(ta), bits(before_a)))


# ------------------------------------------------------------------------------------------------------------
# BSY_OP_GHOST alone
# ------------------------------------------------------------------------------------------------------------
MAPS = [(3, 5), (9, 21), (13, 19)]
WIDTHS = [(16, 8), (40, 24), (64, 72), (320, 160)]
FORMS = [("act", 1, False), ("res", 0, True)]
GHOST_CASES = [(h, w, cin, ch, act, res) for h, w in MAPS for cin, ch in WIDTHS for _, act, res in FORMS]
GHOST_IDS = ["%dx%d-%d-%d-%s" % (h, w, cin, ch, "res" if res else "act") for h, w, cin, ch, act, res in GHOST_CASES]
TILE, GRID_CAP = (8, 16), 1024
WALK = (3, 200, 560, 16, 8)  # 3 x 25 x 35 = 2625 tiles, all inside the map, no multiple of 8


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 15485863 * int(k) for i, k in enumerate(key)) % (2 ** 31))


@lru_cache(maxsize=None)
def _ghost_payload(B, H, W, cin, ch, exact):
    """x (B, H, W, cin) and res (B, H, W, 2 ch), f16-representable; cv1 (w (ch, cin), b), f16-representable weights; cv2 (w (25, ch), b) f32."""
    g = _gen(B, H, W, cin, ch, exact)
    if not exact:
        h = lambda t: t.to(F16).to(F32)  # noqa: E731
        return SimpleNamespace(x=h(torch.randn(B, H, W, cin, generator=g)), res=h(torch.randn(B, H, W, 2 * ch, generator=g)),
                               w1=h(torch.randn(ch, cin, generator=g) * (2.0 / cin) ** 0.5), b1=torch.randn(ch, generator=g) * 0.2,
                               w2=torch.randn(25, ch, generator=g) * (2.0 / 25) ** 0.5, b2=torch.randn(ch, generator=g) * 0.2)
    draw = lambda shp, lim: torch.randint(-lim, lim + 1, shp, generator=g).float()  # noqa: E731
    x = draw((B, H, W, cin), 3) / 8
    x[:, [0, -1]] = torch.where(x[:, [0, -1]] == 0, torch.tensor(0.375), x[:, [0, -1]])  # no tap hides behind a zero edge
    x[:, :, [0, -1]] = torch.where(x[:, :, [0, -1]] == 0, torch.tensor(0.375), x[:, :, [0, -1]])
    w1 = draw((ch, cin), 1) * (torch.rand(ch, cin, generator=g) < min(1.0, 16.0 / cin)).float()
    w2 = (2 * torch.randint(0, 2, (25, ch), generator=g).float() - 1) * (torch.rand(25, ch, generator=g) < 0.6).float() / 4
    return SimpleNamespace(x=x, res=draw((B, H, W, 2 * ch), 24) / 8, w1=w1, b1=draw((ch,), 8) / 8, w2=w2, b2=draw((ch,), 16) / 32)


def _ghost_stages(x, p, act):
    """fp64 stages of the chain from the values the kernels read: cv1 on `x` (B, H, W, cin) -> stage with v, a, ref, S, K."""
    w1 = p.w1.to(F64)
    v = x.to(F64) @ w1.t() + p.b1.to(F64)
    a = F.silu(v) if act else v
    S = x.to(F64).abs() @ w1.abs().t() + p.b1.to(F64).abs()
    return SimpleNamespace(v=v, a=a, ref=a, S=S, act=act, res=None, K=w1.shape[1], nsl=1, out_f32=False)


def _dw_stage(y, p, act):
    v = dw_ref(y, p.w2, p.b2, False, None, 5, 5)
    a = F.silu(v) if act else v
    S = dw_ref(y.abs(), p.w2.abs(), p.b2.abs(), False, None, 5, 5)
    return SimpleNamespace(v=v, a=a, ref=a, S=S, act=act, res=None, K=25, nsl=1, out_f32=False)


def _dyadic(v, step, lim):
    return bool((v / step == (v / step).round()).all()) and float(v.abs().max()) < lim


def _exact_ref(p):
    """The one right answer of a dyadic payload with act = 0 and a shortcut: [y | z] + res in fp64 (asserted exact in f32 and f16)."""
    s1 = _ghost_stages(p.x, p, 0)
    s2 = _dw_stage(s1.ref, p, 0)
    out = torch.cat([s1.ref, s2.ref], -1) + p.res.to(F64)
    assert _dyadic(p.x, 1 / 8, 64) and _dyadic(p.res, 1 / 8, 4)
    for s in (s1, s2):
        assert _dyadic(s.v, 1 / 32, 32) and float(s.S.max()) * 32 < 2 ** 24
    assert _dyadic(out, 1 / 32, 64) and float(s1.v.abs().max()) > 1 and float(s2.v.abs().max()) > 1
    return out + 0.0  # (no -0: the sums start at a +0 or non-zero bias)


def _ghost_run(B, H, W, cin, ch, act, res, p, chain):
    """The GHOST op, or the chain it stands for as ONE plan: CONV 1x1 -> DWCONV_G 5x5 into the halves of the destination (with a
    shortcut: of a scratch buffer, slot 3, then ADD).  -> (destination view, the chain's [y | z] before the shortcut or None)."""
    lds, cs, ldd, cd, ldr, cr, ldp, cp = cin + 16, 8, 2 * ch + 40, 16, 2 * ch + 24, 8, 2 * ch + 16, 8
    src = poisoned((B, H, W, lds), cs, cin, p.x.to(F16), NAN)
    dst = poisoned((B, H, W, ldd), cd, 2 * ch, None, POISON16, dtype=F16)
    rsb = poisoned((B, H, W, ldr), cr, 2 * ch, p.res.to(F16), NAN) if res else None
    w1p, b1p = packed_1x1(p.w1, p.b1)
    blob, (ow1, ob1, ow2, ob2) = poisoned_blob([w1p, b1p, p.w2.numpy(), p.b2.numpy()])
    sv, dv, rv = view(0, lds, cs, cin), view(1, ldd, cd, 2 * ch), view(2, ldr, cr, 2 * ch)
    pair = None
    if not chain:
        op = new_op(L.OP_GHOST, 0, B, H, W)
        op.src0, op.dst, op.ksize, op.stride, op.pad, op.act, op.mid_c, op.dst_scale = sv, dv, 5, 1, 2, act, ch, 1
        op.w_off, op.b_off, op.w2_off, op.b2_off = ow1, ob1, ow2, ob2
        if res:
            op.res = rv
        ops, ext = [op], [src, dst, rsb]
    else:
        if res:
            pair = poisoned((B, H, W, ldp), cp, 2 * ch, None, POISON16, dtype=F16)
            y, z = view(3, ldp, cp, ch), view(3, ldp, cp + ch, ch)
        else:
            y, z = view(1, ldd, cd, ch), view(1, ldd, cd + ch, ch)
        ops = [conv1x1_op(B, H, W, sv, y, ow1, ob1, act=act), dwg_op(0, B, H, W, 5, 5, 1, y, z, ow2, ob2, ch, 0, ch if act else 0)]
        if res:
            add = new_op(L.OP_ADD, 0, B, H, W)
            add.src0, add.src1, add.dst = view(3, ldp, cp, 2 * ch), rv, dv
            ops.append(add)
        ext = [src, dst, rsb, pair]
    sb, rb = src.cpu(), rsb.cpu() if res else None
    run_ops(ops, ext, blob)
    assert_poison_intact(dst, cd, 2 * ch, POISON16)
    assert torch.equal(bits(src), bits(sb)) and (not res or torch.equal(bits(rsb), bits(rb))), "a store reached a source buffer"
    if pair is not None:
        assert_poison_intact(pair, cp, 2 * ch, POISON16)
        pair = pair[..., cp:cp + 2 * ch].cpu()
    return dst[..., cd:cd + 2 * ch].cpu(), pair


def test_ghost_payloads_are_exact_and_cases_reach_every_edge():
    th, tw = TILE
    assert any(h < 5 and w <= 5 for h, w in MAPS) and any(h > th and h % th for h, w in MAPS) and any(w > tw and w % tw for h, w in MAPS)
    assert all(h % th and w % tw for h, w in MAPS)
    assert any(ch % 32 for _, ch in WIDTHS) and any(cin % 32 and cin % 16 for cin, _ in WIDTHS) and (320, 160) in WIDTHS
    for h, w in MAPS:
        for cin, ch in WIDTHS:
            _exact_ref(_ghost_payload(2, h, w, cin, ch, True))
    B, H, W, _, _ = WALK
    assert H % th == 0 and W % tw == 0 and B * (H // th) * (W // tw) > 2.5 * GRID_CAP and (B * (H // th) * (W // tw)) % 8


@gpu
@pytest.mark.parametrize("case", GHOST_CASES, ids=GHOST_IDS)
def test_ghost_op(case):
    H, W, cin, ch, act, res = case
    B = 2
    assert L.lib.bsy_ghost_fused_supported(cin, ch) == 1
    if not act:  # (a) the one right answer of a dyadic payload
        p = _ghost_payload(B, H, W, cin, ch, True)
        got, _ = _ghost_run(B, H, W, cin, ch, 0, res, p, chain=False)
        want = _exact_ref(p).to(F16)
        d = (got.double() - want.double()).abs()
        print("exact", GHOST_IDS[GHOST_CASES.index(case)], f"differing {int((bits(got) != bits(want)).sum())} of {got.numel()}, max {float(d.max()):.3e}")
        assert torch.equal(bits(got), bits(want))
    p = _ghost_payload(B, H, W, cin, ch, False)
    fused, _ = _ghost_run(B, H, W, cin, ch, act, res, p, chain=False)
    chain, pair = _ghost_run(B, H, W, cin, ch, act, res, p, chain=True)
    nd = int((bits(fused) != bits(chain)).sum())
    print("chain", GHOST_IDS[GHOST_CASES.index(case)], f"differing {nd} of {fused.numel()}, y half {int((bits(fused[..., :ch]) != bits(chain[..., :ch])).sum())}")
    yz = pair if res else chain  # the chain's [y | z] before the shortcut
    s1 = _ghost_stages(p.x, p, act)
    s2 = _dw_stage(yz[..., :ch], p, act)  # from the y the GPU wrote
    w1 = _worst(yz[..., :ch], s1.ref, sum(_bound(s1, s1, False)))
    w2 = _worst(yz[..., ch:], s2.ref, sum(_bound(s2, s2, False)))
    print("bound", f"cv1 {w1:.3f} cv2 {w2:.3f} of 1")
    assert nd == 0  # (b)
    assert w1 <= 1.0 and w2 <= 1.0  # (c)
    if res:
        assert torch.equal(bits(chain), bits((yz.double() + p.res.double()).to(F16)))  # the ADD stage: the correctly rounded sum


@gpu
def test_ghost_op_walks_more_tiles_than_its_grid():
    B, H, W, cin, ch = WALK
    p = _ghost_payload(B, H, W, cin, ch, False)
    for act, res in ((1, False), (0, True)):
        fused, _ = _ghost_run(B, H, W, cin, ch, act, res, p, chain=False)
        chain, _ = _ghost_run(B, H, W, cin, ch, act, res, p, chain=True)
        assert bool(torch.isfinite(fused.float()).all())
        nd = int((bits(fused) != bits(chain)).sum())
        print("walk", act, res, f"differing {nd} of {fused.numel()}")
        assert nd == 0


@gpu
@pytest.mark.parametrize("cin,ch", [(16, 200), (520, 8)])
def test_ghost_op_refuses_what_is_not_supported(cin, ch):
    assert L.lib.bsy_ghost_fused_supported(cin, ch) == 0
    p = _ghost_payload(1, 3, 5, cin, ch, False)
    with pytest.raises(L.BsyError, match="ghost_fused"):
        _ghost_run(1, 3, 5, cin, ch, 1, False, p, chain=False)
    # (the destination's poison: _ghost_run checks it only after a run; build the op again on a destination of this test's own)
    dst = poisoned((1, 3, 5, 2 * ch + 8), 8, 2 * ch, None, POISON16, dtype=F16)
    src = poisoned((1, 3, 5, cin), 0, cin, p.x.to(F16), NAN)
    w1p, b1p = packed_1x1(p.w1, p.b1)
    blob, (ow1, ob1, ow2, ob2) = poisoned_blob([w1p, b1p, p.w2.numpy(), p.b2.numpy()])
    op = new_op(L.OP_GHOST, 0, 1, 3, 5)
    op.src0, op.dst, op.ksize, op.stride, op.pad, op.act, op.mid_c = view(0, cin, 0, cin), view(1, 2 * ch + 8, 8, 2 * ch), 5, 1, 2, 1, ch
    op.w_off, op.b_off, op.w2_off, op.b2_off = ow1, ob1, ow2, ob2
    with pytest.raises(L.BsyError):
        run_ops([op], [src, dst], blob)
    torch.cuda.synchronize()
    assert bool((dst.cpu() == POISON16).all())  # nothing was launched
    op.prec = 1
    with pytest.raises(L.BsyError, match="fp32"):  # no fp32 form: the planner never emits it there
        run_ops([op], [src, dst], blob)


# ------------------------------------------------------------------------------------------------------------
# the graphs
# ------------------------------------------------------------------------------------------------------------
def _engine(tag, precision, **kw):
    return engine(tag, precision, _damp, **kw)


@gpu
@pytest.mark.parametrize("precision", ["fp16", "fp32x", "fp32"])
@pytest.mark.parametrize("tag", GRAPHS)
def test_ghost_graph_matches_reference(tag, precision, monkeypatch):
    """y, the raw maps of every level and NMS at the fixture's conf, as test_yolov9.py compares them: on the fixture's own y the device
    NMS returns the fixture's rows; on the engine's y it is the oracle's NMS of that y bit for bit; in the fp32-storage modes the rows
    it keeps are the fixture's within the modes' bounds."""
    monkeypatch.delenv("BSY_FUSE_GHOST", raising=False)
    z, meta = fixture(tag)
    eng = _engine(tag, precision)
    kept = 0
    for si, (b, h, w) in enumerate(meta["shapes"]):
        x = x_of(meta, si)
        y, raws = eng((x.half() if precision == "fp16" else x).to(DEV))
        torch.cuda.synchronize()
        plan = eng.plan_for(b, h, w, *(2 * [F16 if precision == "fp16" else F32]))[0]
        assert bool(kinds(plan, L.OP_GHOST)) == (precision == "fp16") and bool(kinds(plan, L.OP_ADD)) == (precision != "fp16")
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
@pytest.mark.parametrize("tag", ["yolov8s_ghost", "yolov8n_ghost_p2"])
def test_fusion_is_not_a_different_answer(tag, monkeypatch):
    """BSY_FUSE_GHOST = 0 and = 1 on the fp16 path: y and the raw maps are the same bits (torch.equal)."""
    _, meta = fixture(tag)
    outs = {}
    for env in ("0", "1"):
        monkeypatch.setenv("BSY_FUSE_GHOST", env)
        eng = _engine(tag, "fp16")
        outs[env] = outputs(eng, meta, F16)
        for b, h, w in meta["shapes"]:
            plan = eng.plan_for(b, h, w, F16, F16)[0]
            assert bool(kinds(plan, L.OP_GHOST)) == (env == "1") and bool(kinds(plan, L.OP_ADD)) == (env == "0")
        eng.close()
    assert all_equal(outs["0"], outs["1"], tag), tag


@gpu
def test_accelerate_a_ghost_model(monkeypatch):
    from bs_yolo_amd import plugin
    monkeypatch.delenv("BSY_FUSE_GHOST", raising=False)
    tag = "yolov8n_ghost_p2"
    z, meta = fixture(tag)
    m = RefModel(cfg_of(meta), _sd_of(tag)).to(DEV)
    plugin.accelerate(m)
    x = x_of(meta, 1)
    b, h, w = meta["shapes"][1]
    lvl = level_of_anchor([(h // int(s), w // int(s)) for s in meta["stride"]])
    y, raws = m(x.to(DEV))  # fp32 input: the fp32x engine
    st = m._bsy_state
    assert m.calls == 0 and len(raws) == 4 and st["fp32_calls"] == 1 and st["support"] == {"fp16": True, "fp32": True}
    check_y(y.cpu().numpy(), z["y1"], meta["stride"], lvl, max(h, w), "fp32x", f"accelerate {tag}", NC, Y_BOUNDS)
    y16, raws16 = m(x.half().to(DEV))  # fp16 input: the product path, which is the engine's own output
    assert st["engine_calls"] == 1 and m.calls == 0
    eng = _engine(tag, "fp16")
    ye, re_ = eng(x.half().to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(y16, ye) and all(torch.equal(a, c) for a, c in zip(raws16, re_))
    assert kinds(st["engine"].plan_for(b, h, w, F16, F16)[0], L.OP_GHOST)
    check_y(y16.float().cpu().numpy(), z["y1"], meta["stride"], lvl, max(h, w), "fp16", f"accelerate {tag}", NC, Y_BOUNDS)
    for l, r in enumerate(raws16):
        check_raw(r.float().cpu().numpy(), z[f"raw1_{l}"], "fp16", f"accelerate {tag} raw {l}", RAW_BOUNDS)
    eng.close()
    plugin.restore(m)
