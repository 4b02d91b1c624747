"""Pose models on the engine, whole graph: the pose tables of graphs.stock_cfg, the Pose head in the plan, the keypoint mode of the
decode launch (csrc/detect.hip, DEC_KPT) alone and inside the graphs, the engine's (y, (raws, kpt)) output and plugin.accelerate --
against fixtures made by running the reference (tests/golden/make_pose_graph_fixtures.py)."""
import ctypes

import numpy as np
import pytest
import torch

from bs_yolo_amd import lib as L
from bs_yolo_amd.graphs import stock_cfg
from bs_yolo_amd.plan import Plan
from bs_yolo_amd.weights import pack_plan_weights, synth_state_dict
from graph_helpers import fixture, state_dict, x_of
from op_plan_helpers import NAN, POISON16, POISON32, bits, new_op, poisoned, run_op, view
from oracle import postproc_ref as PP

DEV = "cuda:0"
GRAPHS = ["yolo11n_pose", "yolov8n_pose", "yolo11n_pose_k5", "yolo11m_pose", "yolov8n_pose_p6"]
PRECISIONS = ["fp16", "fp32x", "fp32"]
# Plan(stock_cfg("yolo11", "s"), 1, 64, 64) on the commit before the pose plan: 71 ops of these kinds (the fp16 path, every switch
# at its default).  The Detect graphs must not have moved.
YOLO11S_KINDS = [8, 18, 1, 1, 9, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3, 1, 1, 1, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1, 9, 1, 1, 1, 1, 1, 1,
                 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 16, 16, 1, 1, 1, 16, 16, 1, 1, 1, 2, 1, 16, 1]


def _cfg(meta):
    return stock_cfg(meta["family"], meta["scale"], meta["nc"], "pose", kpt_shape=tuple(meta["kpt_shape"]))


def _sd(tag):
    """A copy of the reference's un-fused state dict (no damping rule), for the callers that add or drop keys."""
    return dict(state_dict(tag, None))


# ---- host side (no GPU) ------------------------------------------------------------------------------------------------
def _parsed(layers):
    """A yaml layer list as parse_model reads it: yaml.safe_load leaves nn.Upsample's first argument as the STRING 'None', which
    parse_model evaluates (tasks.py:981-985); stock_cfg holds the value."""
    return [[f, n, m, [None if a == "None" else a for a in args]] for f, n, m, args in layers]


@pytest.mark.parametrize("tag", GRAPHS)
def test_stock_cfg_restates_the_pose_yaml(tag):
    _, meta = fixture(tag)
    cfg, want = _cfg(meta), meta["yaml"]  # yaml.safe_load of the reference's file, recorded by make_pose_graph_fixtures.py
    assert cfg["scales"] == want["scales"] and cfg["backbone"] == _parsed(want["backbone"]) and cfg["head"] == _parsed(want["head"])
    assert cfg["head"][-1][2:] == ["Pose", ["nc", "kpt_shape"]] and want["kpt_shape"] == [17, 3]
    assert cfg["kpt_shape"] == meta["kpt_shape"] and cfg["nc"] == meta["nc"] and cfg["scale"] == meta["scale"]
    with pytest.raises(ValueError, match="kpt_shape"):  # no default: the four-argument call keeps raising, as on every commit before
        stock_cfg(meta["family"], meta["scale"], meta["nc"], "pose")


def test_stock_cfg_pose_families_and_other_tasks():
    for fam in ("bsyolo11", "yolov5", "yolov8-p2", "yolov5-p6", "yolov9"):
        with pytest.raises(ValueError):
            stock_cfg(fam, "n" if fam != "yolov9" else "t", 1, "pose", kpt_shape=(17, 3))
    for task in ("detect", "segment", "obb", "classify"):  # the other tasks carry no kpt_shape, whatever the argument says
        assert "kpt_shape" not in stock_cfg("yolo11", "n", 80, task) and "kpt_shape" not in stock_cfg("yolo11", "n", 80, task, kpt_shape=(5, 2))
    assert stock_cfg("yolov8-p6", "s", 2, "pose", (4, 2))["kpt_shape"] == [4, 2]


def _cv4(plan, i, j):
    return next(w for k, w in plan.wrecs.items() if k.endswith(f".cv4.{i}.{j}"))


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_pose_plan_has_the_padded_keypoint_branch_and_one_decode_launch(precision):
    plan = Plan(stock_cfg("yolo11", "n", 1, "pose", kpt_shape=(17, 3)), 1, 64, 64, precision=precision)
    dec = [o for o in plan.ops if o["kind"] == L.OP_DECODE]
    assert len(dec) == 1 and dec[0]["nk"] == 51 and dec[0]["kdim"] == 3 and dec[0]["nm"] == 0 and dec[0]["ne"] == 0
    assert dec[0]["dst"].C == 4 + 1 + 51 and dec[0]["res"].buf == L.BSY_EXT_BASE + Plan.EXT_KPT == L.BSY_EXT_BASE + 5
    assert len(dec[0]["msk"]) == 3 and all(t.ld % 4 == 0 and t.C == 56 and t.f32 for t in dec[0]["msk"])
    assert not any(o.get("out_f32", 0) >= 2 for o in plan.ops)  # no fused-decoder epilogue: the keypoint rows need the launch
    for i in range(3):  # c4 = max(64 // 4, 51) = 51: the branch runs 56 wide, zero weights and biases in the padding
        a, b, c = (_cv4(plan, i, j) for j in range(3))
        assert (a.cout, a.real_cout, a.real_cin) == (56, 51, 0) and (b.cout, b.real_cout, b.cin, b.real_cin) == (56, 51, 56, 51)
        assert (c.cout, c.real_cout, c.cin, c.real_cin, c.kind) == (56, 51, 56, 51, "plain")
    m = plan.meta
    assert m["task"] == "pose" and m["nk"] == 51 and tuple(m["kpt_shape"]) == (17, 3) and m["no"] == 65 and m["nc"] == 1
    assert m["nm"] == 0 and m["ne"] == 0 and m["A"] == 84 and m["levels"] == [(8, 8), (4, 4), (2, 2)]
    pack_plan_weights(plan, synth_state_dict(plan))
    assert [(o.nk, o.kdim, o.nm, o.ne) for o in plan.c_ops() if o.kind == L.OP_DECODE] == [(51, 3, 0, 0)]
    assert all((o.nk, o.kdim) == (0, 0) for o in plan.c_ops() if o.kind != L.OP_DECODE)


def test_pose_plan_widths_keypoint_shapes_and_levels():
    m = Plan(stock_cfg("yolo11", "m", 1, "pose", kpt_shape=(17, 3)), 1, 64, 64)  # ch0 = 256: c4 = 64, no padding
    for i in range(3):
        a, b, c = (_cv4(m, i, j) for j in range(3))
        assert (a.cout, a.real_cout, b.cout, b.real_cout, b.real_cin, c.cin, c.real_cin) == (64, 0, 64, 0, 0, 64, 0)
        assert (c.cout, c.real_cout) == (56, 51)
    k5 = Plan(stock_cfg("yolo11", "n", 3, "pose", kpt_shape=(5, 2)), 1, 64, 64)
    dec = next(o for o in k5.ops if o["kind"] == L.OP_DECODE)
    assert (dec["nk"], dec["kdim"], dec["dst"].C, k5.meta["nk"]) == (10, 2, 4 + 3 + 10, 10) and all(t.C == 16 for t in dec["msk"])
    assert (_cv4(k5, 0, 0).cout, _cv4(k5, 0, 2).cout, _cv4(k5, 0, 2).real_cout) == (16, 16, 10)  # c4 = max(16, 10)
    k8 = Plan(stock_cfg("yolo11", "n", 1, "pose", kpt_shape=(8, 2)), 1, 64, 64)  # nk = 16: the map is exactly as wide
    assert (_cv4(k8, 0, 2).cout, _cv4(k8, 0, 2).real_cout) == (16, 0)
    p6 = Plan(stock_cfg("yolov8-p6", "n", 1, "pose", kpt_shape=(17, 3)), 1, 64, 64)
    dec = next(o for o in p6.ops if o["kind"] == L.OP_DECODE)
    assert dec["nl"] == 4 and len(dec["msk"]) == 4 and p6.meta["levels"] == [(8, 8), (4, 4), (2, 2), (1, 1)] and p6.meta["strides"][-1] == 64.0
    live = stock_cfg("yolo11", "n", 1, "pose", kpt_shape=(17, 3))  # a live model's line: parse_model appends the channel list
    live["head"][-1] = [[16, 19, 22], 1, "Pose", ["nc", "kpt_shape", [64, 128, 256]]]
    assert Plan(live, 1, 64, 64).meta["nk"] == 51


def test_other_plans_carry_no_keypoints_and_detect_has_not_moved():
    for cfg in (stock_cfg("yolo11", "n"), stock_cfg("yolo11", "n", task="segment"), stock_cfg("yolo11", "n", 15, "obb"),
                stock_cfg("yolo11", "n", 10, "classify")):
        plan = Plan(cfg, 1, 64, 64)
        assert plan.meta.get("nk", 0) == 0 and all(o.get("nk", 0) == 0 and o.get("kdim", 0) == 0 for o in plan.ops)
        pack_plan_weights(plan, synth_state_dict(plan))
        assert all(o.nk == 0 and o.kdim == 0 for o in plan.c_ops())
    fuse = dict(fuse_stem=True, fuse_bneck=True, fuse_head=True, fuse_dwpw=True, merge_c3k=True, fuse_msca=True, fuse_tail=True, fuse_pmsfa=True,
                fuse_attn_pe=True)
    plan = Plan(stock_cfg("yolo11", "s"), 1, 64, 64, **fuse)
    pack_plan_weights(plan, synth_state_dict(plan))
    assert len(plan.c_ops()) == len(YOLO11S_KINDS) == 71 and [o["kind"] for o in plan.ops] == YOLO11S_KINDS


def test_pose_plan_refusals():
    for bad in ((17, 4), (65, 3), (0, 3), (17, 1)):
        with pytest.raises(NotImplementedError):
            Plan(stock_cfg("yolo11", "n", 1, "pose", kpt_shape=bad), 1, 64, 64)
    cfg = stock_cfg("yolo11", "n", 1, "pose", kpt_shape=(17, 3))
    cfg["head"][-1] = [[16, 19, 22], 1, "Pose", ["nc", [17, 3]]]  # the pair spelt out in the head line: not the yaml's form, stays on the reference
    with pytest.raises(NotImplementedError):
        Plan(cfg, 1, 64, 64)
    cfg = stock_cfg("yolo11", "n", 1, "pose", kpt_shape=(17, 3))
    del cfg["kpt_shape"]  # the head names a key the description does not have
    with pytest.raises(NotImplementedError):
        Plan(cfg, 1, 64, 64)
    Plan(stock_cfg("yolo11", "n", 1, "pose", kpt_shape=(64, 3)), 1, 64, 64)  # the largest head the kernels take


@pytest.mark.parametrize("tag", GRAPHS)
def test_pose_weights_pack_from_the_reference_state_dict(tag):
    _, meta = fixture(tag)
    sd = _sd(tag)
    seen = set()

    class Recording(dict):
        def __getitem__(self, k):
            seen.add(k)
            return dict.__getitem__(self, k)

    for precision in ("fp16", "fp32x"):
        plan = Plan(_cfg(meta), 1, 64, 64, precision=precision)
        pack_plan_weights(plan, Recording(sd), meta["bn_eps"])  # a missing key raises KeyError
    cv4 = {n for n in sd if ".cv4." in n}
    assert len(cv4) == len(meta["stride"]) * (2 * 5 + 2) and cv4 <= seen
    assert {n for n in sd if not n.endswith("dfl.conv.weight")} <= seen  # every parameter of the model is read


def test_op_record_size_and_field_offsets():
    assert L.lib.bsy_sizeof_op() == ctypes.sizeof(L.Op) == 624
    # nk and kdim took the two reserved words: every other field is where it was
    assert L.Op.nk.offset == L.Op.lvl_stride.offset + 4 * L.BSY_MAX_LEVELS and L.Op.in_dtype.offset == L.Op.nk.offset + 4
    assert L.Op.kdim.offset == L.Op.ksplit.offset + 4 and L.Op.msk.offset == L.Op.kdim.offset + 4


def test_pose_graph_support_and_stride():
    from bs_yolo_amd.plugin import SUPPORTED_HEADS, graph_support, max_stride
    assert "Pose" in SUPPORTED_HEADS
    for fam, gs in (("yolo11", 32), ("yolov8", 32), ("yolov8-p6", 64)):
        cfg = stock_cfg(fam, "n", 1, "pose", kpt_shape=(17, 3))
        assert graph_support(cfg) == {"fp16": True, "fp32": True} and max_stride(cfg) == gs


# ---- device: the decode launch's keypoint mode alone ----------------------------------------------------------------------
LEVELS = {3: ([(9, 8), (2, 3), (1, 2)], [8.0, 16.0, 32.0]),            # 72 anchors: a full 64-anchor tile and a tail of 8; two partial tiles
          4: ([(9, 8), (3, 5), (2, 3), (1, 2)], [8.0, 16.0, 32.0, 64.0])}  # four levels: the HALVES instance


def _kpt_case(T, nl, nc, nkpt, kdim, koff=0, B=2, seed=0):
    """Logit maps of a Pose head's last convs as the plan lays them out (NHWC f32; class rows padded to 4 floats, keypoint rows to 8
    plus `koff` channels in front), NaN wherever the kernel must not look."""
    g = torch.Generator().manual_seed(1000 * nl + 100 * nc + 7 * nkpt + kdim + seed)
    hw, strides = LEVELS[nl]
    nk = nkpt * kdim
    box = [torch.randn(B, h * w, 64, generator=g) * 2 for h, w in hw]
    cls = [torch.randn(B, h * w, nc, generator=g) * 3 for h, w in hw]
    kpt = [torch.randn(B, h * w, nk, generator=g) * 3 for h, w in hw]
    ldc, ldk = (nc + 3) // 4 * 4, (nk + 7) // 8 * 8 + 2 * koff
    tb = [poisoned((B * t.shape[1], 64), 0, 64, t.reshape(-1, 64), NAN) for t in box]
    tc = [poisoned((B * t.shape[1], ldc), 0, nc, t.reshape(-1, nc), NAN) for t in cls]
    tk = [poisoned((B * t.shape[1], ldk), koff, nk, t.reshape(-1, nk), NAN) for t in kpt]
    raw = torch.cat([t.transpose(1, 2) for t in kpt], 2).to(T).contiguous()  # (B, nk, A): Pose.forward's `kpt`, rounded to T
    return hw, strides, nk, (tb, tc, tk), raw


def _decode_op(T, nl, B, nc, nk, kdim, hw, strides, tensors, koff=0, with_raw=True):
    """(op, ext tensors, y, raw output, their whole allocations): slots 0-3 box, 4-7 class, 8-11 keypoint maps, 12 y, 13 raw."""
    tb, tc, tk = tensors
    A = sum(h * w for h, w in hw)
    op = new_op(L.OP_DECODE, 0, B, 0, 0)
    op.nl, op.nc, op.A, op.out_dtype, op.nk, op.kdim = nl, nc, A, L.dtype_code(T), nk, kdim
    ext = [None] * 14
    for l, (h, w) in enumerate(hw):
        op.box[l], op.cls[l] = view(l, 64, 0, 64), view(4 + l, tc[l].shape[-1], 0, nc)
        ext[l], ext[4 + l] = tb[l], tc[l]
        if nk:
            op.msk[l], ext[8 + l] = view(8 + l, tk[l].shape[-1], koff, nk), tk[l]
        op.lvl_h[l], op.lvl_w[l], op.lvl_stride[l] = h, w, strides[l]
    poison = POISON16 if T == torch.float16 else POISON32
    ny, nr = B * (4 + nc + nk) * A, B * nk * A
    yall = torch.full((ny + 64,), poison, dtype=T, device=DEV)
    rall = torch.full((nr + 64,), poison, dtype=T, device=DEV)
    op.dst, ext[12] = view(12, 0, 0, 4 + nc + nk), yall
    if nk:
        op.res = view(13, 0, 0, nk)
        ext[13] = rall if with_raw else None
    return op, ext, yall[:ny].view(B, 4 + nc + nk, A), rall[:nr].view(B, nk, A), (yall, rall, ny, nr, poison)


def _tail_intact(alloc):
    yall, rall, ny, nr, poison = alloc
    want = bits(torch.full((1,), poison, dtype=yall.dtype)).item()
    return bool((bits(yall[ny:]) == want).all()) and bool((bits(rall[nr:]) == want).all())


def _check_kpt_mode(T, nl, nc, nkpt, kdim, koff):
    from bs_yolo_amd import ops as O
    B = 2
    hw, strides, nk, tensors, raw_want = _kpt_case(T, nl, nc, nkpt, kdim, koff, B)
    op, ext, y, raw, alloc = _decode_op(T, nl, B, nc, nk, kdim, hw, strides, tensors, koff)
    run_op(op, ext)
    assert _tail_intact(alloc), "a store behind y or the raw tensor"
    # the raw rows are the logits rounded to T; the keypoint rows are bsy_kpts_decode of exactly those
    assert torch.equal(bits(raw), bits(raw_want))
    want = O.kpts_decode(raw_want.to(DEV), hw, strides, (nkpt, kdim))
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all(), "a padding NaN reached the output"
    assert torch.equal(bits(y[:, 4 + nc:]), bits(want))
    # boxes and scores are the plain launch's (HALVES at four levels in both)
    op0, ext0, y0, _, alloc0 = _decode_op(T, nl, B, nc, 0, 0, hw, strides, tensors)
    run_op(op0, ext0)
    assert _tail_intact(alloc0) and torch.equal(bits(y[:, :4 + nc]), bits(y0))
    # the raw slot is optional: unbound, y is the same and nothing else is written
    opn, extn, yn, rawn, allocn = _decode_op(T, nl, B, nc, nk, kdim, hw, strides, tensors, koff, with_raw=False)
    run_op(opn, extn)
    assert torch.equal(bits(yn), bits(y)) and _tail_intact(allocn) and bool((rawn == allocn[4]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("kshape", [(17, 3), (5, 2), (1, 2), (64, 3)])
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("nl", [3, 4])
@pytest.mark.parametrize("T", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_decode_keypoint_mode_alone(T, nl, nc, kshape):
    _check_kpt_mode(T, nl, nc, kshape[0], kshape[1], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("nl", [3, 4])
@pytest.mark.parametrize("T", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_decode_keypoint_views_at_a_channel_offset(T, nl):
    """The keypoint maps as views 4 channels into rows 8 channels wider than their payload, NaN on both sides."""
    _check_kpt_mode(T, nl, 3, 17, 3, 4)
    _check_kpt_mode(T, nl, 1, 5, 2, 4)


@pytest.mark.gpu
def test_decode_keypoint_mode_refuses_bad_arguments():
    T, nl, B, nc = torch.float32, 3, 2, 1
    hw, strides, nk, tensors, _ = _kpt_case(T, nl, nc, 17, 3)

    def refused(change):
        op, ext, y, raw, alloc = _decode_op(T, nl, B, nc, nk, 3, hw, strides, tensors)
        change(op)
        with pytest.raises(L.BsyError, match=r"decode.*status -1"):
            run_op(op, ext)
        torch.cuda.synchronize()
        assert bool((y == alloc[4]).all()) and bool((raw == alloc[4]).all()), "the refused op launched"

    refused(lambda op: setattr(op, "nm", 32))               # keypoints with mask coefficients
    refused(lambda op: setattr(op, "ne", 1))                # keypoints with the angle
    refused(lambda op: setattr(op, "nk", 52))               # 52 channels are no whole number of (x, y, v) keypoints
    refused(lambda op: setattr(op, "kdim", 4))
    refused(lambda op: setattr(op, "kdim", 0))
    refused(lambda op: (setattr(op, "nk", 65 * 3),))        # more than 64 keypoints
    ldk = tensors[2][0].shape[-1]
    refused(lambda op: op.msk.__setitem__(1, view(9, ldk, 2, nk)))      # a view 8 bytes into a 16-byte piece
    refused(lambda op: op.msk.__setitem__(0, view(8, ldk - 2, 0, nk)))  # rows that are no multiple of 4 floats
    refused(lambda op: op.msk.__setitem__(2, view(10, 48, 0, nk)))      # rows shorter than the payload


# ---- device: the graphs against the reference ---------------------------------------------------------------------------------
def _engine(tag, precision, **kw):
    from bs_yolo_amd.engine import YoloEngine
    meta = fixture(tag)[1]
    return YoloEngine(_cfg(meta), _sd(tag), bn_eps=meta["bn_eps"], precision=precision, **kw)


TOL = {"fp16": (1e-2, 1.0), "fp32x": (1e-3, None), "fp32": (1e-3, None)}  # score, box (None: 1e-3 imgsz): the project's bounds
# Keypoint x / y on the fp16 path: the logit's fp16-storage error times 2 x stride (up to 128 on the P6 graph) has no derived bound.
# KPT_XY_FP16 is the largest |x or y - reference| over every fixture and input, in pixels, measured on an MI355X (the inputs are
# fixed and the engine is bit-reproducible); the assertion is twice that, the margin the classification graphs use.
KPT_XY_FP16 = 0.9158  # measured 9.157410e-01 (yolo11n_pose, the (2, 96, 128) input; the other graphs: 0.035 .. 0.695)


def _graph_errors(tag, precision, eng, si):
    """One input through the engine: the structural identities asserted, the errors against the fixture returned."""
    from bs_yolo_amd import ops as O
    z, meta = fixture(tag)
    nc, (nkpt, kdim) = meta["nc"], meta["kpt_shape"]
    nk = nkpt * kdim
    x = x_of(meta, si)
    xin = (x.half() if precision == "fp16" else x).to(DEV)
    y, (raws, kpt) = eng(xin)
    y, kpt = y.clone(), kpt.clone()
    y2, (_, kpt2) = eng(xin)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(kpt, kpt2)  # the same input twice: the same bits
    A = y.shape[-1]
    levels = [(x.shape[2] // int(s), x.shape[3] // int(s)) for s in meta["stride"]]
    assert A == sum(h * w for h, w in levels) and len(raws) == len(levels)
    assert tuple(y.shape) == (x.shape[0], 4 + nc + nk, A) and tuple(kpt.shape) == (x.shape[0], nk, A) and y.dtype == kpt.dtype == xin.dtype
    assert all(tuple(r.shape) == (x.shape[0], 64 + nc, h, w) for r, (h, w) in zip(raws, levels))
    # the invariant: the keypoint rows are bsy_kpts_decode of the raw logits the engine returns, bit for bit, in every precision
    assert torch.equal(bits(y[:, 4 + nc:]), bits(O.kpts_decode(kpt, levels, meta["stride"], (nkpt, kdim))))
    yr, yref = y.float().cpu().numpy(), z[f"y{si}"]
    kr, kref = yr[:, 4 + nc:].reshape(-1, nkpt, kdim, A), yref[:, 4 + nc:].reshape(-1, nkpt, kdim, A)
    e = {"score": np.abs(yr[:, 4:4 + nc] - yref[:, 4:4 + nc]).max(), "box": np.abs(yr[:, :4] - yref[:, :4]).max(),
         "xy": np.abs(kr[:, :, :2] - kref[:, :, :2]).max(), "vis": np.abs(kr[:, :, 2:] - kref[:, :, 2:]).max() if kdim == 3 else 0.0}
    rel = 3e-2 if precision == "fp16" else 1e-3  # test_obb's raw-map bound
    kw = z[f"kpt{si}"]
    e["kpt"] = np.abs(kpt.float().cpu().numpy() - kw).max() / max(1.0, np.abs(kw).max())
    e["raw"] = 0.0
    for l, r in enumerate(raws):
        if f"raw{si}_{l}" in z:
            rr = z[f"raw{si}_{l}"]
            e["raw"] = max(e["raw"], np.abs(r.float().cpu().numpy() - rr).max() / max(1.0, np.abs(rr).max()))
    assert si not in meta["raw_shapes"] or all(f"raw{si}_{l}" in z for l in range(len(levels)))
    return e, rel, max(x.shape[2], x.shape[3])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", GRAPHS)
def test_pose_graph_matches_reference(tag, precision):
    meta = fixture(tag)[1]
    eng = _engine(tag, precision)
    assert eng.task == "pose" and eng.meta["nk"] == meta["kpt_shape"][0] * meta["kpt_shape"][1] and eng.nl == len(meta["stride"])
    ts, tb = TOL[precision]
    for si in range(len(meta["shapes"])):
        e, rel, imgsz = _graph_errors(tag, precision, eng, si)
        print(tag, precision, si, " ".join(f"{k} {v:.3e}" for k, v in e.items()))
        assert e["score"] < ts, (tag, precision, si, "score", e["score"])
        assert e["box"] < (tb if tb is not None else 1e-3 * imgsz), (tag, precision, si, "box", e["box"])
        assert e["vis"] < ts, (tag, precision, si, "visibility", e["vis"])
        assert e["kpt"] <= rel and e["raw"] <= rel, (tag, precision, si, "raw", e["kpt"], e["raw"])
        if precision == "fp16":
            assert e["xy"] <= 2 * KPT_XY_FP16, (tag, si, "keypoint x / y", e["xy"])
        else:
            assert e["xy"] <= 1e-3 * imgsz, (tag, precision, si, "keypoint x / y", e["xy"])
    eng.close()


@pytest.mark.gpu
def test_pose_graph_without_raw_outputs_and_in_chunks(monkeypatch):
    tag = "yolo11n_pose"
    meta = fixture(tag)[1]
    eng = _engine(tag, "fp32")
    x = x_of(meta, 1).to(DEV)
    y, (raws, kpt) = eng(x)
    y_full, kpt_full, raw_full = y.clone(), kpt.clone(), [r.clone() for r in raws]
    yn, (rn, kn) = eng(x, want_raw=False)
    torch.cuda.synchronize()
    assert rn == [None, None, None] and kn is None and torch.equal(yn, y_full)
    monkeypatch.setattr(eng, "_max_view_elems", lambda H, W: (1 << 31) // 2)  # forces the chunked large-batch path
    yc, (rc, kc) = eng(x)
    torch.cuda.synchronize()
    assert torch.equal(yc, y_full) and torch.equal(kc, kpt_full) and all(torch.equal(a, b) for a, b in zip(rc, raw_full))
    yc, (rc, kc) = eng(x, want_raw=False)
    assert torch.equal(yc, y_full) and rc == [None, None, None] and kc is None
    ya, (_, ka) = eng(x, augment=True)  # the reference augments DetectionModel only (tasks.py:356-358): the plain forward
    torch.cuda.synchronize()
    assert torch.equal(ya, y_full) and torch.equal(ka, kpt_full)
    prof, plan = eng.profile(x)
    assert len(prof) == len(plan.ops) and sum(1 for _, kind, _ in prof if kind == L.OP_DECODE) == 1
    eng.close()


@pytest.mark.gpu
def test_pose_graph_mode_replays_the_eager_bits():
    tag = "yolo11n_pose"
    meta = fixture(tag)[1]
    xin = x_of(meta, 1).half().to(DEV)
    plain = _engine(tag, "fp16", autotune=False)
    y, (raws, kpt) = plain(xin)
    y, kpt, raws = y.clone(), kpt.clone(), [r.clone() for r in raws]
    plain.close()
    graph = _engine(tag, "fp16", autotune=False, graph=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        outs = []
        for _ in range(4):  # ring of 3: the fourth forward replays the first slot's graph
            yg, (rg, kg) = graph(xin)
            outs.append((yg.clone(), kg.clone(), [r.clone() for r in rg]))
        yn, (rn, kn) = graph(xin, want_raw=False)
        yn = yn.clone()
    s.synchronize()
    torch.cuda.synchronize()
    assert graph.graph_stats["captures"] >= 1 and graph.graph_stats["replays"] >= 1, graph.graph_stats
    for yg, kg, rg in outs:
        assert torch.equal(yg, y) and torch.equal(kg, kpt) and all(torch.equal(a, b) for a, b in zip(rg, raws))
    assert torch.equal(yn, y) and kn is None and rn == [None, None, None]
    graph.close()


@pytest.mark.gpu
def test_nms_on_the_pose_graph_output_matches_the_oracle():
    """The nk keypoint rows ride through bsy_nms as extra columns: on the fp32 engine's own y the device rows are the oracle's."""
    from bs_yolo_amd import nms as HN
    tag = "yolo11n_pose"
    meta = fixture(tag)[1]
    nk = meta["kpt_shape"][0] * meta["kpt_shape"][1]
    eng = _engine(tag, "fp32")
    for si in range(len(meta["shapes"])):
        y, _ = eng(x_of(meta, si).to(DEV), want_raw=False)
        ref = PP.non_max_suppression(y.cpu().clone(), meta["nms_conf"], meta["nms_iou"], nc=meta["nc"])
        det, counts = HN.nms_batched(y.clone(), meta["nms_conf"], meta["nms_iou"], nc=meta["nc"])
        torch.cuda.synchronize()
        assert det.shape[-1] == 6 + nk and len(ref) == y.shape[0]
        for b, r in enumerate(ref):
            n = int(counts[b])
            assert n == len(r) >= 1, (si, b, n, len(r))  # (the generator chose conf so that the reference keeps 5 .. 300 rows)
            assert torch.equal(det[b, :n].cpu(), r), (si, b)
    eng.close()


# ---- device: the plugin -----------------------------------------------------------------------------------------------------
class PoseModel(torch.nn.Module):
    """Stand-in for the reference's PoseModel: `.yaml` (with the top-level kpt_shape the head's argument names), the reference's
    parameter names with the fixture's values, and an original forward that only counts its calls (the engine must not reach it)."""

    def __init__(self, tag):
        super().__init__()
        meta = fixture(tag)[1]
        self.yaml = _cfg(meta)
        for name, t in _sd(tag).items():
            mod = self
            *path, leaf = name.split(".")
            for p in path:
                if not hasattr(mod, p):
                    mod.add_module(p, torch.nn.BatchNorm2d(t.numel(), eps=meta["bn_eps"]) if p == "bn" else torch.nn.Module())
                mod = getattr(mod, p)
            if isinstance(mod, torch.nn.BatchNorm2d):
                with torch.no_grad():
                    getattr(mod, leaf).copy_(t)
            else:
                mod.register_parameter(leaf, torch.nn.Parameter(t.clone(), requires_grad=False))
        self.calls = 0
        self.eval()

    def forward(self, x, *args, **kwargs):
        self.calls += 1
        return "original"


@pytest.mark.gpu
def test_accelerate_pose_model():
    from bs_yolo_amd import plugin
    tag = "yolo11n_pose"
    z, meta = fixture(tag)
    nc = meta["nc"]
    m = PoseModel(tag).to(DEV)
    assert plugin.accelerate(m) is m
    x = x_of(meta, 1).to(DEV)
    y, (raws, kpt) = m(x)  # fp32 input: the fp32x engine
    torch.cuda.synchronize()
    assert m.calls == 0 and m._bsy_state["fp32_calls"] == 1 and len(raws) == 3 and y.dtype == torch.float32
    yr, yref = y.cpu().numpy(), z["y1"]
    kr, kref = yr[:, 4 + nc:].reshape(2, 17, 3, -1), yref[:, 4 + nc:].reshape(2, 17, 3, -1)
    assert np.abs(yr[:, 4:4 + nc] - yref[:, 4:4 + nc]).max() <= 1e-3 and np.abs(yr[:, :4] - yref[:, :4]).max() <= 1e-3 * 128
    assert np.abs(kr[:, :, :2] - kref[:, :, :2]).max() <= 1e-3 * 128 and np.abs(kr[:, :, 2] - kref[:, :, 2]).max() <= 1e-3
    assert np.abs(kpt.cpu().numpy() - z["kpt1"]).max() <= 1e-3 * max(1.0, np.abs(z["kpt1"]).max())
    yh, (_, kh) = m(x.half())  # fp16 input: the fp16 engine
    torch.cuda.synchronize()
    assert m.calls == 0 and m._bsy_state["engine_calls"] == 1 and yh.dtype == kh.dtype == torch.float16
    # what stays on the original forward
    n = 0
    assert m(x, augment=True) == "original"; n += 1  # the reference runs pose single-scale (tasks.py:356-358)
    head = list(m.model.children())[-1]
    head.export = True  # Pose.export: y alone, and kpts_decode's export branch is other arithmetic (head.py:250, :255-272)
    assert m(x) == "original"; n += 1
    head.export = False
    m.train(); assert m(x) == "original"; n += 1; m.eval()
    assert m.calls == n and m._bsy_state["fallbacks"] == n
    y3, _ = m(x)
    assert m.calls == n and torch.equal(y3, y)
    plugin.restore(m)
