"""Four-level detection heads (the P2 and P6 graphs: yolov8-p2, yolov8-p6, yolov5-p6, yolov8-seg-p6) on the engine: graph descriptions,
plan, external slots, C ABI, decode / raw-map kernels, the fused head, host-side plumbing and the plugin hooks, against fixtures made
by running the reference (tests/golden/make_p2p6_fixtures.py).  The P6 shapes put a 1 x 1 and a 2 x 3 map on the stride-64 level."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from bs_yolo_amd import lib as L
from bs_yolo_amd.graphs import stock_cfg
from bs_yolo_amd.plan import Plan
from bs_yolo_amd.weights import pack_plan_weights, synth_state_dict
from graph_helpers import RawBounds, RefModel, YBounds, cfg_of, check_raw, check_y, engine, fixture, level_of_anchor, state_dict, x_of
from op_plan_helpers import DEV

GRAPHS = ["yolov8n_p2", "yolov8n_p6", "yolov5n_p6", "yolov8n_seg_p6"]
DETECT = GRAPHS[:3]
FAMILIES = ["yolov8-p2", "yolov8-p6", "yolov5-p6"]
STRIDES = {"yolov8-p2": [4, 8, 16, 32], "yolov8-p6": [8, 16, 32, 64], "yolov5-p6": [8, 16, 32, 64]}
SHAPES = {"yolov8-p2": [(1, 64, 64), (2, 96, 128)], "yolov8-p6": [(1, 64, 64), (2, 128, 192)], "yolov5-p6": [(1, 64, 64), (2, 128, 192)]}
ANCHORS = {"yolov8-p2": [340, 1020], "yolov8-p6": [85, 510], "yolov5-p6": [85, 510]}
NC = 12
# The project's parity bounds (test_obb.py TOL, README).  fp32 / fp32x: score <= 1e-3, box <= 1e-3 imgsz.  fp16: score < 1e-2, box the
# project's 1 px at stride 32 restated per level as stride / 32 px -- the error is a DFL distance in grid units times the stride -- so
# 2 px on a stride-64 level and 1 px on every other.  Raw maps: 3e-2 (fp16) or 1e-3 of max(1, maximum).
Y_BOUNDS = YBounds(score16=1e-2, p999_16=None, box16=1.0, score32=1e-3, box32=1e-3)
RAW_BOUNDS = RawBounds(rel16=3e-2, strict16=False, floor16=True, rel32=1e-3)
# mask coefficients and prototypes: the bounds test_gpu_parity.py holds the three-level Segment graphs to
MASK_BOUNDS = RawBounds(rel16=2e-2, strict16=True, floor16=False, rel32=1e-3)


# ---- host side (no GPU) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "fp32x", "fp32"])
@pytest.mark.parametrize("family", FAMILIES)
def test_four_level_plans(family, precision):
    cfg = stock_cfg(family, "n", NC, "detect")
    for (b, h, w), A in zip(SHAPES[family], ANCHORS[family]):
        plan = Plan(cfg, b, h, w, precision=precision)
        m = plan.meta
        assert len(m["levels"]) == 4 and m["strides"] == [float(s) for s in STRIDES[family]] and m["A"] == A
        assert m["levels"] == [(h // s, w // s) for s in STRIDES[family]]
        kinds = [o["kind"] for o in plan.ops]
        if precision == "fp16":  # the default: the fused head, on every level
            assert kinds.count(L.OP_DECODE) == 0 and kinds.count(L.OP_RAW_NCHW) == 0
            for mode in (3, 2):  # box, class
                assert sorted(o["level"] for o in plan.ops if o.get("out_f32", 0) == mode) == [0, 1, 2, 3]
            a0 = 0
            for l, (lh, lw) in enumerate(m["levels"]):
                for o in plan.ops:
                    if o.get("out_f32", 0) >= 2 and o["level"] == l:
                        assert o["lvl_h"] == [lh, a0] and o["lvl_w"] == [lw] and o["lvl_stride"] == [float(STRIDES[family][l])] and o["A"] == A
                a0 += lh * lw
        unfused = Plan(cfg, b, h, w, precision=precision, fuse_head=False)
        dec = [o for o in unfused.ops if o["kind"] == L.OP_DECODE]
        raw = [o for o in unfused.ops if o["kind"] == L.OP_RAW_NCHW]
        assert len(dec) == 1 and dec[0]["nl"] == 4 and len(dec[0]["box"]) == 4 and len(dec[0]["cls"]) == 4
        assert [o["level"] for o in raw] == [0, 1, 2, 3] and not any(o.get("out_f32", 0) >= 2 for o in unfused.ops)


def test_segment_on_four_levels_takes_the_decode_launch(monkeypatch):
    monkeypatch.delenv("BSY_LANES", raising=False)
    cfg = stock_cfg("yolov8-p6", "n", NC, "segment")
    for precision in ("fp16", "fp32x", "fp32"):
        plan = Plan(cfg, 2, 128, 192, precision=precision)
        dec = [o for o in plan.ops if o["kind"] == L.OP_DECODE]
        assert len(dec) == 1 and dec[0]["nl"] == 4 and dec[0]["nm"] == 32 and len(dec[0]["msk"]) == 4
        assert plan.meta["A"] == 510 and plan.meta["nm"] == 32 and plan.meta["proto_hw"] == (32, 48)
        lanes = {o.get("lane", 0) for o in Plan(cfg, 2, 128, 192, precision=precision, lanes=True).ops}
        assert lanes == set(range(3 * 4))  # box, class and mask chain of every level on a lane of its own


def _ext_roles(plan):
    """{slot: set of roles} of every external view of a plan."""
    roles = {}

    def add(t, role):
        if t is not None and t.buf >= L.BSY_EXT_BASE:
            roles.setdefault(t.buf - L.BSY_EXT_BASE, set()).add(role)

    for o in plan.ops:
        add(o.get("src0"), "image")
        if o["kind"] == L.OP_RAW_NCHW:
            add(o["dst"], ("raw", o["level"]))
        elif o["kind"] == L.OP_NHWC2NCHW:
            add(o["dst"], "proto")
        elif o["kind"] == L.OP_DECODE or o.get("out_f32", 0) >= 2:
            add(o["dst"], "y")
            if o.get("out_f32", 0) >= 2:
                add(o["box"][0], ("raw", o["level"]))
        else:
            add(o.get("dst"), ("other", o["name"]))
    return roles


@pytest.mark.parametrize("tag", GRAPHS)
def test_external_slots_are_distinct(tag):
    _, meta = fixture(tag)
    for kw in ({}, {"fuse_head": False}, {"precision": "fp32"}):
        roles = _ext_roles(Plan(cfg_of(meta), 1, 64, 64, **kw))
        assert all(len(r) == 1 for r in roles.values()), roles  # no two external views share a slot
        by_role = {next(iter(r)): s for s, r in roles.items()}
        want = {"image", "y"} | {("raw", l) for l in range(4)} | ({"proto"} if meta["task"] == "segment" else set())
        assert set(by_role) == want
        # the slots three-level plans use have not moved; the fourth raw map sits behind the proto slot
        assert [by_role["image"], by_role["y"]] + [by_role[("raw", l)] for l in range(4)] == [0, 1, 2, 3, 4, 6]
        assert meta["task"] != "segment" or by_role["proto"] == 5
    three = _ext_roles(Plan(stock_cfg("yolov8", "n", NC, "segment"), 1, 64, 64))
    assert {next(iter(r)): s for s, r in three.items()} == {"image": 0, "y": 1, ("raw", 0): 2, ("raw", 1): 3, ("raw", 2): 4, "proto": 5}


@pytest.mark.parametrize("tag", GRAPHS)
def test_weights_pack_from_the_reference_state_dict(tag):
    _, meta = fixture(tag)
    sd = state_dict(tag, None)
    seen = set()

    class Recording(dict):
        def __getitem__(self, k):
            seen.add(k)
            return dict.__getitem__(self, k)

    for precision in ("fp16", "fp32x"):
        pack_plan_weights(Plan(cfg_of(meta), 1, 64, 64, precision=precision), Recording(sd))  # a missing key raises KeyError
    branches = ("cv2", "cv3", "cv4") if meta["task"] == "segment" else ("cv2", "cv3")
    fourth = {n for n in sd if any(f".{b}.3." in n for b in branches) and not n.endswith("num_batches_tracked")}
    assert len(fourth) == len(branches) * (2 * 5 + 2) and fourth <= seen
    assert {n for n in sd if n not in seen and not n.endswith("num_batches_tracked")} == {n for n in sd if n.endswith(".dfl.conv.weight")}


def test_c_ops_carry_four_levels():
    plan = Plan(stock_cfg("yolov8-p6", "n", NC, "segment"), 2, 128, 192)
    pack_plan_weights(plan, synth_state_dict(plan))
    dec = [o for o in plan.c_ops() if o.kind == L.OP_DECODE]
    assert len(dec) == 1 and dec[0].nl == 4 and L.BSY_MAX_LEVELS == 4
    assert list(dec[0].lvl_h) == [16, 8, 4, 2] and list(dec[0].lvl_w) == [24, 12, 6, 3] and list(dec[0].lvl_stride) == [8.0, 16.0, 32.0, 64.0]
    for views in (dec[0].box, dec[0].cls, dec[0].msk):
        assert len(views) == 4 and all(v.buf >= 0 and v.ld % 4 == 0 for v in views) and len({v.buf for v in views}) == 4
    raw = [o for o in plan.c_ops() if o.kind == L.OP_RAW_NCHW]
    assert [(o.level, o.dst.buf - L.BSY_EXT_BASE) for o in raw] == [(0, 2), (1, 3), (2, 4), (3, 6)]


def test_graph_support_and_what_is_refused():
    from bs_yolo_amd.plugin import graph_support, max_stride
    for tag in GRAPHS:
        _, meta = fixture(tag)
        assert graph_support(cfg_of(meta)) == {"fp16": True, "fp32": True}
        assert max_stride(cfg_of(meta)) == max(STRIDES[meta["family"]])
    assert max_stride(stock_cfg("yolo11", "n")) == 32
    five = stock_cfg("yolov8-p6", "n", NC, "detect")
    five["head"][-1] = [[20, 23, 26, 29, 29], 1, "Detect", ["nc"]]
    for precision in ("fp16", "fp32"):
        with pytest.raises(NotImplementedError):
            Plan(five, 1, 64, 64, precision=precision)
        for family in FAMILIES:  # an OBB head on four levels: the reference ships no such graph
            with pytest.raises(NotImplementedError):
                Plan(stock_cfg(family, "n", NC, "obb"), 1, 64, 64, precision=precision)
    assert graph_support(five) == {"fp16": False, "fp32": False}
    with pytest.raises(ValueError):
        stock_cfg("yolov8-p2", "n", NC, "pose")


def test_header_declares_the_level_count(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "a host C compiler is needed"
    src = tmp_path / "levels.c"
    src.write_text('#include "bsyolo.h"\n#include <stdio.h>\n'
                   'int main(void) { bsy_op o; printf("%d %d %d\\n", BSY_MAX_LEVELS, (int)sizeof(bsy_op), (int)(sizeof(o.box) / sizeof(o.box[0]))); return 0; }\n')
    exe = tmp_path / "levels"
    r = subprocess.run([cc, "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    levels, size, nbox = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert levels == nbox == L.BSY_MAX_LEVELS == 4
    assert size == C.sizeof(L.Op) == L.lib.bsy_sizeof_op()
    assert len(L.Op().box) == len(L.Op().lvl_stride) == 4
    common = (ROOT / "bs_yolo_amd" / "csrc" / "common.h").read_text()
    assert "box[BSY_MAX_LEVELS]" in common and "box[3]" not in common


# ---- device ---------------------------------------------------------------------------------------------------------------
def _engine(tag, precision, **kw):
    return engine(tag, precision, None, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp16", "fp32x", "fp32"])
@pytest.mark.parametrize("tag", GRAPHS)
def test_four_level_graph_matches_reference(tag, precision):
    z, meta = fixture(tag)
    eng = _engine(tag, precision)
    seg = meta["task"] == "segment"
    for si, (b, h, w) in enumerate(meta["shapes"]):
        x = x_of(meta, si)
        xin = (x.half() if precision == "fp16" else x).to(DEV)
        y, aux = eng(xin)
        raws = aux[0] if seg else aux
        y1, r1 = y.clone(), [r.clone() for r in raws]
        p1 = aux[2].clone() if seg else None
        y2, aux2 = eng(xin)
        torch.cuda.synchronize()
        raws2 = aux2[0] if seg else aux2
        assert torch.equal(y1, y2) and all(torch.equal(a, c) for a, c in zip(r1, raws2))  # the same input twice: the same bits
        levels = [(h // int(s), w // int(s)) for s in meta["stride"]]
        A = sum(lh * lw for lh, lw in levels)
        assert tuple(y1.shape) == (b, 4 + NC + (32 if seg else 0), A) and len(r1) == 4
        assert [tuple(r.shape) for r in r1] == [(b, 64 + NC, lh, lw) for lh, lw in levels]
        yr, yref = y1.float().cpu().numpy(), z[f"y{si}"]
        check_y(yr, yref, meta["stride"], level_of_anchor(levels), max(h, w), precision, f"{tag} shape {si}", NC, Y_BOUNDS)
        if si in meta["raw_shapes"]:
            for l, r in enumerate(r1):
                check_raw(r.float().cpu().numpy(), z[f"raw{si}_{l}"], precision, f"{tag} shape {si} raw {l}", RAW_BOUNDS)
        if seg:
            assert torch.equal(aux[1], y[:, 4 + NC:]) and torch.equal(p1, aux2[2])
            check_raw(yr[:, 4 + NC:], z[f"mc{si}"], precision, f"{tag} shape {si} mc", MASK_BOUNDS)
            check_raw(p1.float().cpu().numpy(), z[f"proto{si}"], precision, f"{tag} shape {si} proto", MASK_BOUNDS)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", DETECT)
def test_fused_head_is_not_a_different_answer(tag):
    """fp16 path: the fused head (default), the same untuned, and the decode launch return the same bits (for heads of four levels the
    decode kernel sums the DFL in the fused epilogue's order, csrc/detect.hip HALVES)."""
    _, meta = fixture(tag)
    engines = [_engine(tag, "fp16"), _engine(tag, "fp16", autotune=False), _engine(tag, "fp16", fuse_head=False)]
    for si in range(len(meta["shapes"])):
        x = x_of(meta, si).half().to(DEV)
        outs = [e(x) for e in engines]
        torch.cuda.synchronize()
        plans = [e.plan_for(x.shape[0], x.shape[2], x.shape[3], x.dtype, x.dtype)[0] for e in engines]
        assert [sum(o["kind"] == L.OP_DECODE for o in p.ops) for p in plans] == [0, 0, 1]
        for y, raws in outs[1:]:
            assert torch.equal(y, outs[0][0]) and len(raws) == 4 and all(torch.equal(a, b) for a, b in zip(raws, outs[0][1]))
    assert engines[0].tuning(*meta["shapes"][1]) and not engines[1].tuning(*meta["shapes"][1])
    for e in engines:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag,precision", [("yolov8n_p2", "fp16"), ("yolov8n_seg_p6", "fp16")])
def test_head_lanes_hold_four_levels(tag, precision, monkeypatch):
    """Every (level, branch) chain on a stream of its own -- 2 x 4 lanes for Detect, 3 x 4 for Segment -- joined before the raw outputs:
    the bits of the serial schedule."""
    _, meta = fixture(tag)
    x = x_of(meta, 1).half().to(DEV)
    monkeypatch.setenv("BSY_LANES", "0")
    serial = _engine(tag, precision)
    y0, aux0 = serial(x)
    monkeypatch.setenv("BSY_LANES", "1")
    eng = _engine(tag, precision)
    plan = eng.plan_for(x.shape[0], x.shape[2], x.shape[3], x.dtype, x.dtype)[0]
    assert len({o.get("lane", 0) for o in plan.ops} - {0}) == (3 * 4 - 1 if meta["task"] == "segment" else 2 * 4 - 1)
    for _ in range(2):
        y, aux = eng(x)
        torch.cuda.synchronize()
        r0, r = (aux0[0], aux[0]) if meta["task"] == "segment" else (aux0, aux)
        assert torch.equal(y, y0) and all(torch.equal(a, b) for a, b in zip(r, r0))
        assert meta["task"] != "segment" or torch.equal(aux[2], aux0[2])
    serial.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["yolov8n_p2", "yolov8n_seg_p6"])
def test_without_raw_maps_and_in_chunks(tag, monkeypatch):
    _, meta = fixture(tag)
    seg = meta["task"] == "segment"
    for precision in ("fp16", "fp32"):
        eng = _engine(tag, precision)
        x = x_of(meta, 1)
        x = (x.half() if precision == "fp16" else x).to(DEV)
        y_full, aux_full = eng(x)
        y_full = y_full.clone()
        y, aux = eng(x, want_raw=False)
        assert (aux[0] if seg else aux) == [None] * 4 and torch.equal(y, y_full)
        monkeypatch.setattr(eng, "_max_view_elems", lambda H, W: (1 << 31) // 2)  # forces the chunked large-batch path
        yc, auxc = eng(x)
        rc, rf = (auxc[0], aux_full[0]) if seg else (auxc, aux_full)
        assert torch.equal(yc, y_full) and len(rc) == 4 and all(torch.equal(a, b) for a, b in zip(rc, rf))
        if seg:
            assert torch.equal(auxc[1], yc[:, 4 + NC:]) and torch.equal(auxc[2], aux_full[2])
        yn, auxn = eng(x, want_raw=False)
        assert torch.equal(yn, y_full) and (auxn[0] if seg else auxn) == [None] * 4
        eng.close()


@pytest.mark.gpu
def test_nms_on_the_graph_outputs_matches_reference():
    from bs_yolo_amd import nms as HN
    total = 0
    for tag in GRAPHS:
        z, meta = fixture(tag)
        for si in range(len(meta["shapes"])):
            got = HN.non_max_suppression(torch.from_numpy(z[f"y{si}"]).to(DEV), meta["nms_conf"], meta["nms_iou"], nc=NC)
            assert len(got) == meta["shapes"][si][0]
            for b, g in enumerate(got):
                w = z[f"nms{si}_{b}"]
                assert tuple(g.shape) == w.shape and np.allclose(g.cpu().numpy(), w, atol=1e-5, rtol=0), (tag, si, b)
                total += len(g)
    assert total > 0


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp16", "fp32x", "fp32"])
def test_augment_on_a_p6_graph_matches_reference(precision):
    from bs_yolo_amd import tta as T
    z, meta = fixture("yolov8n_p6")
    eng = _engine("yolov8n_p6", precision)
    x = x_of(meta, 1)
    b, h, w = meta["shapes"][1]
    y, aux = eng((x.half() if precision == "fp16" else x).to(DEV), augment=True)
    torch.cuda.synchronize()
    want = z["aug1"]
    assert aux is None and tuple(y.shape) == want.shape
    # the level of every merged anchor: each pass's window of its own levels (gs = 64: all three passes run at 128 x 192)
    lvl = []
    for p in eng.tta_geometry(h, w):
        lv = level_of_anchor([(p.padded[0] // int(s), p.padded[1] // int(s)) for s in meta["stride"]])
        lvl.append(lv[p.window[0]:p.window[1]])
    lvl = np.concatenate(lvl)
    assert len(lvl) == want.shape[-1] and [p.padded for p in eng.tta_geometry(h, w)] == [(128, 192)] * 3
    assert [p.window for p in eng.tta_geometry(h, w)] == T.reference_windows([510] * 3, 4)
    check_y(y.float().cpu().numpy(), want, meta["stride"], lvl, max(h, w), precision, "augment", NC, Y_BOUNDS)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["yolov8n_p2", "yolov8n_p6"])
def test_accelerate_a_four_level_model(tag):
    from bs_yolo_amd import plugin
    z, meta = fixture(tag)
    m = RefModel(cfg_of(meta), state_dict(tag, None)).to(DEV)
    plugin.accelerate(m)
    x = x_of(meta, 1).to(DEV)
    y, raws = m(x)  # fp32 input: the fp32x engine
    assert m.calls == 0 and len(raws) == 4 and m._bsy_state["fp32_calls"] == 1
    yr = y.cpu().numpy()
    assert np.abs(yr[:, 4:] - z["y1"][:, 4:]).max() <= 1e-3
    assert np.abs(yr[:, :4] - z["y1"][:, :4]).max() <= 1e-3 * max(x.shape[2:])
    # 96 x 128: multiples of 32; on the P6 graph not of its max stride 64 -> the original forward, once
    odd = torch.rand(1, 3, 96, 128, device=DEV)
    res = m(odd)
    if meta["family"] == "yolov8-p6":
        assert res == "original" and m.calls == 1 and m._bsy_state["fallbacks"] == 1
    else:
        assert m.calls == 0 and tuple(res[0].shape) == (1, 4 + NC, 1020)
    plugin.restore(m)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["yolov8n_p2", "yolov5n_p6"])
def test_stand_alone_decode_on_four_levels(tag):
    from bs_yolo_amd import ops as O
    z, meta = fixture(tag)
    eng = _engine(tag, "fp32")
    b, h, w = meta["shapes"][0]
    y, raws = eng(x_of(meta, 0).to(DEV))

    def split(maps):
        maps = [m.to(DEV).float().permute(0, 2, 3, 1) for m in maps]
        return ([m[..., :64].reshape(-1, 64).contiguous() for m in maps], [m[..., 64:].reshape(-1, NC).contiguous() for m in maps],
                [tuple(m.shape[1:3]) for m in maps])

    box, cls, hw = split(raws)  # the engine's own raw maps: the same kernel on the same logits, the same bits
    assert len(hw) == 4 and torch.equal(O.detect_decode(box, cls, hw, meta["stride"], NC), y)
    box, cls, hw = split([torch.from_numpy(z[f"raw0_{l}"]) for l in range(4)])  # the reference's: within the fp32 parity bounds
    got = O.detect_decode(box, cls, hw, meta["stride"], NC).cpu().numpy()
    yr = y.cpu().numpy()
    assert got.shape == yr.shape and np.abs(got[:, 4:] - yr[:, 4:]).max() <= 1e-3 and np.abs(got[:, :4] - yr[:, :4]).max() <= 1e-3 * max(h, w)
    assert np.abs(got[:, 4:] - z["y0"][:, 4:]).max() <= 1e-3 and np.abs(got[:, :4] - z["y0"][:, :4]).max() <= 1e-3 * max(h, w)
    with pytest.raises(L.BsyError):
        O.detect_decode(box + box[:1], cls + cls[:1], hw + hw[:1], meta["stride"] + [128.0], NC)  # five levels
    eng.close()


class Detect(torch.nn.Module):
    """What plugin.install looks at on a reference Detect instance (head.py:21-62), with four levels."""
    reg_max, export, format, end2end = 16, False, None, False

    def __init__(self, strides):
        super().__init__()
        self.nl, self.nc, self.no = len(strides), NC, 64 + NC
        self.stride = torch.tensor(strides)
        self.calls = 0

    def _inference(self, x):
        self.calls += 1
        return "original"


@pytest.mark.gpu
def test_per_module_detect_hook_takes_four_levels():
    from bs_yolo_amd import plugin
    z, meta = fixture("yolov8n_p6")
    head = Detect(meta["stride"]).eval()
    model = torch.nn.Sequential(head)
    assert plugin.install(model) == 1
    y = head._inference([torch.from_numpy(z[f"raw1_{l}"]).to(DEV) for l in range(4)])
    assert head.calls == 0 and head._bsy_block["calls"] == 1
    yr = y.cpu().numpy()
    assert np.abs(yr[:, 4:] - z["y1"][:, 4:]).max() <= 1e-3 and np.abs(yr[:, :4] - z["y1"][:, :4]).max() <= 1e-3 * 192
    assert head._inference([torch.from_numpy(z[f"raw1_{l}"]) for l in range(4)]) == "original"  # CPU tensors: the module's own
    assert plugin.uninstall(model) == 1


@pytest.mark.gpu
def test_sliced_inference_admits_native_tiles_by_the_models_stride():
    """Slices of 96 px are multiples of 32 but not of a P6 graph's stride 64: they take the letterbox route (imgsz 640), not the native
    one (which the engine would refuse); 128-px slices run natively.  The full-image pass is padded to a multiple of 64."""
    from bs_yolo_amd import sahi as HS
    eng = _engine("yolov8n_p6", "fp16", autotune=False)
    assert eng.max_stride == 64 and eng.nl == 4
    seen = []
    model = lambda t, want_raw=False: (seen.append(tuple(t.shape[2:])), eng(t, want_raw=False))[1]  # noqa: E731
    model.max_stride, model.device = eng.max_stride, eng.device
    img = (torch.rand(160, 224, 3, generator=torch.Generator().manual_seed(7)) * 255).to(torch.uint8).to(DEV)
    for size, tile in ((96, (640, 640)), (128, (128, 128))):
        del seen[:]
        det, boxes = HS.get_sliced_prediction(img, model, size, size, conf=0.001)
        assert det.dim() == 2 and det.shape[1] == 6 and len(boxes) > 1
        assert seen[0] == tile and seen[-1] == (128, 128) and all(h % 64 == 0 and w % 64 == 0 for h, w in seen)
    with pytest.raises(ValueError):
        eng(torch.zeros(1, 3, 96, 96, dtype=torch.float16, device=DEV))
    eng.close()
