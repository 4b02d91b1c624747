"""CPU tests of the host side: C-ABI surface, graph flattening, weight packing, letterbox geometry, sharding."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT

from bs_yolo_amd import lib as L
from bs_yolo_amd.graphs import stock_cfg
from bs_yolo_amd.letterbox import LetterBox
from bs_yolo_amd.parallel import shard_bounds
from bs_yolo_amd.plan import Plan
from bs_yolo_amd.weights import fold_conv_bn, pack_plan_weights, pack_record, record_keys, synth_state_dict
from oracle import yolo_ref as R


def test_library_exports_every_declared_symbol():
    hdr = (ROOT / "include" / "bsyolo.h").read_text()
    declared = set(re.findall(r"\b(bsy_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    assert declared == set(L.SYMBOLS), declared ^ set(L.SYMBOLS)
    for s in declared:
        assert hasattr(L.lib, s), s
    assert L.lib.bsy_version() >= 1


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    import ctypes as C
    cp, kp = C.c_int(), C.c_int()
    assert L.lib.bsy_conv_packed_dims(80, 64, 3, C.byref(cp), C.byref(kp)) == 0
    assert (cp.value, kp.value) == (128, 576)
    assert L.lib.bsy_conv_packed_dims(16, 8, 3, C.byref(cp), C.byref(kp)) == 0
    assert (cp.value, kp.value) == (128, 96)
    assert L.lib.bsy_conv_packed_dims(16, 8, 5, C.byref(cp), C.byref(kp)) != 0
    assert b"bad shape" in L.lib.bsy_last_error()
    with pytest.raises(L.BsyError):
        L.check(L.lib.bsy_nms(None, 0, 1, 1, 0, 1, 0.25, 0.45, None, 0, 0, 0, 300, 30000, 7680.0, 1, None, None, None, 0, None))
    assert L.lib.bsy_nms_workspace_bytes(64, 8400, 80, 0, 30000) >= 64 * 16384 * 8
    assert L.lib.bsy_nms_workspace_bytes(2, 8400, 80, 1, 30000) >= 2 * (1 << 20) * 8


def test_header_is_plain_c(tmp_path):
    """The boundary is a C ABI: include/bsyolo.h compiles as strict C99 (no C++ in the signatures), and a C translation unit that
    names every declared entry point links against the shared library (no GPU call is made)."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    hdr = ROOT / "include" / "bsyolo.h"
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", str(hdr)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = sorted(set(re.findall(r"\b(bsy_[a-z0-9_]+)\s*\(", hdr.read_text())))
    src = tmp_path / "abi.c"
    src.write_text('#include "bsyolo.h"\n#include <stdio.h>\nint main(void) {\n  const void* f[] = {' + ", ".join(f"(const void*)(size_t){n}" for n in names) +
                   '};\n  printf("%d %d %d\\n", (int)(sizeof(f) / sizeof(f[0])), bsy_version(), bsy_sizeof_op());\n  return 0;\n}\n')
    exe = tmp_path / "abi"
    r = subprocess.run([gcc, "-std=c99", "-I", str(hdr.parent), str(src), "-o", str(exe), str(L.LIB_PATH), f"-Wl,-rpath,{L.LIB_PATH.parent}",
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    n, ver, sz = map(int, r.stdout.split())
    import ctypes as C
    assert n == len(names) == len(L.SYMBOLS) and ver >= 1 and sz == C.sizeof(L.Op)


def test_op_struct_layout():
    import ctypes as C
    # mirrors include/bsyolo.h: the two int64 offsets sit on an 8-byte boundary after 32 int32 fields
    assert L.Op.w_off.offset == 128 and L.Op.b_off.offset == 136
    assert C.sizeof(L.View) == 16
    assert C.sizeof(L.Op) % 8 == 0


@pytest.mark.parametrize("scale,gflops,nconv", [("n", 6.48, 80), ("s", 21.47, 80), ("m", 67.98, 105)])
def test_plan_work_matches_reference_counts(scale, gflops, nconv, monkeypatch):
    """Dense-conv FLOPs per 640x640 image equal the reference graph (BASELINE.md section 2 / SURVEY 8d); the
    reference counts 81 dense convs for n/s because DFL is a 1x1 conv there (block.py:58-77), here it lives in decode."""
    monkeypatch.setenv("BSY_FUSE_BOXTAIL", "0")  # one op per conv module
    p = Plan(stock_cfg("yolo11", scale), 1, 640, 640, fuse_stem=False, fuse_bneck=False, fuse_dwpw=False, merge_c3k=False, fuse_tail=False)
    dense = 0
    n = 0
    for o in p.ops:
        if o["kind"] in (L.OP_CONV, L.OP_CONV_FIRST):
            cin = 3 if o["kind"] == L.OP_CONV_FIRST else o["src0"].C + (o["src1"].C if o.get("src1") else 0)
            dense += 2 * o["OH"] * o["OW"] * o.get("cout", o["dst"].C) * cin * o["ksize"] ** 2
            n += 1
    assert n == nconv
    assert abs(dense / 1e9 - gflops) < 0.01 * gflops
    assert p.meta["A"] == 8400 and p.meta["strides"] == [8.0, 16.0, 32.0]


def test_box_branch_tail_is_one_op(monkeypatch):
    """Detect's cv2.i.1 + cv2.i.2 (+ DFL) become ONE conv op (plan.py _box_tail) where the branch is 64 wide; the weight records --
    and with them the blob layout and synth_state_dict's draws -- are those of the unfused plan."""
    cfg = stock_cfg("yolo11", "s")
    fused = Plan(cfg, 2, 640, 640)
    monkeypatch.setenv("BSY_FUSE_BOXTAIL", "0")
    plain = Plan(cfg, 2, 640, 640)
    assert list(fused.wrecs) == list(plain.wrecs)
    assert len(plain.ops) - len(fused.ops) == 3 and fused.flops == plain.flops
    tails = [o for o in fused.ops if o["kind"] == L.OP_CONV and o.get("mid_c")]
    assert [o["name"] for o in tails] == [f"model.23.cv2.{i}.1+2" for i in range(3)]
    for o in tails:
        assert (o["ksize"], o["out_f32"], o["act"], o["cout"], o["wkey2"]) == (3, 3, 1, 64, o["wkey"][:-1] + "2")
    monkeypatch.delenv("BSY_FUSE_BOXTAIL")
    # YOLO11x: the box branch is 96 wide (max(16, 384 // 4, 64)) -> no tail
    assert not [o for o in Plan(stock_cfg("yolo11", "x"), 1, 64, 64).ops if o["kind"] == L.OP_CONV and o.get("mid_c")]
    # Segment heads keep the separate decode op (mask coefficients): no tail either
    assert not [o for o in Plan(stock_cfg("yolo11", "n", 80, "segment"), 1, 64, 64).ops if o["kind"] == L.OP_CONV and o.get("mid_c")]


def test_c3k_branch_merge():
    """C3k's cv1 and cv2 (same input) become one conv of twice the width writing the concat buffer; parameters, their
    random draws and the packed rows are those of the two separate convs."""
    from bs_yolo_amd.weights import pack_plan_weights, synth_state_dict
    cfg = stock_cfg("yolo11", "s")
    a, b = Plan(cfg, 1, 64, 64, merge_c3k=False), Plan(cfg, 1, 64, 64, merge_c3k=True)
    assert len(a.ops) - len(b.ops) == 3 and a.flops == b.flops
    merged = [o for o in b.ops if "+" in str(o.get("wkey", ""))]
    assert [o["name"] for o in merged] == ["model.6.m.0.cv1", "model.8.m.0.cv1", "model.22.m.0.cv1"]
    sa, sb = synth_state_dict(a, 0), synth_state_dict(b, 0)
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    ba, bb = pack_plan_weights(a, sa), pack_plan_weights(b, sb)
    ra1, ra2, rb = a.wrecs["model.6.m.0.cv1"], a.wrecs["model.6.m.0.cv2"], b.wrecs["model.6.m.0.cv1+model.6.m.0.cv2"]
    c_, kp = ra1.cout, 128  # 1x1 over 128 input channels: rows of 128 halves
    rows = lambda blob, off, n: blob[off: off + n * kp * 2]
    assert rb.cout == 2 * c_ and rows(bb, rb.w_off, c_) == rows(ba, ra1.w_off, c_)
    assert rows(bb, rb.w_off + c_ * kp * 2, c_) == rows(ba, ra2.w_off, c_)
    assert bb[rb.b_off: rb.b_off + 4 * c_] == ba[ra1.b_off: ra1.b_off + 4 * c_]
    assert bb[rb.b_off + 4 * c_: rb.b_off + 8 * c_] == ba[ra2.b_off: ra2.b_off + 4 * c_]


def test_stem_fusion_peephole():
    """Layers 0 + 1 become one OP_STEM launch where csrc/stem_fused.hip supports the widths (n: 16/32, s: 32/64);
    m/l/x keep two launches.  Work accounting (plan.flops) and the parameter records do not change."""
    for scale, fused in (("n", True), ("s", True), ("m", False)):
        a = Plan(stock_cfg("yolo11", scale), 2, 640, 640, fuse_stem=False, fuse_bneck=False, fuse_tail=False)
        b = Plan(stock_cfg("yolo11", scale), 2, 640, 640, fuse_stem=True, fuse_bneck=False, fuse_tail=False)
        assert a.flops == b.flops and list(a.wrecs) == list(b.wrecs)
        if fused:
            assert len(b.ops) == len(a.ops) - 1 and b.ops[0]["kind"] == L.OP_STEM
            assert b.ops[0]["dst"] is not None and b.ops[0]["mid_c"] == a.ops[0]["dst"].C
            assert b.ops[0]["wkey"] == "model.0" and b.ops[0]["wkey2"] == "model.1"
            assert b.layer_out[0] is None and sum(b.buf_bytes) < sum(a.buf_bytes)
        else:
            assert len(b.ops) == len(a.ops) and b.ops[0]["kind"] == L.OP_CONV_FIRST
    odd = Plan(stock_cfg("yolo11", "s"), 1, 64, 64, fuse_stem=True)
    assert odd.ops[0]["kind"] == L.OP_STEM
    assert L.OP_STEM == 8 and L.Op.mid_c.offset == 380 and L.Op.w2_off.offset == 384 and L.Op.b2_off.offset == 392


def test_bottleneck_fusion_peephole():
    """C3k2's thin Bottlenecks with shortcut (32 -> 16 -> 32: model.2.m.0 of YOLO11s; 64 -> 32 -> 64: model.4.m.0 / model.16.m.0)
    become one OP_BNECK launch each; other widths keep two convs.  FLOP accounting and parameter records are unchanged."""
    a = Plan(stock_cfg("yolo11", "s"), 2, 640, 640, fuse_stem=False, fuse_bneck=False, fuse_tail=False)
    b = Plan(stock_cfg("yolo11", "s"), 2, 640, 640, fuse_stem=False, fuse_bneck=True, fuse_tail=False)
    assert a.flops == b.flops and list(a.wrecs) == list(b.wrecs)
    fused = [o for o in b.ops if o["kind"] == L.OP_BNECK]
    assert [o["name"] for o in fused] == ["model.2.m.0", "model.4.m.0", "model.16.m.0"] and len(b.ops) == len(a.ops) - 3
    o = fused[0]
    assert (o["src0"].C, o["mid_c"], o["dst"].C) == (32, 16, 32) and o["src0"].buf == o["dst"].buf  # slices of the concat buffer
    assert o["wkey"] == "model.2.m.0.cv1" and o["wkey2"] == "model.2.m.0.cv2" and L.OP_BNECK == 9
    assert [(o["src0"].C, o["mid_c"]) for o in fused[1:]] == [(64, 32), (64, 32)]
    for r in ("cv1", "cv2"):
        ra, rb = a.wrecs[f"model.2.m.0.{r}"], b.wrecs[f"model.2.m.0.{r}"]
        assert (ra.kind, ra.cout, ra.cin, ra.k) == (rb.kind, rb.cout, rb.cin, rb.k)
    n = Plan(stock_cfg("yolo11", "n"), 1, 64, 64, fuse_bneck=True, fuse_tail=False)  # same widths one level down
    assert [o["name"] for o in n.ops if o["kind"] == L.OP_BNECK] == ["model.4.m.0", "model.13.m.0", "model.16.m.0", "model.19.m.0"]
    m = Plan(stock_cfg("yolo11", "m"), 1, 64, 64, fuse_bneck=True)  # C3k blocks, e = 1.0: not fused
    assert not any(o["kind"] == L.OP_BNECK for o in m.ops)


def test_yolov5u_plan():
    """YOLOv5u (cfg/models/v5/yolov5.yaml): the 6x6 stride-2 pad-2 stem becomes space-to-depth + a 3x3 conv over 16 channels
    whose packed weights are the module's 6x6 weights re-laid-out (exactly: every 6x6 tap appears once, the padding channels
    are zero); C3 blocks expand to cv1 / cv2 / n x (1x1, 3x3 + shortcut) / cv3; dense FLOPs match the documented model size."""
    from bs_yolo_amd.weights import pack_record
    p = Plan(stock_cfg("yolov5", "s"), 1, 640, 640, merge_c3k=False)
    assert p.ops[0]["kind"] == L.OP_S2D and p.ops[1]["kind"] == L.OP_CONV and (p.ops[1]["ksize"], p.ops[1]["stride"], p.ops[1]["src0"].C) == (3, 1, 16)
    r = p.wrecs["model.0"]
    assert (r.kind, r.cout, r.cin, r.k) == ("first_s2d", 32, 3, 6)
    g = torch.Generator().manual_seed(0)
    sd = {"model.0.conv.weight": torch.randn(32, 3, 6, 6, generator=g), "model.0.conv.bias": torch.randn(32, generator=g)}
    wb, _ = pack_record(sd, r)
    wp = torch.frombuffer(bytearray(wb), dtype=torch.float16).view(128, -1)[:32, :144].float().view(32, 3, 3, 16)  # [co][a][b][(dy,dx,c)]
    x = torch.randn(1, 3, 12, 16, generator=g).half().float()
    s2d = torch.zeros(1, 16, 6, 8)
    for dy in (0, 1):
        for dx in (0, 1):
            s2d[:, (dy * 2 + dx) * 3:(dy * 2 + dx) * 3 + 3] = x[:, :, dy::2, dx::2]
    got = F.conv2d(s2d, wp.permute(0, 3, 1, 2), None, 1, 1)
    want = F.conv2d(x, sd["model.0.conv.weight"].half().float(), None, 2, 2)
    assert torch.allclose(got, want, atol=1e-4)
    assert abs(p.flops / 1e9 - 24.0) < 0.5  # docs/en/models/yolov5.md: YOLOv5su 24.0 GFLOPs
    names = [o["name"] for o in p.ops if o["name"].startswith("model.2.")]
    assert names == ["model.2.cv1", "model.2.cv2", "model.2.m.0.cv1", "model.2.m.0.cv2", "model.2.cv3"]
    m0 = [o for o in p.ops if o["name"].startswith("model.2.m.0.")]
    assert (m0[0]["ksize"], m0[1]["ksize"]) == (1, 3) and m0[1]["res"] is not None  # Bottleneck k = ((1,1),(3,3)) + shortcut
    head_c3 = [o for o in p.ops if o["name"] == "model.13.m.0.cv2"][0]
    assert head_c3["res"] is None  # C3(..., False) in the neck
    assert [o["name"] for o in Plan(stock_cfg("yolov5", "m"), 1, 64, 64).ops if "+" in str(o.get("wkey", ""))][:1] == ["model.2.cv1"]  # merged cv1 + cv2


def test_top_level_dwconv_layer():
    """A `DWConv` layer of a yaml graph (conv.py:224-229) runs on the generic depthwise kernel; c1 != c2 (a grouped conv) is
    refused so the caller keeps the reference forward."""
    cfg = {"nc": 80, "scale": "n", "scales": {"n": [1.0, 1.0, 1024]},
           "backbone": [[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "DWConv", [16, 3, 1]], [-1, 1, "Conv", [32, 3, 2]], [-1, 1, "DWConv", [32, 5, 2]],
                        [-1, 1, "Conv", [64, 3, 2]], [-1, 1, "Conv", [64, 3, 2]]],
           "head": [[[3, 4, 5], 1, "Detect", ["nc"]]]}
    p = Plan(cfg, 1, 64, 64)
    dw = [o for o in p.ops if o["kind"] == L.OP_DWCONV_G]
    assert [(o["ksize"], o["stride"], o["src0"].C) for o in dw] == [(3, 1, 16), (5, 2, 32)]
    assert p.wrecs["model.1"].kind == "dwg" and p.wrecs["model.3"].k == 5
    bad = dict(cfg, backbone=[[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "DWConv", [32, 3, 1]]] + cfg["backbone"][2:])
    with pytest.raises(NotImplementedError):
        Plan(bad, 1, 64, 64)


def test_c3k2_fusion_peephole():
    """A whole C3k2 block with one thin Bottleneck (Cin 64 -> c 32 -> 128: model.2 of YOLO11s, model.4 of YOLO11n) becomes ONE
    OP_C3K2 launch (csrc/c3k2_fused.hip); blocks fed by a Concat (model.16 of YOLO11n) and C3k blocks keep their launches.
    FLOP accounting, parameter records and their order (synth_state_dict draws follow it) are unchanged."""
    for scale, want in (("s", ["model.2"]), ("n", ["model.4"]), ("m", [])):
        a = Plan(stock_cfg("yolo11", scale), 2, 640, 640, fuse_tail=False)
        b = Plan(stock_cfg("yolo11", scale), 2, 640, 640, fuse_tail=True)
        assert a.flops == b.flops and list(a.wrecs) == list(b.wrecs)
        fused = [o for o in b.ops if o["kind"] == L.OP_C3K2]
        assert [o["name"] for o in fused] == want
        assert sum(o.get("mfma_flops", 0) for o in a.ops) == sum(o.get("mfma_flops", 0) for o in b.ops)
        for o in fused:
            assert (o["src0"].C, o["mid_c"], o["dst"].C) == (64, 32, 128) and len(o["wkeys"]) == 4
            assert o["wkeys"] == [o["name"] + sfx for sfx in (".cv1", ".m.0.cv1", ".m.0.cv2", ".cv2")]
            assert len(a.ops) - len(b.ops) == 2  # cv1 conv + fused Bottleneck + cv2 conv -> one op
            assert sum(b.buf_bytes) < sum(a.buf_bytes)  # no concat buffer
    assert L.OP_C3K2 == 18 and L.Op.aux_off.offset % 8 == 0


def test_dwpw_fusion_peephole():
    """YOLO11's class branch units nn.Sequential(DWConv, Conv 1x1) (head.py:49-57) become one OP_DWPW launch where the
    depthwise width is <= 256 (levels 0 and 1 of YOLO11s; the 512-wide level keeps two launches)."""
    a = Plan(stock_cfg("yolo11", "s"), 2, 640, 640, fuse_dwpw=False)
    b = Plan(stock_cfg("yolo11", "s"), 2, 640, 640, fuse_dwpw=True)
    assert a.flops == b.flops and list(a.wrecs) == list(b.wrecs)
    fused = [o["name"] for o in b.ops if o["kind"] == L.OP_DWPW]
    assert fused == ["model.23.cv3.0.0", "model.23.cv3.0.1", "model.23.cv3.1.0", "model.23.cv3.1.1", "model.23.cv3.2.1"]
    assert len(b.ops) == len(a.ops) - len(fused) and L.OP_DWPW == 16
    assert any(o["kind"] == L.OP_DWCONV and o["name"] == "model.23.cv3.2.0.0" for o in b.ops)


def test_plan_consumes_exactly_the_reference_parameters():
    for fam, scale in (("yolo11", "n"), ("yolo11", "x"), ("yolov8", "s"), ("bsyolo11", "n"), ("bsyolo11", "m"), ("yolov5", "n"),
                       ("yolov5", "l")):
        p = Plan(stock_cfg(fam, scale), 2, 96, 64)
        m = R.Model(fam, scale, 80, "detect")
        want = {n for n, _ in m.param_specs() if not n.endswith("dfl.conv.weight")}
        assert {k for r in p.wrecs.values() for k in record_keys(r)} == want
        # every view stays inside its buffer and respects the kernels' alignment rules
        for o in p.ops:
            for key in ("src0", "src1", "dst", "res"):
                t = o.get(key)
                if t is None or t.buf >= L.BSY_EXT_BASE:
                    continue
                assert t.coff + t.C <= t.ld
                assert t.coff % (4 if t.f32 else 8) == 0
                hs, ws = (t.H // 2, t.W // 2) if t.up else (t.H, t.W)
                if o["kind"] == L.OP_ELA and key == "res":
                    continue  # ELA's f32 scratch: sized by the op, not by a map shape
                assert p.buf_bytes[t.buf] == p.B * hs * ws * t.ld * (4 if t.f32 else 2)


@pytest.mark.parametrize("fam,width", [("yolo11", 0.1875), ("yolov8", 0.1875), ("yolov8", 0.3125), ("yolov5", 0.3125), ("yolov5", 0.1875)])
def test_c2f_chunks_that_are_not_multiples_of_8_are_zero_padded_pieces(fam, width):
    """A width multiple like 0.1875 gives C2f / C3k2 chunk widths of 12 channels (tasks.py:1016, block.py:3295-3317), 0.3125 gives 20;
    YOLOv5u's C3 then has halves of 12 / 20 channels (the C3k path).  The fp16 kernels read 8-channel pieces, so the plan carries every chunk on the next multiple of 8 as a
    zero-padded piece (plan.py T.cmap): the conv that writes a piece has zero weight rows and bias at the padding, the conv that reads it zero
    weight columns.  Checked on the packed matrices, against the module's own folded weights."""
    R.SCALES[fam] = dict(R.SCALES[fam], t=(0.5, width, 1024))
    try:
        cfg = dict(stock_cfg(fam, "n"), scale="t", scales={"t": [0.5, width, 1024]})
        p = Plan(cfg, 2, 96, 64)
        m = R.Model(fam, "t", 80, "detect")
        want = {n for n, _ in m.param_specs() if not n.endswith("dfl.conv.weight")}
        assert {k for r in p.wrecs.values() for k in record_keys(r)} == want
        sd = synth_state_dict(p, 3)
        for n_, shape in m.param_specs():  # the synthetic parameters have the MODULE's shapes, not the padded ops'
            if n_ in sd:
                assert tuple(sd[n_].shape) == tuple(shape), (n_, tuple(sd[n_].shape), tuple(shape))
        blob = pack_plan_weights(p, sd)
        padded = 0
        for o in p.ops:
            if o["kind"] != L.OP_CONV:
                continue
            srcs = [t for t in (o["src0"], o.get("src1")) if t is not None]
            dst = o["dst"]
            if dst.cmap is None and all(t.cmap is None for t in srcs):
                continue
            padded += 1
            r = p.wrecs[o["wkey"]]
            k, cin, cout = o["ksize"], sum(t.C for t in srcs), dst.C
            cp, kp = (cout + 127) // 128 * 128, (k * k * cin + 31) // 32 * 32
            wp = torch.frombuffer(bytearray(blob[r.w_off:r.w_off + cp * kp * 2]), dtype=torch.float16).view(cp, kp).float()
            bp = torch.frombuffer(bytearray(blob[r.b_off:r.b_off + cp * 4]), dtype=torch.float32)
            if r.kind == "conv2":
                (w0, b0), (w1, b1) = fold_conv_bn(sd, r.name), fold_conv_bn(sd, r.post)
                wm, bm = torch.cat([w0, w1]), torch.cat([b0, b1])
            else:
                wm, bm = fold_conv_bn(sd, r.name)
            rows = list(dst.cmap) if dst.cmap is not None else list(range(cout))
            cols, base = [], 0
            for t in srcs:
                cols += [base + v if v >= 0 else -1 for v in (t.cmap if t.cmap is not None else range(t.C))]
                base += t.real
            assert wm.shape[0] == sum(v >= 0 for v in rows) and wm.shape[1] == base, (o["name"], tuple(wm.shape), base)
            wk = wp[:cout, :k * k * cin].view(cout, k * k, cin)
            for i, ri in enumerate(rows):
                if ri < 0:
                    assert torch.all(wk[i] == 0) and bp[i] == 0, o["name"]
                    continue
                assert abs(float(bp[i] - bm[ri])) < 1e-6
                for j, cj in enumerate(cols):
                    got = wk[i, :, j]
                    if cj < 0:
                        assert torch.all(got == 0), (o["name"], i, j)
                    else:
                        assert torch.equal(got, wm[ri, cj].reshape(-1).half().float()), (o["name"], i, j)
        assert padded >= 3
        for o in p.ops:  # pieces stay aligned
            for key in ("src0", "src1", "dst", "res"):
                t = o.get(key)
                if t is not None and t.buf < L.BSY_EXT_BASE and not t.f32:
                    assert t.coff % 8 == 0 and t.C % 8 == 0 or o["kind"] not in (L.OP_CONV, L.OP_BNECK), (o["name"], key, t)
    finally:
        R.SCALES[fam].pop("t", None)


def test_plan_says_which_precisions_run_a_width():
    """YOLO11 at a width multiple of 0.3125: C2PSA's attention heads are 40 / 80 channels wide (block.py:4253-4258), which the fp16 attention
    kernel does not take -- the plan says so when it is built (plugin.graph_support relies on that), the fp32-storage modes build."""
    cfg = dict(stock_cfg("yolo11", "n"), scale="t", scales={"t": [0.5, 0.3125, 1024]})
    with pytest.raises(NotImplementedError, match="attention heads"):
        Plan(cfg, 1, 64, 64)
    Plan(cfg, 1, 64, 64, precision="fp32")
    Plan(cfg, 1, 64, 64, precision="fp32x")
    Plan(dict(cfg, scales={"t": [0.5, 0.1875, 1024]}), 1, 64, 64)  # 48 / 96: on the fp16 path


def test_plan_rejects_unsupported_graphs():
    cfg = stock_cfg("yolo11", "n")
    cfg["backbone"] = list(cfg["backbone"])
    cfg["backbone"][2] = [-1, 2, "C3k2_LRSA", [256, False, 0.25]]  # one of the fork's dead experiments: not accelerated
    with pytest.raises(NotImplementedError):
        Plan(cfg, 1, 64, 64)
    cfg = stock_cfg("yolo11", "n")
    cfg["head"] = list(cfg["head"])
    cfg["head"][-1] = [[16, 19, 22], 1, "Pose", ["nc", [17, 3]]]  # other task heads stay on the reference
    with pytest.raises(NotImplementedError):
        Plan(cfg, 1, 64, 64)


def _edited(family, size, edits=None, nc=80, task="detect", append=None, **top):
    """A stock graph with the layers `edits` names ({index over backbone + head: layer}) replaced, `append` put behind the last one and
    the top-level keys `top` set (None: removed)."""
    cfg = stock_cfg(family, size, nc, task, kpt_shape=(17, 3) if task == "pose" else None)
    nb = len(cfg["backbone"])
    layers = list(cfg["backbone"]) + list(cfg["head"]) + ([append] if append else [])
    for i, layer in (edits or {}).items():
        layers[i] = layer
    cfg["backbone"], cfg["head"] = layers[:nb], layers[nb:]
    for k, v in top.items():
        cfg.pop(k) if v is None else cfg.update({k: v})
    return cfg


_T11 = dict(scale="t", scales={"t": [0.5, 0.1875, 1024]})  # YOLO11 at a width multiple of 0.1875: layer 1 is 24 channels wide
# (id, () -> graph, Plan keywords): one row per `raise NotImplementedError` of the graph walk
PLAN_REFUSALS = [
    ("zeropad-not-before-pool", lambda: _edited("yolov3-tiny", None, {12: [-1, 1, "Conv", [512, 3, 1]]}), {}),
    ("zeropad-arguments", lambda: _edited("yolov3-tiny", None, {11: [-1, 1, "nn.ZeroPad2d", [[1, 1, 1, 1]]]}), {}),
    ("zeropad-second-reader", lambda: _edited("yolov3-tiny", None, {14: [11, 1, "Conv", [256, 1, 1]]}), {}),
    ("relu-module", lambda: _edited("yolov6", "n", {13: [-1, 1, "C2f", [256]]}), {}),
    ("conv-image-repeated", lambda: _edited("yolov6", "n", {0: [-1, 6, "Conv", [64, 3, 2]]}), {}),
    ("conv-chain-width", lambda: _edited("yolov6", "n", {2: [-1, 6, "Conv", [256, 3, 1]]}), {}),
    ("conv-chain-padding", lambda: _edited("yolov6", "n", {2: [-1, 6, "Conv", [128, 3, 1, 0]]}), {}),
    ("conv-image-ksp", lambda: _edited("yolo11", "n", {0: [-1, 1, "Conv", [64, 5, 2]]}), {}),
    ("conv-padding", lambda: _edited("yolo11", "n", {1: [-1, 1, "Conv", [128, 3, 2, 0]]}), {}),
    ("ghostconv-image", lambda: _edited("yolov8-ghost", "n", {0: [-1, 1, "GhostConv", [64, 3, 2]]}), {}),
    ("ghostconv-groups", lambda: _edited("yolov8-ghost", "n", {1: [-1, 1, "GhostConv", [128, 3, 2, 2]]}), {}),
    ("ghostconv-halves-12", lambda: _edited("yolov8-ghost", "n", {1: [-1, 1, "GhostConv", [96, 3, 2]]}), {}),
    ("dwconv-widths", lambda: _edited("yolo11", "n", {1: [-1, 1, "DWConv", [128, 3, 2]]}), {}),
    ("spp-k", lambda: _edited("yolov3-spp", None, {12: [-1, 1, "SPP", [512, [5, 9]]]}), {}),
    ("spp-hidden-width", lambda: _edited("yolo11", "n", {2: [-1, 1, "SPP", [256, [5, 9, 13]]]}, **_T11), {}),
    ("bottleneck-groups", lambda: _edited("yolov3", None, {2: [-1, 1, "Bottleneck", [64, True, 2]]}), {}),
    ("bottleneck-chain-width", lambda: _edited("yolov3", None, {4: [-1, 2, "Bottleneck", [256]]}), {}),
    ("sppelan-k", lambda: _edited("yolov9", "c", {9: [-1, 1, "SPPELAN", [512, 256, 3]]}), {}),
    ("sppelan-hidden-width", lambda: _edited("yolov9", "c", {9: [-1, 1, "SPPELAN", [512, 100]]}), {}),
    ("maxpool-arguments", lambda: _edited("yolov3-tiny", None, {1: [-1, 1, "nn.MaxPool2d", [3, 2, 1]]}), {}),
    ("deconv-on-concat", lambda: _edited("yolov6", "n", {13: [-1, 1, "nn.ConvTranspose2d", [256, 2, 2, 0]]}), {}),
    ("deconv-arguments", lambda: _edited("yolov6", "n", {11: [-1, 1, "nn.ConvTranspose2d", [256, 3, 2, 0]]}), {}),
    ("obb-ne", lambda: _edited("yolo11", "n", {23: [[16, 19, 22], 1, "OBB", ["nc", 2]]}, task="obb"), {}),
    ("pose-spelled-out", lambda: _edited("yolo11", "n", {23: [[16, 19, 22], 1, "Pose", ["nc", [17, 3]]]}, 1, "pose"), {}),
    ("pose-no-kpt-shape", lambda: _edited("yolo11", "n", None, 1, "pose", kpt_shape=None), {}),
    ("pose-kpt-shape-range", lambda: _edited("yolo11", "n", None, 1, "pose", kpt_shape=[17, 4]), {}),
    ("v10detect-not-last", lambda: _edited("yolov10", "n", append=[-1, 1, "Conv", [64, 1, 1]]), {}),
    ("classify-list", lambda: _edited("yolo11", "n", {10: [[-1, 8], 1, "Classify", ["nc"]]}, 1000, "classify"), {}),
    ("classify-not-last", lambda: _edited("yolo11", "n", None, 1000, "classify", append=[-1, 1, "Conv", [64, 1, 1]]), {}),
    ("classify-arguments", lambda: _edited("yolo11", "n", {10: [-1, 1, "Classify", ["nc", 3]]}, 1000, "classify"), {}),
    ("unknown-module", lambda: _edited("yolo11", "n", {2: [-1, 2, "C3k2_LRSA", [256, False, 0.25]]}), {}),
]


@pytest.mark.parametrize("cid,graph,kw", PLAN_REFUSALS, ids=[r[0] for r in PLAN_REFUSALS])
def test_graph_walk_refusals_are_the_recorded_ones(cid, graph, kw, snap):
    """Every `raise NotImplementedError` of Plan._build, reached through a stock graph with one layer (or one top-level key) edited:
    the exception's exact type and its whole message equal what tests/golden/plan_refusals.json recorded before the walk was
    split into per-module lowerings (the plan snapshots see only graphs that build).  Two sites have no row, because no graph reaches them:
      * "nn.ZeroPad2d is accelerated only in front of nn.MaxPool2d [2, 1, 0] (model.i is ...)", the gate at the top of the walk: the
        ZeroPad2d layer itself has by then refused every graph whose next layer is not that pool reading it alone, and every graph in
        which another layer names it in `f`, so the layer that receives its output is always the pool;
      * "... lowers to op ... which has no ReLU", the post-check on RELU_KINDS: of RELU_MODULES only Detect can emit another kind
        (DWCONV / DWPW of the light class branch), and it does so only where a C3k2 has cleared `legacy` -- C3k2 is not in
        RELU_MODULES, so a ReLU graph is refused at that layer first."""
    want = json.loads((GOLDEN / "plan_refusals.json").read_text())
    assert sorted(want) == sorted(r[0] for r in PLAN_REFUSALS)
    with pytest.raises(NotImplementedError) as e:
        Plan(graph(), 1, 64, 64, **kw)
    assert {"type": type(e.value).__name__, "message": str(e.value)} == want[cid]


def test_segment_plan_matches_reference_work():
    """YOLOv8l-seg @640 (BASELINE config 4): 210.4 GFLOP/image, protos at (160, 160)."""
    p = Plan(stock_cfg("yolov8", "l", 80, "segment"), 1, 640, 640)
    assert abs(p.flops / 1e9 - 210.4) < 0.5
    assert p.meta["proto_hw"] == (160, 160) and p.meta["nm"] == 32 and p.meta["A"] == 8400
    m = R.Model("yolov8", "l", 80, "segment")
    want = {n for n, _ in m.param_specs() if not n.endswith("dfl.conv.weight")}
    assert {k for r in p.wrecs.values() for k in record_keys(r)} == want


def test_fold_matches_reference_known_answer():
    z = np.load(GOLDEN / "modules.npz")
    c = R.Conv("m", 8, 12, 3, 1)
    sd = {n: R.synth_param(n, s, 11) for n, s in c.specs()}
    w, b = fold_conv_bn(sd, "m")
    np.testing.assert_allclose(w.numpy(), z["fuse.w"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(b.numpy(), z["fuse.b"], rtol=1e-6, atol=1e-7)
    # an already-fused state_dict (what the model holds after BaseModel.fuse) gives the same
    fused = {"m.conv.weight": torch.from_numpy(z["fuse.w"]), "m.conv.bias": torch.from_numpy(z["fuse.b"])}
    w2, b2 = fold_conv_bn(fused, "m")
    assert torch.equal(w2, fused["m.conv.weight"]) and torch.equal(b2, fused["m.conv.bias"])


def test_packed_weight_layout_is_the_gemm_the_kernel_runs():
    """[CoutPad][Kpad] with K = (kh, kw, cin): im2col rows in the kernel's K order times the packed matrix == conv2d."""
    from bs_yolo_amd.plan import WRec
    g = torch.Generator().manual_seed(0)
    cin, cout, k = 16, 24, 3
    sd = {"c.conv.weight": torch.randn(cout, cin, k, k, generator=g), "c.conv.bias": torch.randn(cout, generator=g)}
    wb, bb = pack_record(sd, WRec("c", "conv", cout, cin, k))
    wp = torch.frombuffer(bytearray(wb), dtype=torch.float16).view(128, 160).float()
    bp = torch.frombuffer(bytearray(bb), dtype=torch.float32)
    assert torch.all(wp[cout:] == 0) and torch.all(wp[:, 144:] == 0) and torch.all(bp[cout:] == 0)
    x = torch.randn(1, cin, 6, 5, generator=g)
    xp = F.pad(x, (1, 1, 1, 1)).permute(0, 2, 3, 1)  # NHWC
    rows = []
    for oh in range(6):
        for ow in range(5):
            rows.append(torch.cat([xp[0, oh + kh, ow + kw] for kh in range(3) for kw in range(3)]))
    got = torch.stack(rows) @ wp[:cout, :144].t() + bp[:cout]
    ref = F.conv2d(x, sd["c.conv.weight"].half().float(), sd["c.conv.bias"], 1, 1)[0].permute(1, 2, 0).reshape(30, cout)
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=1e-4)


def test_qkv_permutation_groups_heads():
    p = Plan(stock_cfg("yolo11", "s"), 1, 64, 64)
    r = p.wrecs["model.10.m.0.attn.qkv"]
    nh, kd, hd = 4, 32, 64
    assert sorted(r.perm) == list(range(nh * (2 * kd + hd)))
    assert r.perm[:kd] == list(range(0, kd))                       # head 0 q
    assert r.perm[kd:2 * kd] == list(range(128, 128 + kd))         # head 1 q (reference row 1*128 + 0..31)
    assert r.perm[nh * kd] == kd                                   # first k row of head 0
    assert r.perm[2 * nh * kd] == 2 * kd                           # first v row of head 0
    assert r.perm[2 * nh * kd + hd] == 128 + 2 * kd                # first v row of head 1


def test_pack_blob_offsets_are_aligned_and_disjoint():
    p = Plan(stock_cfg("yolo11", "n"), 1, 64, 64)
    blob = pack_plan_weights(p, synth_state_dict(p, 0))
    spans = []
    for r in p.wrecs.values():
        assert r.w_off % 256 == 0 and r.b_off % 256 == 0 and 0 <= r.w_off < r.b_off < len(blob)
        spans.append((r.w_off, r.b_off))
    assert spans == sorted(spans)


# ---- the device layouts and the channel step of weights.py, element by element against expectations written here -------------------
def test_dense_f16_layout_element_by_element():
    """fp16 [CoutPad][Kpad] with K order (kh, kw, cin) and zero padding; an image conv gets a zero 4th input channel; the padded dims
    are the library's (bsy_conv_packed_dims)."""
    import ctypes as C
    from bs_yolo_amd.weights import dense_f16
    cout, cin, k = 5, 8, 3
    w = torch.arange(cout * cin * k * k, dtype=torch.float32).view(cout, cin, k, k)  # integers below 2048: exact in fp16
    b = torch.arange(cout, dtype=torch.float32) + 0.5
    wp, bp = dense_f16(w, b)
    assert wp.dtype == torch.float16 and tuple(wp.shape) == (128, 96) and bp.dtype == torch.float32 and tuple(bp.shape) == (128,)
    for co in range(cout):
        for kh in range(k):
            for kw in range(k):
                for ci in range(cin):
                    assert float(wp[co, (kh * 3 + kw) * cin + ci]) == float(w[co, ci, kh, kw])
    assert torch.all(wp[cout:] == 0) and torch.all(wp[:, k * k * cin:] == 0)
    assert torch.equal(bp[:cout], b) and torch.all(bp[cout:] == 0)
    w3 = 1 + torch.arange(cout * 3 * k * k, dtype=torch.float32).view(cout, 3, k, k)  # the image case: cin 3 -> 4
    wp, bp = dense_f16(w3)
    assert tuple(wp.shape) == (128, 64) and torch.all(bp == 0)
    for co in range(cout):
        for tap in range(k * k):
            for ci in range(4):
                assert float(wp[co, tap * 4 + ci]) == (float(w3[co, ci, tap // 3, tap % 3]) if ci < 3 else 0.0)
    assert torch.all(wp[cout:] == 0) and torch.all(wp[:, k * k * 4:] == 0)
    cp, kp = C.c_int(), C.c_int()
    for c2 in (5, 128, 129):
        for c1 in (3, 8, 40):
            for kk in (1, 3):
                assert L.lib.bsy_conv_packed_dims(c2, c1, kk, C.byref(cp), C.byref(kp)) == 0
                wp, bp = dense_f16(torch.zeros(c2, c1, kk, kk))
                assert tuple(wp.shape) == (cp.value, kp.value) and tuple(bp.shape) == (cp.value,), (c2, c1, kk)


def test_dense_f32_and_split_layout_element_by_element():
    """f32 [K][Cout], K order (kh, kw, cin), bias as it is; the fp32x mode's f16 planes hi + lo give w back to 2^-22 relative -- hi
    keeps 11 bits, lo 11 more of the exact remainder, and with |w| >= 2^-3 lo stays clear of the f16 subnormals' absolute 2^-25 --
    and sit in the record where csrc/op_args.h build_conv32 looks for them: each part padded to 256 bytes."""
    from bs_yolo_amd.plan import WRec
    from bs_yolo_amd.weights import dense_f32
    g = torch.Generator().manual_seed(5)
    cout, cin, k = 5, 8, 3
    K = k * k * cin
    w = (0.125 + 3.875 * torch.rand(cout, cin, k, k, generator=g)) * (1 - 2 * torch.randint(0, 2, (cout, cin, k, k), generator=g))
    b = torch.randn(cout, generator=g)
    (m,), bb = dense_f32(w, b)
    assert m.dtype == torch.float32 and tuple(m.shape) == (K, cout) and torch.equal(bb, b)
    for co in range(cout):
        for kh in range(k):
            for kw in range(k):
                for ci in range(cin):
                    assert float(m[(kh * 3 + kw) * cin + ci, co]) == float(w[co, ci, kh, kw])
    (m2, hi, lo), _ = dense_f32(w, b, split=True)
    assert torch.equal(m2, m) and hi.dtype == lo.dtype == torch.float16 and tuple(hi.shape) == tuple(lo.shape) == (cout, 96)
    assert torch.all(hi[:, K:] == 0) and torch.all(lo[:, K:] == 0)
    for co in range(cout):
        for kk in range(K):
            want = float(w[co, kk % cin, kk // cin // 3, kk // cin % 3])
            assert abs(float(hi[co, kk]) + float(lo[co, kk]) - want) <= 2.0 ** -22 * abs(want)
    wb, bias = pack_record({"c.weight": w, "c.bias": b}, WRec("c", "plain", cout, cin, k), f32=True, split=True)
    align256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    hi_off = align256(K * cout * 4)  # op_args.h: hi_off = align256(K * Cout * 4), lo_off = hi_off + align256(Cout * kpad * 2)
    lo_off = hi_off + align256(cout * 96 * 2)
    assert (hi_off, lo_off, len(wb)) == (1536, 2560, 2560 + cout * 96 * 2)
    assert wb[:K * cout * 4] == m.numpy().tobytes() and wb[hi_off:hi_off + cout * 96 * 2] == hi.numpy().tobytes()
    assert wb[lo_off:] == lo.numpy().tobytes() and bias == b.numpy().tobytes()


def test_depthwise_layout_element_by_element():
    """f32 [kh*kw][C], taps in (kh, kw) order, channels adjacent: a 3x3 and a 1x5 strip."""
    from bs_yolo_amd.weights import depthwise
    g = torch.Generator().manual_seed(6)
    for kh, kw in ((3, 3), (1, 5)):
        w, b = torch.randn(8, 1, kh, kw, generator=g), torch.randn(8, generator=g)
        wp, bp = depthwise(w, b)
        assert wp.dtype == torch.float32 and tuple(wp.shape) == (kh * kw, 8) and wp.is_contiguous() and torch.equal(bp, b)
        for c in range(8):
            for i in range(kh):
                for j in range(kw):
                    assert float(wp[i * kw + j, c]) == float(w[c, 0, i, j])


def test_channel_step_puts_zero_rows_columns_and_biases_where_the_maps_say():
    from bs_yolo_amd.plan import WRec
    from bs_yolo_amd.weights import op_channels
    g = torch.Generator().manual_seed(7)
    w, b = torch.randn(3, 5, 3, 3, generator=g), torch.randn(3, generator=g)
    rows, cols = [2, -1, 0, 1], [-1, 4, 0, 1, 2, 3]
    w2, b2 = op_channels(WRec("c", "conv", 4, 6, 3, rows=rows, cols=cols), w, b)
    assert tuple(w2.shape) == (4, 6, 3, 3) and tuple(b2.shape) == (4,)
    for i, ri in enumerate(rows):
        assert float(b2[i]) == (float(b[ri]) if ri >= 0 else 0.0)
        for j, cj in enumerate(cols):
            assert torch.equal(w2[i, j], w[ri, cj] if ri >= 0 and cj >= 0 else torch.zeros(3, 3)), (i, j)
    w2, b2 = op_channels(WRec("c", "conv", 8, 8, 3, real_cout=3, real_cin=5), w, b)
    assert tuple(w2.shape) == (8, 8, 3, 3) and torch.equal(w2[:3, :5], w) and torch.equal(b2[:3], b)
    assert torch.all(w2[3:] == 0) and torch.all(w2[:, 5:] == 0) and torch.all(b2[3:] == 0)


def test_letterbox_geometry_matches_reference_golden():
    z = np.load(GOLDEN / "letterbox.npz")
    for c in json.loads(str(z["cases"])):
        kw = dict(c["kw"])
        new_shape = tuple(kw.pop("new_shape"))
        H2, W2, nw, nh, left, top, _ = LetterBox(new_shape, **kw).geometry(tuple(c["shape"]))
        assert [H2, W2, 3] == c["out_shape"], c
        assert [top, top + nh, left, left + nw] == c["box"], c


def test_shard_bounds():
    assert [e - s for s, e in shard_bounds(70, 8)] == [9, 9, 9, 9, 9, 9, 8, 8]  # SAHI config 5
    assert [e - s for s, e in shard_bounds(256, 8)] == [32] * 8                 # config 3
    b = shard_bounds(5, 8)
    assert b[0] == (0, 1) and b[-1] == (5, 5) and sum(e - s for s, e in b) == 5


WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from bs_yolo_amd.parallel import gather_detections, gather_detections_async, shard_bounds
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + sys.argv[2], rank=rank, world_size=world)
n_items = int(sys.argv[3])
s, e = shard_bounds(n_items, world)[rank]
det = torch.zeros(e - s, 4, 6)
counts = torch.zeros(e - s, dtype=torch.int32)
for i in range(s, e):
    det[i - s, :, 0] = i          # item id in column 0
    det[i - s, :, 4] = rank
    counts[i - s] = i % 5
d, c = gather_detections(det, counts, n_items)
assert d.shape == (n_items, 4, 6) and c.shape == (n_items,)
assert torch.equal(d[:, 0, 0], torch.arange(n_items, dtype=torch.float32)), d[:, 0, 0]
assert torch.equal(c, (torch.arange(n_items) % 5).to(torch.int32))
exp_rank = torch.cat([torch.full((b - a,), float(k)) for k, (a, b) in enumerate(shard_bounds(n_items, world))])
assert torch.equal(d[:, 0, 4], exp_rank)
# two gathers in flight (bench.py overlaps the gather of step k with the forward of step k+1)
h1 = gather_detections_async(det, counts, n_items)
h2 = gather_detections_async(det + 1, counts + 1, n_items)
d1, c1 = h1.wait()
d2, c2 = h2.wait()
assert torch.equal(d1, d) and torch.equal(c1, c) and torch.equal(d2, d + 1) and torch.equal(c2, c + 1)
assert c2.dtype == torch.int32 and d2.shape == (n_items, 4, 6)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
'''


@pytest.mark.parametrize("n_items", [8, 7])
def test_gather_detections_gloo_world2(tmp_path, n_items):
    """world_size-2 rehearsal of the N>1 path on CPU (gloo): even and uneven shards come back in global order."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    port = str(29500 + os.getpid() % 1000 + n_items)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1")
        procs.append(subprocess.Popen([sys.executable, str(script), str(ROOT), port, str(n_items)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=120)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o


def decode_state_dict(z, prefix, codes):
    """tests/golden/make_fixtures.py encode_state_dict, inverted: a recorded reference state_dict, bit for bit."""
    sd = {}
    for i, (k, shape, dtype, code) in enumerate(codes):
        if code == "raw":
            sd[k] = torch.from_numpy(z[f"{prefix}_{i}"].copy())
        else:
            t = R.synth_param(k, shape, 0)
            if code == "scaled":
                t = t * torch.from_numpy(z[f"{prefix}_{i}"].copy()).view(-1, *[1] * (len(shape) - 1))
            sd[k] = t.to(getattr(torch, dtype))
        assert list(sd[k].shape) == shape and str(sd[k].dtype) == "torch." + dtype, k
    return sd


F16_KINDS = ("conv", "conv2", "plain", "first", "first_s2d", "deconv")  # weights.pack_record: fp16 weights in the fp16 layout


def blob_values(plan, blob):
    """A packed fp16-mode weight blob -> {record: (weights, biases)} as the values it stores (fp16 dense-conv weights, fp32 the
    rest; each with its zero padding)."""
    recs = list(plan.wrecs.items())
    ends = [r.w_off for _, r in recs[1:]] + [len(blob)]
    return {k: (np.frombuffer(blob[r.w_off:r.b_off], np.float16 if r.kind in F16_KINDS else np.float32).astype(np.float32),
                np.frombuffer(blob[r.b_off:e], np.float32))
            for (k, r), e in zip(recs, ends)}


def test_plugin_reads_a_live_reference_model():
    """accelerate()'s inputs -- model.yaml + state_dict() of a live reference DetectionModel, before and after
    BaseModel.fuse() -- produce the same packed weights as the oracle's parameters.  The live model's yaml dict, BatchNorm eps
    and both state_dicts are recorded in tests/golden/live_model.npz (make_fixtures.py live_model_fixture).  The fused weights
    are compared as the values the blob stores (blob_values): their BatchNorm was folded by a different sequence of fp32
    operations, which may round differently in the last place."""
    from bs_yolo_amd.plugin import cfg_of, model_bn_eps
    z = np.load(GOLDEN / "live_model.npz", allow_pickle=False)

    def live(tag):
        meta = json.loads(str(z[f"{tag}_meta"]))
        m = torch.nn.Module()  # what cfg_of / model_bn_eps read of the model: .yaml and its BatchNorm modules
        m.yaml = meta["yaml"]
        m.bn = torch.nn.BatchNorm2d(1, eps=meta["bn_eps"])
        return m, decode_state_dict(z, f"{tag}_unfused", meta["unfused"]), decode_state_dict(z, f"{tag}_fused", meta["fused"])

    m, sd, fused = live("yolo11n")
    cfg = cfg_of(m)
    assert abs(model_bn_eps(m) - 1e-3) < 1e-12
    p1 = Plan(cfg, 1, 64, 64); b1 = pack_plan_weights(p1, sd, model_bn_eps(m))
    po = Plan(cfg, 1, 64, 64); bo = pack_plan_weights(po, R.synth_params(R.Model("yolo11", "n", 80, "detect"), 0))
    assert b1 == bo, "unfused reference state_dict packs differently from the oracle parameters"
    p2 = Plan(cfg, 1, 64, 64); b2 = pack_plan_weights(p2, fused)
    assert len(b1) == len(b2), "fused state_dict packs differently"
    v1, v2 = blob_values(p1, b1), blob_values(p2, b2)
    assert list(v1) == list(v2)
    for k in v1:
        for x1, x2 in zip(v1[k], v2[k]):
            assert x1.shape == x2.shape and np.abs(x1 - x2).max(initial=0.0) < 2e-3, f"fused state_dict packs {k} differently"
    # the BS-YOLO graph itself (cfg/models/11/yolo11.yaml, nc = 12): the live model's yaml + state_dict pack exactly like the
    # oracle's parameters, un-fused and fused
    mb, sdb, fusedb = live("bsyolo11")
    cb = cfg_of(mb)
    assert cb["nc"] == 12
    q1 = Plan(cb, 1, 64, 64); c1 = pack_plan_weights(q1, sdb, model_bn_eps(mb))
    qo = Plan(cb, 1, 64, 64); co = pack_plan_weights(qo, R.synth_params(R.Model("bsyolo11", "n", 12, "detect"), 0))
    assert c1 == co, "BS-YOLO: reference state_dict packs differently from the oracle parameters"
    assert q1.wrecs["model.15"].coef == qo.wrecs["model.15"].coef and q1.wrecs["model.15"].coef[0] > 0
    q2 = Plan(cb, 1, 64, 64); c2 = pack_plan_weights(q2, fusedb)
    assert len(c1) == len(c2)


# ---- plan snapshots: what the planner hands to the device, byte for byte (tools/plan_snapshot.py) ------------------------------
def _plan_snapshot():
    sys.path.insert(0, str(ROOT / "tools"))
    import plan_snapshot
    return plan_snapshot


@pytest.fixture
def snap(monkeypatch):
    """tools/plan_snapshot.py, with everything a Plan reads from the environment unset."""
    S = _plan_snapshot()
    for k in S.PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    return S


def test_plans_are_the_recorded_ones(snap):
    """Op array, buffer table, weight records (their blob offsets, the blob's length) and both arena layouts of every case of tools/plan_snapshot.py equal the
    committed digests (tests/golden/plan_snapshots.json): a host-side change of the planner that is meant to leave the device's work
    alone leaves these alone.  python tools/plan_snapshot.py --dump DIR at two commits shows what moved."""
    want = json.loads(snap.FIXTURE.read_text())
    cases = snap.cases()
    assert sorted(want) == sorted(cid for cid, _, _ in cases) and len(cases) >= 117 + 16 + 135 + 3
    got = {cid: snap.snapshot(build, pack)[0] for cid, build, pack in cases}
    assert not {cid: (got[cid], want[cid]) for cid in want if got[cid] != want[cid]}


def test_plan_switches_read_their_environment_variable(snap, monkeypatch):
    """BSY_FUSE_X=0 (BSY_MERGE_C3K=0) builds the plan of keyword X=False, on graphs where every switch changes something; BSY_LANES
    forces the head lanes off / on at a size where they are on by default; an unknown switch is a TypeError."""
    from bs_yolo_amd.plan import SWITCHES
    assert snap.SWITCH_ENV == SWITCHES  # (the tool keeps a copy of the table so that it also runs on a tree without one)
    digest = lambda build: snap.snapshot(build, False)[0]["digest"]  # noqa: E731
    graphs = [(stock_cfg("yolo11", "s"), 2, 64, 96), (stock_cfg("yolo11", "m", 80, "segment"), 2, 64, 96), (stock_cfg("bsyolo11", "s"), 2, 64, 96)]
    for name, env in snap.SWITCH_ENV.items():
        moved = 0
        for g in graphs:
            on, off = digest(lambda: Plan(*g)), digest(lambda: Plan(*g, **{name: False}))
            moved += on != off
            monkeypatch.setenv(env, "0")
            assert digest(lambda: Plan(*g)) == off, (name, env)
            assert digest(lambda: Plan(*g, **{name: True})) == on, (name, env)  # the argument wins over the variable
            monkeypatch.delenv(env)
        assert moved, f"{name} changes none of the graphs"
    big = (stock_cfg("yolo11", "s"), 16, 640, 640)
    lanes = lambda p: sum(1 for o in p.ops if o.get("lane", 0) > 0)  # noqa: E731
    assert lanes(Plan(*big)) == 14 and lanes(Plan(*big, lanes=False)) == 0
    assert sum(1 for o in Plan(stock_cfg("yolo11", "s"), 8, 640, 640, latency=True).ops if o.get("ksplit")) == 2
    for value, kw in (("0", False), ("1", True)):
        want = digest(lambda: Plan(*big, lanes=kw))
        monkeypatch.setenv("BSY_LANES", value)
        assert digest(lambda: Plan(*big)) == want
        monkeypatch.delenv("BSY_LANES")
    with pytest.raises(TypeError, match="fuse_stemm"):
        Plan(*graphs[0], fuse_stemm=False)


def test_emitter_refuses_unknown_fields():
    """c_ops() reads every field with a default, so a misspelt key would serialise as zero: Plan._emit asserts on it instead; it fills
    the lane and the map sizes itself, and lets only the kinds the engine forks for onto a side lane."""
    p = Plan(stock_cfg("yolo11", "n"), 1, 64, 64)
    with pytest.raises(AssertionError, match="strid"):
        p._emit(L.OP_COPY, "x", src0=p.ops[1]["dst"], dst=p.ops[1]["dst"], strid=2)
    n, fl = len(p.ops), p.flops
    with pytest.raises(AssertionError, match="flops"):  # positional: a keyword of that name would be taken for a field
        p._emit(L.OP_COPY, "x", src0=p.ops[1]["dst"], dst=p.ops[1]["dst"], flops=7)
    o = p._emit(L.OP_COPY, "x", 7, src0=p.ops[1]["src0"], dst=p.ops[1]["dst"], mfma_flops=0)
    assert p.ops[n] is o and len(p.ops) == n + 1 and p.flops == fl + 7 and o["lane"] == 0 and "mfma_flops" not in o
    assert (o["H"], o["W"], o["OH"], o["OW"]) == (p.ops[1]["H"], p.ops[1]["W"], p.ops[1]["OH"], p.ops[1]["OW"])
    assert all("lane" in o for o in p.ops)
    p._lane = 1
    with pytest.raises(AssertionError, match="side lane"):
        p._emit(L.OP_COPY, "y", src0=p.ops[1]["dst"], dst=p.ops[1]["dst"])


def test_max_view_elems_counts_source_destination_and_residual_views():
    """Plan.max_view_elems (the engine's batch-split threshold): the largest one-image view among src0 / src1 / dst / res, an upsampled
    source at its stored size; the per-level lists (box / cls / msk, the split-K slabs among them) are not counted."""
    for cfg, hw in ((stock_cfg("yolo11", "s"), (640, 640)), (stock_cfg("yolov8", "l", 80, "segment"), (96, 64)), (stock_cfg("bsyolo11", "s"), (64, 96))):
        p = Plan(cfg, 1, *hw)
        want = 1
        for o in p.ops:
            for k in ("src0", "src1", "dst", "res"):
                t = o.get(k)
                if t is not None and t.buf < L.BSY_EXT_BASE:
                    hs, ws = (t.H // 2, t.W // 2) if t.up else (t.H, t.W)
                    want = max(want, hs * ws * t.ld)
        assert p.max_view_elems() == want > 1


# ---- a plan's external outputs: Plan.outputs, and the engine's pure functions over it -------------------------------------------
def _task_cfg(family, scale, task, nc=3):
    return stock_cfg(family, scale, nc, task, **({"kpt_shape": (17, 3)} if task == "pose" else {}))


OUTPUT_GRAPHS = [("yolo11", "n", t, (64, 64)) for t in ("detect", "segment", "obb", "pose", "classify")] + [
    ("yolov8-p6", "n", "segment", (128, 192)), ("yolov9", "t", "detect", (64, 64)), ("bsyolo11", "n", "detect", (64, 64))]


@pytest.mark.parametrize("family,scale,task,hw", OUTPUT_GRAPHS)
def test_output_table_says_what_the_ops_write(family, scale, task, hw):
    """Plan.outputs against the op list, which is what the device sees: the external slots the ops' views name are the image and the
    table's slots, one name per slot; every view onto a slot is as wide as its entry's shape[1] (the raw maps a fused head conv writes
    through box[0]: `no`); raw_only marks the raw maps, the raw keypoint logits and the logits, nothing else; and the entries are the
    ones the engine's return forms are written for (slots pinned as numbers: they are the library's ABI)."""
    B = 2
    for kw in ({}, {"fuse_head": False}, {"precision": "fp32"}):
        plan = Plan(_task_cfg(family, scale, task), B, *hw, **kw)
        m, table = plan.meta, plan.outputs
        by_slot = {}
        for o in table.values():
            by_slot.setdefault(o.slot, []).append(o)
        assert all(len(v) == 1 for v in by_slot.values()), table
        assert [n for n, o in table.items() if n != o.name] == []
        seen = set()
        for op in plan.ops:
            views = [(k, op.get(k)) for k in ("src0", "src1", "dst", "res")] + [(k, t) for k in ("box", "cls", "msk") for t in op.get(k) or []]
            for k, t in views:
                if t is None or t.buf < L.BSY_EXT_BASE:
                    continue
                slot = t.buf - L.BSY_EXT_BASE
                seen.add(slot)
                if slot:
                    assert t.C == by_slot[slot][0].shape[1], (op["name"], k, slot, t.C)
                    if op["kind"] == L.OP_CONV and k == "box":
                        assert op["out_f32"] >= 2 and t.C == m["no"] and by_slot[slot][0].name == f"raw{op['level']}"
        assert seen == {0} | set(by_slot), (seen, table)
        assert {o.name for o in table.values() if o.raw_only} == {n for n in table if n.startswith("raw") or n in ("kpt", "x")}
        if task == "classify":
            k = min(3, 5)
            want = {"y": (1, (B, 3), "io"), "x": (2, (B, 3), "io"), "topk_idx": (3, (B, k), "int32"), "topk_val": (4, (B, k), "float32")}
        else:
            nl = len(m["levels"])
            assert nl == (4 if family == "yolov8-p6" else 3) and m["no"] == 64 + 3
            want = {"y": (1, (B, 4 + 3 + m["nm"] + m["ne"] + m.get("nk", 0), m["A"]), "io")}
            want.update({f"raw{l}": ([2, 3, 4, 6][l], (B, m["no"]) + tuple(m["levels"][l]), "io") for l in range(nl)})
            if task == "segment":
                want["proto"] = (5, (B, 32) + tuple(m["proto_hw"]), "io")
            if task == "pose":
                want["kpt"] = (5, (B, 51, m["A"]), "io")
        assert {n: (o.slot, o.shape, o.dtype) for n, o in table.items()} == want


def _tree_equal(a, b):
    """Same nesting, the same None positions, torch.equal tensors."""
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_tree_equal(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("want_raw", [True, False])
@pytest.mark.parametrize("task", ["detect", "segment", "obb", "pose", "classify"])
def test_pack_and_cat_outputs(task, want_raw):
    """engine.pack_outputs / cat_outputs, on CPU tensors shaped by a real plan's table at B = 5: the return value packed from the
    concatenated chunks (2, 2, 1 images) is the one packed from the whole batch, in the form of the task's head (head.py:74, :197,
    :223, :250, :304), and the rows behind the scores that Segment and OBB return are views of the returned y."""
    from bs_yolo_amd.engine import cat_outputs, pack_outputs
    plan = Plan(_task_cfg("yolo11", "n", task), 5, 64, 64)
    g = torch.Generator().manual_seed(5)
    dtypes = {"io": torch.float16, "int32": torch.int32, "float32": torch.float32}
    whole = {n: None if o.raw_only and not want_raw else (torch.rand(o.shape, generator=g) * 100).to(dtypes[o.dtype]) for n, o in plan.outputs.items()}
    chunks = [{n: None if t is None else t[a:b] for n, t in whole.items()} for a, b in ((0, 2), (2, 4), (4, 5))]
    cat = cat_outputs(chunks)
    assert list(cat) == list(whole) and all(_tree_equal(cat[n], whole[n]) for n in whole)
    one, many = pack_outputs(plan.meta, whole), pack_outputs(plan.meta, cat)
    assert _tree_equal(one, many)
    nl, raws = 3, [whole.get(f"raw{l}") for l in range(3)]
    assert raws == [None] * nl if not want_raw or task == "classify" else all(r is not None for r in raws)
    for y, extra in (one, many):
        assert y.shape[0] == 5
        rows = y[:, 4 + 3:]
        if task == "detect":
            assert isinstance(extra, list) and len(extra) == nl
        elif task == "segment":
            assert len(extra) == 3 and len(extra[0]) == nl and extra[2].shape == (5, 32, 16, 16)
        elif task == "obb":
            assert len(extra) == 2 and len(extra[0]) == nl and extra[1].shape == (5, 1, y.shape[2])
        elif task == "pose":
            assert len(extra) == 2 and len(extra[0]) == nl and (extra[1].shape == (5, 51, y.shape[2]) if want_raw else extra[1] is None)
        else:
            assert y.shape == (5, 3) and (extra.shape == (5, 3) if want_raw else extra is None)
        if task in ("segment", "obb"):
            assert extra[1]._base is y and extra[1].data_ptr() == rows.data_ptr() and extra[1].shape == rows.shape and extra[1].stride() == rows.stride()


def test_library_says_which_shapes_the_fused_kernels_take():
    """The planner asks the library (bsy_*_supported), it keeps no list of its own: the three predicates it asks besides the *_fused ones,
    at the edges the kernels define."""
    for (kd, hd), ok in {(16, 32): 1, (32, 64): 1, (64, 128): 1, (40, 80): 0, (80, 160): 0, (0, 32): 0, (32, 48): 0}.items():
        assert L.lib.bsy_attention_supported(kd, hd) == ok, (kd, hd)
    for c, ok in {32: 1, 64: 1, 48: 0, 128: 0}.items():
        assert L.lib.bsy_pmsfa_tail_supported(c) == ok, c
    for (h, w), ok in {(42, 45): 1, (31, 61): 0, (0, 45): 0, (0, 1): 0}.items():  # 1890 px fit LDS, 1891 do not
        assert L.lib.bsy_msca_spatial_supported(h, w) == ok, (h, w)


# ---- build / ISA guards (need hipcc's binutils only, no GPU) ----------------------------------------------------------------
def test_isa_has_no_packed_f32():
    """The concurrency-hazard mitigation of DESIGN.md section 7, enforced on the SHIPPED code objects: no kernel of
    libbsyolo_hip.so carries packed f32 arithmetic (v_pk_fma/mul/add_f32) -- hence none can pair it with SDWA f16->f32
    converts -- and no conv / fused-conv kernel has a private (scratch) frame."""
    sys.path.insert(0, str(ROOT / "tools"))
    import isa_scan
    bad, n, scratch = isa_scan.scan()
    assert n >= 130, f"only {n} kernels found: the disassembly failed"
    assert not bad, f"packed f32 arithmetic in {bad}"
    fam = ("conv_mfma_kernel", "conv3x3_patch", "conv1x1_persist", "conv1x1_wres", "c3k2_fused", "bneck_fused", "stem_fused", "dwpw_fused", "conv_first_mfma")
    conv_scratch = [k for k in scratch if any(f in k for f in fam)]
    assert not conv_scratch, f"scratch frames in {conv_scratch}"


def test_build_signature_tracks_flags_and_headers(tmp_path):
    """bs_yolo_amd/build.py rebuilds an object when its command line or ANY header of csrc/ / include/ changes (ADVICE r1:
    the correctness workaround is a flag, and image_conv.h was not tracked)."""
    from bs_yolo_amd import build as Bd
    src = tmp_path / "a.hip"
    hdr = tmp_path / "h.h"
    src.write_text("int f();")
    hdr.write_text("// v1")
    s0 = Bd._signature(["hipcc", "gfx950", "-fno-slp-vectorize", "a.hip"], src, [hdr])
    assert s0 == Bd._signature(["hipcc", "gfx950", "-fno-slp-vectorize", "a.hip"], src, [hdr])
    assert s0 != Bd._signature(["hipcc", "gfx950", "a.hip"], src, [hdr])
    hdr.write_text("// v2")
    assert s0 != Bd._signature(["hipcc", "gfx950", "-fno-slp-vectorize", "a.hip"], src, [hdr])
    hdrs = sorted(p.name for p in Bd.CSRC.glob("*.h"))
    assert "image_conv.h" in hdrs and "common.h" in hdrs


def test_stale_library_is_refused(monkeypatch):
    """bs_yolo_amd.lib refuses an in-tree library that was not built from the current sources (bs_yolo_amd/build.py stale_sources: object
    signatures = flags + source + every header): a source that stops compiling must not leave every test running yesterday's .so."""
    import importlib
    import bs_yolo_amd.build as BLD
    assert BLD.stale_sources() == []          # the tree the tests run on is up to date
    real = BLD._signature
    monkeypatch.setattr(BLD, "_signature", lambda cmd, src, headers: real(cmd, src, headers) + ("x" if src.name == "nms.hip" else ""))
    assert BLD.stale_sources() == ["nms.hip"]
    import bs_yolo_amd.lib as LL
    with pytest.raises(ImportError, match="not built from the current sources"):
        LL._load()
    monkeypatch.setenv("BSY_ALLOW_STALE_LIB", "1")
    assert LL._load() is not None
    importlib.reload(BLD)


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it must start two ranks itself (it exited asking for
    torch.distributed.run).  Without a GPU every rank stops at bench.py's own "needs a ROCm GPU" check -- which proves that
    the child launcher ran bench.py under WORLD_SIZE = 2 (the parent never gets that far: it only relays)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        pytest.skip("on a GPU box this would start a real 2-rank run")
    assert r.returncode != 0
    # at least one child rank got as far as the check (the launcher tears the other down when the first exits) and saw WORLD_SIZE = 2
    import re
    assert re.search(r"bench\.py needs a ROCm GPU.*\(rank [01] of 2\)", r.stderr), r.stderr[-2000:]


def test_weights_fingerprint_accepts_inference_tensors():
    """plugin._weights_version on parameters created under torch.inference_mode() (what fuse() produces inside the
    predictor's smart_inference_mode, engine/predictor.py:219): they have no version counter -- reading `_version` raises --
    so the fingerprint falls back to their storage pointers; ordinary tensors still count in-place updates."""
    from bs_yolo_amd import plugin
    with torch.inference_mode():
        conv = torch.nn.Conv2d(4, 4, 1)
    assert all(p.is_inference() for p in conv.parameters())
    with pytest.raises(RuntimeError):
        conv.weight._version
    f0 = plugin._weights_version(conv)
    assert f0 == plugin._weights_version(conv)
    conv.half()
    assert plugin._weights_version(conv) != f0      # new storages
    lin = torch.nn.Linear(3, 3)
    f1 = plugin._weights_version(lin)
    with torch.no_grad():
        lin.weight.mul_(2.0)
    assert plugin._weights_version(lin) != f1       # in-place update of an ordinary tensor
