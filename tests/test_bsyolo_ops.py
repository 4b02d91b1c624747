"""The BS-YOLO ops, each ALONE: PMSFA_TAIL, MSCA_SPATIAL, ELA, DWCONV_G in fp16 and DWPW as one-op plans (op_plan_helpers.run_op) on
channel views of poisoned buffers -- NaN around every source and between the weight records, 777.0 / 7.77e7 around every
destination -- as tests/test_glue_ops.py does for the glue ops.

Each fused op has two comparators that do not depend on each other: the launches it replaces, each run as its own one-op plan on
views of its own with the same weight records (bit for bit: the claim in each kernel's header), and an fp64 reference written here
that rounds every intermediate map to f16 where the module stores one.  The tolerances are those of the project's existing tests
of the same arithmetic (named next to each test); inputs are drawn as weights.synth_state_dict draws them.

Run on the MI355X box with ``pytest -m gpu``.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from op_plan_helpers import (DEV, NAN, POISON16, POISON32, assert_outside_views_intact, assert_poison_intact, bits, conv1x1_op, dw_ref,
                             dwg_op, dwg_record, nchw, new_op, nhwc, packed_1x1, poisoned, poisoned_blob, run_op, ulp16, view)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bs_yolo_amd import lib as L  # noqa: F401  (fails loudly when the .so is missing)

F16 = torch.float16


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _map16(g, *shape):
    """An O(1) map of f16 values."""
    return torch.randn(*shape, generator=g).to(F16)


def _dw_weights(g, kh, kw, Cc):
    """Depthwise (taps, C) weights and (C,) bias as weights.synth_state_dict draws them: He-normal over the taps, bias O(0.3)."""
    return torch.randn(kh * kw, Cc, generator=g) * (2.0 / (kh * kw)) ** 0.5, torch.rand(Cc, generator=g) * 0.6 - 0.3


def _dense_weights(g, cout, cin):
    """Dense 1x1 weights, He-normal and rounded to f16 (what the packed matrix holds), and the f32 bias."""
    return (torch.randn(cout, cin, generator=g) * (2.0 / cin) ** 0.5).to(F16).float(), torch.rand(cout, generator=g) * 0.6 - 0.3


def _h(t):
    """Round an fp64 map to f16, as the engine stores it, and go on in fp64."""
    return t.to(F16).double()


def _ratio(got, ref, tol):
    """worst |got - ref| / (atol + rtol |ref|) with rtol = atol = tol; inf when got is not finite (a padding NaN reached it)."""
    got, ref = got.double().cpu().numpy(), ref.numpy()
    if not np.isfinite(got).all():
        return math.inf
    return float((np.abs(got - ref) / (tol + tol * np.abs(ref))).max())


def _refused(op, ext, blob=b""):
    with pytest.raises(L.BsyError):
        run_op(op, ext, blob)


# ------------------------------------------------------------------------------------------------------------
# PMSFA_TAIL (pmsfa_fused.hip pmsfa_tail_kernel<32, 16, 16> / <64, 8, 16>)
# ------------------------------------------------------------------------------------------------------------
PMSFA_SHAPES = [(1, 1, 1), (2, 2, 2), (1, 16, 16), (1, 8, 16), (1, 17, 33), (3, 9, 13), (2, 3, 40), (2, 21, 5)]
PMSFA_MANY = {32: (130, 17, 17), 64: (65, 17, 33)}  # 520 / 585 tiles for 512 persistent workgroups: some walk two tiles
PMSFA_CASES = [(c, s) for c in (32, 64) for s in PMSFA_SHAPES + [PMSFA_MANY[c]]]


def _pmsfa_inputs(Cc, B, H, W):
    g = _gen(Cc, B, H, W)
    CH, CQ = Cc // 2, Cc // 4
    P, x = _map16(g, B, H, W, Cc), _map16(g, B, H, W, Cc)
    w2, b2 = _dw_weights(g, 5, 5, CH)
    w3, b3 = _dw_weights(g, 7, 7, CQ)
    ident = torch.zeros(49, CH - CQ)
    ident[24] = 1.0  # weights.pack_record kind "dwg_ext": centre tap 1, bias 0, no activation
    w3x, b3x = torch.cat((w3, ident), 1), torch.cat((b3, torch.zeros(CH - CQ)))
    w4, b4 = _dense_weights(g, Cc, Cc)
    return P, x, (w2, b2, w3, b3, w3x, b3x, w4, b4)


def _pmsfa_ref(P, x, wts):
    """block.py's PMSFA tail in fp64, the maps the module stores rounded to f16: q = SiLU(conv2 p1), s = SiLU(conv3 q1),
    conv4 = SiLU(W4 [s | q2 | p2] + b4), out = conv4 + x."""
    w2, b2, w3, b3, _, _, w4, b4 = wts
    Cc = P.shape[-1]
    CH, CQ = Cc // 2, Cc // 4
    q = _h(dw_ref(P[..., :CH], w2, b2, True, None, 5, 5))
    s = _h(dw_ref(q[..., :CQ], w3, b3, True, None, 7, 7))
    cat = torch.cat((s, q[..., CQ:], P[..., CH:].double()), -1)
    return _h(F.silu(cat @ w4.double().t() + b4.double())) + x.double()


def _pmsfa_blobs(wts):
    """-> (the unfused chain's blob, the fused op's, the six offsets).  Same records at the same offsets; the fused op's copy holds NaN
    in the identity half of the conv3 record, which the tail kernel has no reason to read."""
    w2, b2, w3, b3, w3x, b3x, w4, b4 = wts
    CQ = w3.shape[1]
    wp, bp = packed_1x1(w4, b4)
    chain, offs = poisoned_blob([w2.numpy(), b2.numpy(), w3x.numpy(), b3x.numpy(), wp, bp])
    w3n, b3n = w3x.clone(), b3x.clone()
    w3n[:, CQ:], b3n[CQ:] = NAN, NAN
    fused, offs2 = poisoned_blob([w2.numpy(), b2.numpy(), w3n.numpy(), b3n.numpy(), wp, bp])
    assert offs == offs2
    return chain, fused, offs


def _pmsfa_op(Cc, B, H, W, vP, vx, vd, offs):
    op = new_op(L.OP_PMSFA_TAIL, 0, B, H, W)
    op.src0, op.res, op.dst = vP, vx, vd
    op.ksize, op.stride, op.pad, op.act, op.heads, op.key_dim = 1, 1, 0, 1, Cc // 2, Cc // 2
    for i, o in enumerate(offs):
        op.aux_off[i] = o
    return op


@pytest.mark.parametrize("Cc,shape", PMSFA_CASES, ids=["%d-%dx%dx%d" % ((c,) + s) for c, s in PMSFA_CASES])
def test_pmsfa_tail(Cc, shape):
    """Bit for bit the chain DWCONV_G 5x5 -> DWCONV_G 7x7 (dwg_ext, writing S over p1 of a copy of P) -> CONV 1x1 + x, and within rtol =
    atol = 4e-3 of fp64 (the bound of test_c3k2_fused_matches_unfused_and_oracle: three chained f16 stages and a shortcut).  P at
    channel 8 of rows of C + 16; x and dst adjacent slices of ONE buffer of 3C + 8 channels (C3k2_gai's concat) at 17 x 33 and in
    the many-tile case, else in buffers of their own."""
    B, H, W = shape
    CH, CQ = Cc // 2, Cc // 4
    shared = shape == (1, 17, 33) or shape == PMSFA_MANY[Cc]
    if shape == PMSFA_MANY[Cc]:
        th, tw = (16, 16) if Cc == 32 else (8, 16)
        assert B * math.ceil(H / th) * math.ceil(W / tw) > 512
    P, x, wts = _pmsfa_inputs(Cc, B, H, W)
    chain_blob, fused_blob, offs = _pmsfa_blobs(wts)
    ldp, cp = Cc + 16, 8
    bufP = poisoned((B, H, W, ldp), cp, Cc, P, NAN)
    if shared:  # [NaN C | x | dst | 777 x 8]
        ldx = ldd = 3 * Cc + 8
        cx, cd = Cc, 2 * Cc
        host = torch.full((B, H, W, ldx), NAN, dtype=F16)
        host[..., cx:cx + Cc], host[..., cd:] = x, POISON16
        bufs = [host.to(DEV), host.to(DEV)]  # the fused run's and the chain's
        before = [host, host]
    else:
        ldx, cx, ldd, cd = Cc + 24, 8, Cc + 24, 16
        bufx = poisoned((B, H, W, ldx), cx, Cc, x, NAN)
        bufs = [poisoned((B, H, W, ldd), cd, Cc, None, POISON16, dtype=F16) for _ in range(2)]
        before = [b.cpu() for b in bufs]
    # the fused op
    xs = bufs[0] if shared else bufx
    run_op(_pmsfa_op(Cc, B, H, W, view(0, ldp, cp, Cc), view(1, ldx, cx, Cc), view(2 if not shared else 1, ldd, cd, Cc), offs),
           [bufP, xs] + ([] if shared else [bufs[0]]), fused_blob)
    # the chain, one plan per launch
    ldq, cq = CH + 16, 8
    Q = poisoned((B, H, W, ldq), cq, CH, None, POISON16, dtype=F16)
    run_op(dwg_op(0, B, H, W, 5, 5, 1, view(0, ldp, cp, CH), view(1, ldq, cq, CH), offs[0], offs[1], CH, 0, CH), [bufP, Q], chain_blob)
    assert_poison_intact(Q, cq, CH, POISON16)
    Pc = bufP.clone()
    run_op(dwg_op(0, B, H, W, 7, 7, 1, view(0, ldq, cq, CH), view(1, ldp, cp, CH), offs[2], offs[3], CH, 0, CQ, mid_c=CQ), [Q, Pc], chain_blob)
    assert_outside_views_intact(Pc, bufP.cpu(), [(cp, CH)])
    xs = bufs[1] if shared else bufx
    run_op(conv1x1_op(B, H, W, view(0, ldp, cp, Cc), view(2 if not shared else 1, ldd, cd, Cc), offs[4], offs[5], True, view(1, ldx, cx, Cc)),
           [Pc, xs] + ([] if shared else [bufs[1]]), chain_blob)
    for b, b0 in zip(bufs, before):
        assert_outside_views_intact(b, b0, [(cd, Cc)])
    assert torch.equal(bits(bufP)[..., cp:cp + Cc], bits(P)), "the op wrote its source"
    got, chain = bufs[0][..., cd:cd + Cc].cpu(), bufs[1][..., cd:cd + Cc].cpu()
    ratio = _ratio(got, _pmsfa_ref(P, x, wts), 4e-3)
    ndiff = int((bits(got) != bits(chain)).sum())
    print(f"pmsfa_tail C {Cc} {B}x{H}x{W} shared {shared}: worst error / bound {ratio:.3f}; {ndiff} elements differ from the chain")
    assert ndiff == 0 and ratio <= 1.0, f"{ndiff} of {got.numel()} elements differ from the unfused chain; worst error / bound {ratio:.3f}"


def test_pmsfa_tail_refusals():
    """Host-side refusals (BSY_ERR_ARG before any launch); every tensor and the blob are large enough for the layout they name."""
    B, H, W = 1, 4, 4
    z = lambda c: torch.zeros(B, H, W, c, dtype=F16, device=DEV)  # noqa: E731
    blob = bytes(256 * 1024)
    offs = [0, 8192, 16384, 65536, 131072, 196608]

    def op(Cc, vP, vx, vd):
        return _pmsfa_op(Cc, B, H, W, vP, vx, vd, offs)
    for Cc in (16, 128):                                                                               # widths without a kernel
        _refused(op(Cc, view(0, Cc, 0, Cc), view(1, Cc, 0, Cc), view(2, Cc, 0, Cc)), [z(Cc), z(Cc), z(Cc)], blob)
    _refused(op(32, view(0, 64, 0, 64), view(1, 32, 0, 32), view(2, 32, 0, 32)), [z(64), z(32), z(32)], blob)  # src0.C != dst.C
    for lds in ((44, 32, 32), (32, 44, 32), (32, 32, 44)):                                             # a row stride of 44 elements
        _refused(op(32, view(0, lds[0], 0, 32), view(1, lds[1], 0, 32), view(2, lds[2], 0, 32)), [z(48), z(48), z(48)], blob)
    _refused(op(32, view(0, 32, 0, 32), view(1, 32, 0, 32), view(1, 32, 0, 32)), [z(32), z(32)], blob)  # dst = x
    _refused(op(32, view(0, 32, 0, 32), view(1, 32, 0, 32), view(0, 32, 0, 32)), [z(32), z(32)], blob)  # dst = P


# ------------------------------------------------------------------------------------------------------------
# MSCA_SPATIAL (bsyolo_ops.hip msca_spatial_kernel)
# ------------------------------------------------------------------------------------------------------------
MSCA_SHAPES = [(1, 1), (2, 2), (3, 5), (7, 7), (8, 15), (1, 30), (30, 1), (20, 20), (42, 45)]
MSCA_STRIPS = (5, 7, 11, 21)


def _msca_records(g, Cc):
    """The nine (w [taps][C], b [C]) pairs in the op's order: conv0 (5 x 5), then per strip its 1 x k and k x 1 conv; the depthwise 1 x 1
    `dilconv` (y -> a y + d) is folded into the first three column convs in f32, as weights.pack_record does."""
    def plain(kh, kw):
        return torch.randn(kh * kw, Cc, generator=g) * (2.0 / (kh * kw)) ** 0.5, torch.rand(Cc, generator=g) * 0.4 - 0.2
    recs = [plain(5, 5)]
    a, d = torch.rand(Cc, generator=g) + 0.5, torch.rand(Cc, generator=g) * 0.4 - 0.2
    for i, k in enumerate(MSCA_STRIPS):
        recs.append(plain(1, k))
        w, b = plain(k, 1)
        recs.append((w * a, a * b + d) if i < 3 else (w, b))
    return recs


def _msca_ref(x, recs):
    """The four branch maps in fp64, every map the unfused plan stores rounded to f16."""
    attn = _h(dw_ref(x, *recs[0], False, None, 5, 5))
    out = []
    for i, k in enumerate(MSCA_STRIPS):
        t = _h(dw_ref(attn, *recs[1 + 2 * i], False, None, 1, k))
        out.append(dw_ref(t, *recs[2 + 2 * i], False, None, k, 1))
    return out


@pytest.mark.parametrize("H,W", MSCA_SHAPES)
@pytest.mark.parametrize("Cc", [8, 24])  # one channel block, three
def test_msca_spatial(Cc, H, W):
    """All eight outputs bit for bit the thirteen-op chain (DWCONV_G 5 x 5, four pairs of 1 x k / k x 1, four GAP); the branch maps
    within rtol = atol = 4e-3 of fp64 (three chained f16 maps, as for PMSFA above); each mean against the fp64 mean of the branch map
    the kernel itself wrote, under test_gap's bound ulp16(mean) + (ceil(HW / 256) + 9) 2^-24 mean|x|."""
    B, HW = 2, H * W
    assert L.lib.bsy_msca_spatial_supported(H, W) == 1
    g = _gen(Cc, H, W)
    x = _map16(g, B, H, W, Cc)
    recs = _msca_records(g, Cc)
    blob, offs = poisoned_blob([t.numpy() for r in recs for t in r])
    lds, cs = Cc + 16, 8
    ldb, ldg = 4 * (Cc + 8) + 8, 4 * (Cc + 8) + 8
    cb = [8 + i * (Cc + 8) for i in range(4)]
    src = poisoned((B, H, W, lds), cs, Cc, x, NAN)
    views = [(c, Cc) for c in cb]
    # the fused op
    br = poisoned((B, H, W, ldb), 0, 0, None, POISON16, dtype=F16)
    mean = poisoned((B, ldg), 0, 0, None, POISON16, dtype=F16)
    op = new_op(L.OP_MSCA_SPATIAL, 0, B, H, W)
    op.src0 = view(0, lds, cs, Cc)
    for i in range(4):
        bv, gv = view(1, ldb, cb[i], Cc), view(2, ldg, cb[i], Cc)
        if i < 3:
            op.box[i], op.cls[i] = bv, gv
        else:
            op.res, op.msk[0] = bv, gv
    for i, o in enumerate(offs):
        op.aux_off[i] = o
    run_op(op, [src, br, mean], blob)
    # the chain
    br2 = poisoned((B, H, W, ldb), 0, 0, None, POISON16, dtype=F16)
    mean2 = poisoned((B, ldg), 0, 0, None, POISON16, dtype=F16)
    lda, ca = Cc + 8, 0
    attn = poisoned((B, H, W, lda), ca, Cc, None, POISON16, dtype=F16)
    run_op(dwg_op(0, B, H, W, 5, 5, 1, view(0, lds, cs, Cc), view(1, lda, ca, Cc), offs[0], offs[1], Cc, 0, 0), [src, attn], blob)
    for i, k in enumerate(MSCA_STRIPS):
        t = poisoned((B, H, W, lda), ca, Cc, None, POISON16, dtype=F16)
        run_op(dwg_op(0, B, H, W, 1, k, 1, view(0, lda, ca, Cc), view(1, lda, ca, Cc), offs[2 + 4 * i], offs[3 + 4 * i], Cc, 0, 0), [attn, t], blob)
        run_op(dwg_op(0, B, H, W, k, 1, 1, view(0, lda, ca, Cc), view(1, ldb, cb[i], Cc), offs[4 + 4 * i], offs[5 + 4 * i], Cc, 0, 0), [t, br2], blob)
        gop = new_op(L.OP_GAP, 0, B, H, W)
        gop.src0, gop.dst = view(0, ldb, cb[i], Cc), view(1, ldg, cb[i], Cc)
        run_op(gop, [br2, mean2])
    full16 = lambda *s: torch.full(s, POISON16, dtype=F16)  # noqa: E731
    for t in (br, br2):
        assert_outside_views_intact(t, full16(B, H, W, ldb), views)
    for t in (mean, mean2):
        assert_outside_views_intact(t, full16(B, ldg), views)
    ref = _msca_ref(x, recs)
    worst, worst_mean, ndiff = 0.0, 0.0, 0
    for i in range(4):
        got, gm = br[..., cb[i]:cb[i] + Cc].cpu(), mean[:, cb[i]:cb[i] + Cc].cpu()
        ndiff += int((bits(got) != bits(br2[..., cb[i]:cb[i] + Cc])).sum()) + int((bits(gm) != bits(mean2[:, cb[i]:cb[i] + Cc])).sum())
        worst = max(worst, _ratio(got, ref[i], 4e-3))
        own = got.double().reshape(B, HW, Cc).numpy()
        m64, mabs = own.mean(1), np.abs(own).mean(1)
        bound = ulp16(m64) + (math.ceil(HW / 256) + 9) * 2.0 ** -24 * mabs
        gm = gm.double().numpy()
        worst_mean = max(worst_mean, float((np.abs(gm - m64) / bound).max()) if np.isfinite(gm).all() else math.inf)
    print(f"msca_spatial C {Cc} {H}x{W}: branch maps worst error / bound {worst:.3f}, means {worst_mean:.3f}; {ndiff} elements differ from the chain")
    assert ndiff == 0 and worst <= 1.0 and worst_mean <= 1.0, (f"{ndiff} elements differ from the unfused chain; worst error / bound: "
                                                               f"branch maps {worst:.3f}, means {worst_mean:.3f}")


def test_msca_spatial_limit():
    """42 x 45 = 1890 pixels is the last map the kernel's LDS takes (run above); 43 x 44 = 1892 is refused on the host."""
    assert L.lib.bsy_msca_spatial_supported(42, 45) == 1 and L.lib.bsy_msca_spatial_supported(43, 44) == 0
    B, H, W, Cc = 1, 43, 44, 8
    op = new_op(L.OP_MSCA_SPATIAL, 0, B, H, W)
    op.src0 = view(0, Cc, 0, Cc)
    for i in range(4):
        bv, gv = view(1 + i, Cc, 0, Cc), view(5 + i, Cc, 0, Cc)
        if i < 3:
            op.box[i], op.cls[i] = bv, gv
        else:
            op.res, op.msk[0] = bv, gv
    for i in range(18):
        op.aux_off[i] = 1024 * i
    z = lambda *s: torch.zeros(*s, dtype=F16, device=DEV)  # noqa: E731
    _refused(op, [z(B, H, W, Cc)] + [z(B, H, W, Cc) for _ in range(4)] + [z(B, Cc) for _ in range(4)], bytes(18 * 1024))


# ------------------------------------------------------------------------------------------------------------
# ELA (bsyolo_ops.hip ela_stats / ela_gate / ela_apply; ref32.hip ela_stats32 / ela_apply32)
# ------------------------------------------------------------------------------------------------------------
ELA_CASES = [  # C, H, W, k, B
    (8, 1, 1, 3, 2), (8, 1, 9, 3, 2),
    (8, 2, 300, 3, 2),    # a line longer than the 256 slots
    (24, 5, 7, 3, 2),     # one group of 24; 255 of 256 threads
    (40, 9, 13, 3, 2),    # groups of 20
    (48, 9, 13, 3, 2),    # 42 slots, 252 threads
    (64, 9, 13, 3, 2), (256, 20, 20, 5, 2), (16, 6, 4, 1, 2),
    (16, 6, 4, 15, 2),    # the dilated reach (28) exceeds the line
    (24, 661, 1, 3, 1),   # the longest side the gate kernel's LDS takes at 24 channels per group
]


def _ela_formula(x, wsp, wch, gnw, gnb, coef, k):
    """oracle.yolo_ref.ELA's formula on x (B, C, H, W) in x's own precision, without its f16 roundings."""
    B, Cc, H, W = x.shape
    groups = max(1, Cc // 16)
    ch = torch.sigmoid(F.conv1d(x.mean((2, 3)).view(B, Cc, 1), wch, None, 1, (k - 1) // 2, 1, Cc)).view(B, Cc, 1, 1)

    def gate(v):  # v (B, C, L)
        return torch.sigmoid(F.group_norm(F.conv1d(v, wsp, None, 1, (k - 1) * 2 // 2, 2, Cc), groups, gnw, gnb, 1e-5))
    mask = coef[0] * ch + coef[1] * (gate(x.mean(3)).view(B, Cc, H, 1) * gate(x.mean(2)).view(B, Cc, 1, W))
    return x * mask + coef[2] * x


def _ela_inputs(Cc, H, W, k, B, prec):
    g = _gen(Cc, H, W, k, prec)
    x = torch.randn(B, H, W, Cc, generator=g)
    x = x.to(F16) if prec == 0 else x
    wsp, wch = (torch.randn(Cc, 1, k, generator=g) * (2.0 / k) ** 0.5 for _ in range(2))
    gnw, gnb = torch.rand(Cc, generator=g) * 0.6 + 0.7, torch.rand(Cc, generator=g) * 0.6 - 0.3
    coef = [float(v) for v in torch.rand(3, generator=g) * 0.9 + 0.05]  # the three sigmoids: in (0, 1)
    return x, (wsp, wch, gnw, gnb), coef


def _ela_op(prec, B, H, W, Cc, k, coef, vs, vd, vscratch, w_off):
    op = new_op(L.OP_ELA, prec, B, H, W)
    op.src0, op.dst, op.res, op.ksize, op.w_off = vs, vd, vscratch, k, w_off
    op.scale, op.lvl_stride[0], op.lvl_stride[1] = coef
    return op


def _ela_scratch(B, H, W, Cc):
    """The f32 scratch of (2 (H + W) + 2) C floats per image, NaN (the op writes what it reads), with 64 poisoned floats behind it."""
    n = B * (2 * (H + W) + 2) * Cc
    t = torch.full((n + 64,), NAN, dtype=torch.float32)
    t[n:] = POISON32
    return t.to(DEV), n


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("Cc,H,W,k,B", ELA_CASES)
def test_ela(Cc, H, W, k, B, prec):
    """Against oracle.yolo_ref.ELA's formula in fp64.  prec 1: |got - ref| <= 1e-5 max(max|ref|, 1), the fp32-storage bound of
    test_dwconv_generic_f32.  prec 0: |got - ref| <= ulp16(ref) + 2^-16 |x| (ca + sb + rr), the form of test_msca_mix's bound: fast
    exponentials under gates of at most one, then one f16 rounding.  The same formula in float32 on the CPU has to stay within half
    of each bound: the inputs then are not in a GroupNorm cancellation where no f32 evaluation could."""
    x, (wsp, wch, gnw, gnb), coef = _ela_inputs(Cc, H, W, k, B, prec)
    ref = nhwc(_ela_formula(nchw(x.double()), wsp.double(), wch.double(), gnw.double(), gnb.double(), coef, k)).numpy()
    cpu32 = nhwc(_ela_formula(nchw(x.float()), wsp, wch, gnw, gnb, coef, k)).double().numpy()
    if prec == 0:
        bound = ulp16(ref) + 2.0 ** -16 * np.abs(x.double().numpy()) * sum(coef)
    else:
        bound = np.full_like(ref, 1e-5 * max(float(np.abs(ref).max()), 1.0))
    r32 = float((np.abs(cpu32 - ref) / bound).max())
    blob, (w_off,) = poisoned_blob([torch.cat([wsp.reshape(-1), wch.reshape(-1), gnw, gnb]).numpy()])
    lds, cs, ldd, cd = Cc + 16, 8, Cc + 24, 16
    dt, poison = (F16, POISON16) if prec == 0 else (torch.float32, POISON32)
    src = poisoned((B, H, W, lds), cs, Cc, x, NAN)
    dst = poisoned((B, H, W, ldd), cd, Cc, None, poison, dtype=dt)
    scratch, n = _ela_scratch(B, H, W, Cc)
    run_op(_ela_op(prec, B, H, W, Cc, k, coef, view(0, lds, cs, Cc), view(1, ldd, cd, Cc), view(2, Cc, 0, Cc), w_off), [src, dst, scratch], blob)
    got = dst[..., cd:cd + Cc].double().cpu().numpy()
    assert np.isfinite(got).all(), "a padding NaN reached the output"
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"ela prec {prec} C {Cc} {B}x{H}x{W} k {k}: worst error / bound {ratio:.3f} (float32 on the CPU: {r32:.3f})")
    assert r32 <= 0.5, r32
    assert ratio <= 1.0, ratio
    assert_poison_intact(dst, cd, Cc, poison)
    assert_poison_intact(scratch[None], 0, n, POISON32)


@pytest.mark.parametrize("prec", [0, 1])
def test_ela_refusals(prec):
    dt = F16 if prec == 0 else torch.float32
    for Cc, H, W, k in ((24, 662, 1, 3),              # one row more than the gate kernel's LDS takes
                        (16, 6, 4, 4), (16, 6, 4, 17),  # an even kernel, one longer than 15
                        (264, 4, 4, 5),               # 16 GroupNorm groups do not divide 264 channels
                        (12, 4, 4, 3)):               # not a multiple of 8
        B, ld = 1, (Cc + 7) // 8 * 8
        src, dst = (torch.zeros(B, H, W, ld, dtype=dt, device=DEV) for _ in range(2))
        scratch, _ = _ela_scratch(B, H, W, ld)
        _refused(_ela_op(prec, B, H, W, Cc, k, (0.5, 0.5, 0.5), view(0, ld, 0, Cc), view(1, ld, 0, Cc), view(2, Cc, 0, Cc), 0), [src, dst, scratch],
                 bytes(4 * (2 * ld * k + 2 * ld)))


# ------------------------------------------------------------------------------------------------------------
# DWCONV_G in fp16 (dwconv_tile_kernel<5 | 7, 1 | 2 | 4, .>, dwconv_win_kernel<1 | 3 s2 | 5 | 11 | 21>, dwconv_generic_kernel)
# ------------------------------------------------------------------------------------------------------------
DWG_TILED = [(k, k, 1, c, hw) for k in (5, 7) for c in (8, 16, 40) for hw in ((9, 13), (17, 35), (1, 1))]  # 1, 2, 4 chunks per workgroup
DWG_OTHER = [(kh, kw, s, 24, hw) for kh, kw, s in ((3, 3, 2), (1, 21, 1), (21, 1, 1), (1, 5, 1), (11, 1, 1), (9, 9, 1)) for hw in ((9, 13), (17, 35))]


def _dwg_run(x, wk, bias, kh, kw, stride, act_c, mid_c=0):
    """One fp16 DWCONV_G op on views: x (B, H, W, C) at channel 8 of rows of C + 16, weights in columns [8, 8 + C) of rows of C + 16."""
    B, H, W, Cc = x.shape
    wld, koff, lds, cs, ldd, cd = Cc + 16, 8, Cc + 16, 8, Cc + 24, 16
    blob, (w_off, b_off) = poisoned_blob(dwg_record(wk, bias, wld, koff))
    op = dwg_op(0, B, H, W, kh, kw, stride, view(0, lds, cs, Cc), view(1, ldd, cd, Cc), w_off, b_off, wld, koff, act_c, mid_c)
    src = poisoned((B, H, W, lds), cs, Cc, x, NAN)
    dst = poisoned((B, op.OH, op.OW, ldd), cd, Cc, None, POISON16, dtype=F16)
    run_op(op, [src, dst], blob)
    assert_poison_intact(dst, cd, Cc, POISON16)
    return dst[..., cd:cd + Cc].cpu()


@pytest.mark.parametrize("kh,kw,stride,Cc,hw", DWG_TILED + DWG_OTHER, ids=["%dx%d-s%d-C%d-%dx%d" % (c[:4] + c[4]) for c in DWG_TILED + DWG_OTHER])
def test_dwconv_generic_fp16(kh, kw, stride, Cc, hw):
    """SiLU on no, half and all channels, weight rows longer than the launch (key_dim = 8); rtol = atol = 2e-3 against fp64, the bound
    of test_dwconv_generic_matches_oracle."""
    B, (H, W) = 2, hw
    g = _gen(kh, kw, stride, Cc, H, W)
    x = _map16(g, B, H, W, Cc)
    wk, bias = _dw_weights(g, kh, kw, Cc)
    for act_c in (0, Cc // 2, Cc):
        got = _dwg_run(x, wk, bias, kh, kw, stride, act_c)
        ref = dw_ref(x, wk, bias, True, None, kh, kw, stride, act_c)
        assert tuple(ref.shape) == tuple(got.shape)
        ratio = _ratio(got, ref, 2e-3)
        print(f"dwconv_g fp16 {kh}x{kw} s{stride} C {Cc} {H}x{W} act {act_c}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, (act_c, ratio)


@pytest.mark.parametrize("hw", [(9, 13), (17, 35)], ids=["9x13", "17x35"])
@pytest.mark.parametrize("Cc", [16, 64])
def test_dwconv_generic_fp16_identity_half(Cc, hw, monkeypatch):
    """PMSFA's conv3 as the plan runs it: 7 x 7 on the first half, an identity kernel (centre tap 1, bias 0) on the second, SiLU on the
    first.  The tiled form copies the second half; it must return the bits of the window kernel (BSY_NO_DWTILE=1), which multiplies
    through: x + 0 exactly, so a -0 comes out as +0."""
    B, (H, W) = 2, hw
    CH = Cc // 2
    g = _gen(Cc, H, W)
    x = _map16(g, B, H, W, Cc)
    x[:, ::2, ::3, CH::5] = -0.0
    wk, bias = _dw_weights(g, 7, 7, CH)
    ident = torch.zeros(49, CH)
    ident[24] = 1.0
    wk2, bias2 = torch.cat((wk, ident), 1), torch.cat((bias, torch.zeros(CH)))
    for act_c in (CH // 2, CH):  # SiLU on half of the conv half; on all of it, as Plan.pmsfa asks
        monkeypatch.delenv("BSY_NO_DWTILE", raising=False)
        tiled = _dwg_run(x, wk2, bias2, 7, 7, 1, act_c, mid_c=CH)
        monkeypatch.setenv("BSY_NO_DWTILE", "1")
        win = _dwg_run(x, wk2, bias2, 7, 7, 1, act_c, mid_c=CH)
        monkeypatch.delenv("BSY_NO_DWTILE")
        assert torch.equal(bits(tiled), bits(win))
        assert torch.equal(bits(tiled[..., CH:]), bits((x[..., CH:].float() + 0.0).to(F16)))
        assert not bool(torch.signbit(tiled[..., CH:][x[..., CH:] == 0]).any())
        ratio = _ratio(tiled[..., :CH], dw_ref(x[..., :CH], wk, bias, True, None, 7, 7, 1, act_c), 2e-3)
        print(f"dwconv_g fp16 identity half C {Cc} {H}x{W} act {act_c}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, (act_c, ratio)


# ------------------------------------------------------------------------------------------------------------
# DWPW (dwpw_fused.hip dwpw_fused_kernel<1 | 2>)
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(17, 21), (3, 5)])
@pytest.mark.parametrize("Cc,C2", [(64, 80), (128, 128), (32, 128)])
def test_dwpw(Cc, C2, H, W):
    """Bit for bit the chain DWCONV (3 x 3, SiLU) -> CONV (1 x 1, SiLU), each a one-op plan, and rtol = atol = 3e-3 against fp64 with the
    depthwise map rounded to f16 (the bound of test_dwpw_fused_matches_unfused_and_oracle)."""
    B = 2
    g = _gen(Cc, C2, H, W)
    x = _map16(g, B, H, W, Cc)
    wd, bd = _dw_weights(g, 3, 3, Cc)
    w, b = _dense_weights(g, C2, Cc)
    blob, offs = poisoned_blob([wd.numpy(), bd.numpy(), *packed_1x1(w, b)])
    lds, cs, ldd, cd, ldm, cm = Cc + 16, 8, C2 + 24, 16, Cc + 8, 8
    src = poisoned((B, H, W, lds), cs, Cc, x, NAN)
    out, out2 = (poisoned((B, H, W, ldd), cd, C2, None, POISON16, dtype=F16) for _ in range(2))
    op = new_op(L.OP_DWPW, 0, B, H, W)
    op.src0, op.dst, op.ksize, op.stride, op.pad, op.act = view(0, lds, cs, Cc), view(1, ldd, cd, C2), 3, 1, 1, 1
    op.w_off, op.b_off, op.w2_off, op.b2_off = offs
    run_op(op, [src, out], blob)
    mid = poisoned((B, H, W, ldm), cm, Cc, None, POISON16, dtype=F16)
    dop = new_op(L.OP_DWCONV, 0, B, H, W)
    dop.src0, dop.dst, dop.ksize, dop.stride, dop.pad, dop.act = view(0, lds, cs, Cc), view(1, ldm, cm, Cc), 3, 1, 1, 1
    dop.w_off, dop.b_off = offs[0], offs[1]
    run_op(dop, [src, mid], blob)
    assert_poison_intact(mid, cm, Cc, POISON16)
    run_op(conv1x1_op(B, H, W, view(0, ldm, cm, Cc), view(1, ldd, cd, C2), offs[2], offs[3]), [mid, out2], blob)
    for t in (out, out2):
        assert_poison_intact(t, cd, C2, POISON16)
    got = out[..., cd:cd + C2].cpu()
    ndiff = int((bits(got) != bits(out2[..., cd:cd + C2])).sum())
    ref = F.silu(_h(dw_ref(x, wd, bd, True, None)) @ w.double().t() + b.double())
    ratio = _ratio(got, ref, 3e-3)
    print(f"dwpw C {Cc} -> {C2} {H}x{W}: worst error / bound {ratio:.3f}; {ndiff} elements differ from the chain")
    assert ndiff == 0 and ratio <= 1.0, f"{ndiff} of {got.numel()} elements differ from the unfused chain; worst error / bound {ratio:.3f}"
