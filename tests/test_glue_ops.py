"""The memory-bound ops between the convs, each ALONE: one bsy_op per plan (op_plan_helpers.run_op), every tensor a channel view
of a wider, poisoned buffer, in fp16 storage (prec 0) and exact fp32 storage (prec 1; prec 2 shares run_op_f32).

Ops whose output has one right answer (copy, transpose, maximum, f16 product) are compared bit for bit; GAP, MSCA_MIX, the
depthwise convs and the decode against an fp64 reference, with the bound derived next to each test.  Sources carry NaN outside
their view (a read of it reaches the output), destinations 777.0 / 7.77e7 (a store outside the view changes it).  The refusal
tests only pass layouts that the launchers reject on the host, before any launch.

Run on the MI355X box with ``pytest -m gpu``.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from op_plan_helpers import (DEV, NAN, POISON16, POISON32, assert_poison_intact, bits, dw_ref as _dw_ref, nchw, new_op, nhwc,
                             poisoned, run_op, ulp16, ulp32, view, weights_blob)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bs_yolo_amd import lib as L  # noqa: F401  (fails loudly when the .so is missing)

PREC = [0, 1]


def _dt(prec):
    return torch.float16 if prec == 0 else torch.float32


def _poison(prec):
    return POISON16 if prec == 0 else POISON32


def _randn(g, *shape, prec=0, scale=1.0):
    """randn in the storage format of `prec` (f16 values for prec 0)."""
    return (torch.randn(*shape, generator=g) * scale).to(_dt(prec))


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# ------------------------------------------------------------------------------------------------------------
# COPY (copy_view_kernel / copy32_kernel)
# ------------------------------------------------------------------------------------------------------------
COPY_CASES = [  # up0, H, W (the destination's), C, source coff, destination coff, precisions
    (0, 1, 1, 8, 8, 16, (0, 1)), (0, 3, 5, 24, 8, 16, (0, 1)), (0, 9, 7, 64, 8, 16, (0, 1, 2)),
    (1, 2, 2, 8, 8, 16, (0, 1)), (1, 6, 10, 24, 8, 16, (0, 1, 2)), (1, 4, 14, 64, 8, 16, (0, 1)),
    (0, 3, 5, 6, 1, 1, (1,)), (1, 6, 10, 6, 1, 1, (1,)),  # f32 only: six channels, views one float into the row
]


@pytest.mark.parametrize("up,H,W,Cc,cs,cd,prec", [c[:6] + (p,) for c in COPY_CASES for p in c[6]])
def test_copy(up, H, W, Cc, cs, cd, prec):
    """dst[n, y, x] = src[n, y >> up, x >> up] on views: identity or F.interpolate(mode="nearest"), bit for bit."""
    B = 2
    x = _randn(_gen(up, H, W, Cc, prec), B, H >> up, W >> up, Cc, prec=prec)
    ref = nhwc(F.interpolate(nchw(x.float()), scale_factor=2.0, mode="nearest")).to(x.dtype) if up else x
    lds, ldd = cs + Cc + 8, cd + Cc + 8
    src = poisoned((B, H >> up, W >> up, lds), cs, Cc, x, NAN)
    dst = poisoned((B, H, W, ldd), cd, Cc, None, _poison(prec), dtype=_dt(prec))
    op = new_op(L.OP_COPY, prec, B, H, W)
    op.src0, op.dst, op.up0 = view(0, lds, cs, Cc), view(1, ldd, cd, Cc), up
    run_op(op, [src, dst])
    assert torch.equal(bits(dst[..., cd:cd + Cc]), bits(ref))
    assert_poison_intact(dst, cd, Cc, _poison(prec))


# ------------------------------------------------------------------------------------------------------------
# GAP (gap_kernel / gap32_kernel)
# ------------------------------------------------------------------------------------------------------------
GAP_HW = {1: (1, 1), 2: (1, 2), 255: (15, 17), 256: (16, 16), 257: (1, 257), 1600: (40, 40)}


@pytest.mark.parametrize("HW,Cc,prec", [(hw, c, p) for hw in sorted(GAP_HW) for c in (8, 1280) for p in PREC] + [(257, 8, 2)])
def test_gap(HW, Cc, prec):
    """Mean over H * W.  The kernel sums 256 strided partials in f32 (ceil(HW / 256) additions each), then a tree of 8 steps, divides
    and rounds once: |got - mean64| <= one ulp of mean64 in the output format + (ceil(HW / 256) + 9) * 2^-24 * mean64(|x|)."""
    B, (H, W) = 3, GAP_HW[HW]
    lds, cs, ldo, cd = Cc + 24, 8, Cc + 16, 8
    g = _gen(HW, Cc, prec)
    for kind in ("randn", "positive", "wide"):
        x = torch.randn(B, H, W, Cc, generator=g)
        x = (x.abs() + 3 if kind == "positive" else 200 * x if kind == "wide" else x).to(_dt(prec))
        src = poisoned((B, H, W, lds), cs, Cc, x, NAN)
        dst = poisoned((B, ldo), cd, Cc, None, _poison(prec), dtype=_dt(prec))
        op = new_op(L.OP_GAP, prec, B, H, W)
        op.src0, op.dst = view(0, lds, cs, Cc), view(1, ldo, cd, Cc)
        run_op(op, [src, dst])
        x64 = x.double().reshape(B, HW, Cc).numpy()
        mean, mabs = x64.mean(1), np.abs(x64).mean(1)
        bound = (ulp16(mean) if prec == 0 else ulp32(mean)) + (math.ceil(HW / 256) + 9) * 2.0 ** -24 * mabs
        got = dst[:, cd:cd + Cc].double().cpu().numpy()
        ratio = float((np.abs(got - mean) / bound).max())
        print(f"gap prec {prec} HW {HW} C {Cc} {kind}: worst error / bound {ratio:.3f}")
        assert np.isfinite(got).all() and ratio <= 1.0, (kind, ratio)
        assert_poison_intact(dst, cd, Cc, _poison(prec))


# ------------------------------------------------------------------------------------------------------------
# MUL (mul_kernel / mul32_kernel)
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PREC)
@pytest.mark.parametrize("Cc", [8, 40])
@pytest.mark.parametrize("npix", [1, 31, 257])
def test_mul(npix, Cc, prec):
    """a * b on three different row strides.  fp16: the f32 product of two f16 values is exact, so (a.float() * b.float()).half()
    is the one correct rounding -- subnormal results (a third of the elements are drawn for them) and overflow to inf included."""
    g = _gen(npix, Cc, prec)
    k = torch.arange(npix * Cc).reshape(1, 1, npix, Cc) % 3
    sa, sb = torch.tensor([1.0, 1e-3, 300.0])[k], torch.tensor([1.0, 0.05, 300.0])[k]
    a = (torch.randn(1, 1, npix, Cc, generator=g) * sa).to(_dt(prec))
    b = (torch.randn(1, 1, npix, Cc, generator=g) * sb).to(_dt(prec))
    ref = (a.float() * b.float()).half() if prec == 0 else a * b
    if prec == 0:
        assert torch.equal(ref, (a.double() * b.double()).half())
        sub = ((ref.float().abs() > 0) & (ref.float().abs() < 2.0 ** -14)).float().mean().item()
        assert npix == 1 or (sub > 0.1 and bool(torch.isinf(ref).any())), sub
    lda, ca, ldb, cb, ldd, cd = Cc + 8, 8, Cc + 16, 0, Cc + 24, 16
    ta, tb = poisoned((1, 1, npix, lda), ca, Cc, a, NAN), poisoned((1, 1, npix, ldb), cb, Cc, b, NAN)
    dst = poisoned((1, 1, npix, ldd), cd, Cc, None, _poison(prec), dtype=_dt(prec))
    op = new_op(L.OP_MUL, prec, 1, 1, npix)
    op.src0, op.src1, op.dst = view(0, lda, ca, Cc), view(1, ldb, cb, Cc), view(2, ldd, cd, Cc)
    run_op(op, [ta, tb, dst])
    assert torch.equal(bits(dst[..., cd:cd + Cc]), bits(ref))
    assert_poison_intact(dst, cd, Cc, _poison(prec))


# ------------------------------------------------------------------------------------------------------------
# MSCA_MIX (msca_mix_kernel / mix32_kernel)
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PREC)
@pytest.mark.parametrize("HW", [1, 63, 700])
@pytest.mark.parametrize("Cc", [8, 24, 136, 1032, 2048])  # C8 = 1, 3 (255 of 256 threads), 17, 129 (one pixel per pass), 256
def test_msca_mix(Cc, HW, prec):
    """out = sum_i softmax_i(sigmoid(logit_i)) * branch_i over four branches that are views of ONE buffer.  Against fp64:
    |got - ref| <= 2^-16 * sum_i |w_i b_i| (the fast exponentials of the sigmoid and the softmax, four f32 FMAs) plus, in fp16, one
    f16 ulp of ref for the output rounding."""
    B, H, W = 2, (1 if HW != 700 else 20), (HW if HW != 700 else 35)
    g = _gen(Cc, HW, prec)
    ldb, ldl, cl, ldd, cd = 4 * Cc + 16, Cc + 8, 4, Cc + 16, 8
    br = [_randn(g, B, H, W, Cc, prec=prec) for _ in range(4)]
    buf = poisoned((B, H, W, ldb), 8, 4 * Cc, torch.cat(br, -1), NAN)
    lg = [torch.randn(B, Cc, generator=g) * s for s in (0.1, 1.0, 5.0, 30.0)]
    tl = [poisoned((B, ldl), cl, Cc, t, NAN) for t in lg]
    dst = poisoned((B, H, W, ldd), cd, Cc, None, _poison(prec), dtype=_dt(prec))
    op = new_op(L.OP_MSCA_MIX, prec, B, H, W)
    for i in range(4):
        bv, lv = view(0, ldb, 8 + i * Cc, Cc), view(1 + i, ldl, cl, Cc)
        if i < 3:
            op.box[i], op.cls[i] = bv, lv
        else:
            op.res, op.msk[0] = bv, lv
    op.dst = view(5, ldd, cd, Cc)
    run_op(op, [buf] + tl + [dst])
    w = torch.softmax(torch.sigmoid(torch.stack(lg).double()), 0)            # (4, B, C)
    terms = w[:, :, None, None, :] * torch.stack(br).double()                # (4, B, H, W, C)
    ref, mag = terms.sum(0).numpy(), terms.abs().sum(0).numpy()
    bound = 2.0 ** -16 * mag + (ulp16(ref) if prec == 0 else 0.0)
    got = dst[..., cd:cd + Cc].double().cpu().numpy()
    ratio = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    print(f"msca_mix prec {prec} C {Cc} HW {HW}: worst error / bound {ratio:.3f}")
    assert np.isfinite(got).all() and ratio <= 1.0, ratio
    assert_poison_intact(dst, cd, Cc, _poison(prec))


# ------------------------------------------------------------------------------------------------------------
# S2D (s2d_kernel; fp16 plans only)
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldd", [16, 24])
@pytest.mark.parametrize("H,W", [(2, 2), (6, 10), (34, 62)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_s2d(dtype, H, W, ldd):
    """BCHW image -> NHWC f16, channel (dy * 2 + dx) * 3 + c = image[c][2Y + dy][2X + dx] rounded once, channels 12..15 zero."""
    B = 2
    img = torch.rand(B, 3, H, W, generator=_gen(H, W, ldd)).to(dtype)
    a = img.numpy()
    ref = np.zeros((B, H // 2, W // 2, 16), np.float16)
    for dy in range(2):
        for dx in range(2):
            for c in range(3):
                ref[..., (dy * 2 + dx) * 3 + c] = a[:, c, dy::2, dx::2].astype(np.float16)
    dst = poisoned((B, H // 2, W // 2, ldd), 0, 16, None, POISON16, dtype=torch.float16)
    op = new_op(L.OP_S2D, 0, B, H, W)
    op.src0, op.dst, op.in_dtype = view(0, W, 0, 3), view(1, ldd, 0, 16), L.dtype_code(dtype)
    run_op(op, [img.to(DEV), dst])
    assert torch.equal(bits(dst[..., :16]), bits(torch.from_numpy(ref)))
    assert_poison_intact(dst, 0, 16, POISON16)


# ------------------------------------------------------------------------------------------------------------
# NHWC2NCHW (nhwc2nchw_kernel / nhwc2nchw32_kernel) and RAW_NCHW (raw_nchw_kernel)
# ------------------------------------------------------------------------------------------------------------
def _dense_out(n, dtype):
    """A dense output of n elements with 64 poisoned elements behind it, as one row."""
    return poisoned((1, n + 64), 0, n, None, POISON16 if dtype == torch.float16 else POISON32, dtype=dtype)


@pytest.mark.parametrize("prec", PREC)
@pytest.mark.parametrize("HW", [1, 33, 1025])
@pytest.mark.parametrize("Cc", [8, 32, 40])
def test_nhwc2nchw(Cc, HW, prec):
    B, lds, cs = 2, Cc + 16, 8
    x = _randn(_gen(Cc, HW, prec), B, 1, HW, Cc, prec=prec, scale=30.0)
    src = poisoned((B, 1, HW, lds), cs, Cc, x, NAN)
    for odt in (torch.float16, torch.float32):
        out = _dense_out(B * Cc * HW, odt)
        op = new_op(L.OP_NHWC2NCHW, prec, B, 1, HW)
        op.src0, op.dst, op.out_dtype = view(0, lds, cs, Cc), view(1, 0, 0, Cc), L.dtype_code(odt)
        run_op(op, [src, out])
        ref = x.reshape(B, HW, Cc).transpose(1, 2).to(odt)  # f32 -> f16 is .half(); f16 -> f32 is exact
        assert torch.equal(bits(out[0, :B * Cc * HW]), bits(ref.reshape(-1)))
        assert_poison_intact(out, 0, B * Cc * HW, POISON16 if odt == torch.float16 else POISON32)
    op.dst = view(1, 0, 0, Cc)
    run_op(op, [src, None])  # optional output: an unbound slot is OK and writes nothing
    run_op(op, [src])


@pytest.mark.parametrize("prec", PREC)
@pytest.mark.parametrize("h,w", [(1, 1), (15, 17), (1, 257)])
@pytest.mark.parametrize("nc", [1, 5, 80])
@pytest.mark.parametrize("level", [0, 3])
def test_raw_nchw(level, nc, h, w, prec):
    """cat(box, cls[:, :nc]) of one level as BCHW; the f32 logit maps are the same in both storage modes."""
    B, hw, ldb = 2, h * w, 72
    g = _gen(level, nc, hw, prec)
    box, cls = torch.randn(B, hw, 64, generator=g) * 4, torch.randn(B, hw, nc, generator=g) * 4
    tb = poisoned((B, hw, ldb), 0, 64, box, NAN)
    for ldc in ((nc + 3) & ~3, ((nc + 3) & ~3) + 8):
        tc = poisoned((B, hw, ldc), 0, nc, cls, NAN)
        for odt in (torch.float16, torch.float32):
            n = B * (64 + nc) * hw
            out = _dense_out(n, odt)
            op = new_op(L.OP_RAW_NCHW, prec, B, h, w)
            op.level, op.nc, op.out_dtype = level, nc, L.dtype_code(odt)
            op.box[level], op.cls[level], op.dst = view(0, ldb, 0, 64), view(1, ldc, 0, nc), view(2, 0, 0, 64 + nc)
            op.lvl_h[level], op.lvl_w[level] = h, w
            run_op(op, [tb, tc, out])
            ref = torch.cat((box, cls), -1).transpose(1, 2).to(odt)
            assert torch.equal(bits(out[0, :n]), bits(ref.reshape(-1)))
            assert_poison_intact(out, 0, n, POISON16 if odt == torch.float16 else POISON32)
    run_op(op, [tb, tc, None])  # optional output


# ------------------------------------------------------------------------------------------------------------
# SPPF_POOL (sppf_pool_lds_kernel, sppf_pool_kernel; sppf32_lds_kernel<4 / 2 / 1>, sppf32x4_kernel, sppf32_kernel)
# ------------------------------------------------------------------------------------------------------------
def _sppf16_form(B, H, W, Cc):
    """launch_sppf_pool's rule (elementwise.hip): the LDS kernel with `cg` chunks per workgroup, or the global-memory kernel."""
    if H * W * 32 <= 64 * 1024:
        for k in range(8, 1, -1):
            if (Cc // 8) % k == 0 and H * W * 32 * k <= 64 * 1024 and (Cc // 8 // k) * B >= 512:
                return ("lds", k)
        return ("lds", 1)
    return ("global", 0)


def _sppf32_form(B, H, W, Cc, ld, coff, slow):
    """launch_sppf32's rule (ref32.hip): LDS with V float4s per pixel, the x4 kernel, or the scalar kernel."""
    vec4 = Cc % 4 == 0 and ld % 4 == 0 and coff % 4 == 0
    V = next((v for v in (4, 2, 1) if H * W * v * 32 <= 65536 and (Cc // 4) % v == 0), 0)
    if vec4 and V and not slow and B <= 65535:
        return ("lds", V)
    return ("x4", 0) if vec4 else ("scalar", 0)


def _sppf_run(x, coff, prec):
    """x (B, H, W, C) -> the (B, H, W, 4C) the op leaves in channels [coff, coff + 4C) of a poisoned buffer of ld = 4C + 8.  The poison
    is the large finite one: fmaxf drops a NaN, 777 / 7.77e7 wins every maximum it enters."""
    B, H, W, Cc = x.shape
    ld = 4 * Cc + 8
    buf = poisoned((B, H, W, ld), coff, Cc, x, _poison(prec))
    op = new_op(L.OP_SPPF_POOL, prec, B, H, W)
    op.src0 = view(0, ld, coff, Cc)
    run_op(op, [buf])
    assert_poison_intact(buf, coff, 4 * Cc, _poison(prec))
    return buf[..., coff:coff + 4 * Cc].cpu()


def _sppf_ref(x):
    y = [nchw(x.float())]
    for _ in range(3):
        y.append(F.max_pool2d(y[-1], 5, 1, 2))
    return nhwc(torch.cat(y, 1)).to(x.dtype)


SPPF16_CASES = [  # B, H, W, C, form
    (2, 20, 13, 32, ("lds", 1)), (1, 1, 1, 8, ("lds", 1)), (512, 5, 4, 64, ("lds", 8)), (512, 5, 4, 48, ("lds", 6)),
    (2, 32, 64, 8, ("lds", 1)),     # both LDS maps = exactly 64 KiB
    (2, 41, 50, 8, ("global", 0)),  # 2050 pixels
    (2, 3, 9, 16, ("lds", 1)), (2, 9, 4, 16, ("lds", 1)),  # H < 5, W < 5: a window covers the whole axis
]


@pytest.mark.parametrize("B,H,W,Cc,form", SPPF16_CASES)
def test_sppf_pool_fp16(B, H, W, Cc, form):
    assert _sppf16_form(B, H, W, Cc) == form
    if (H, W) == (32, 64):
        assert H * W * 32 == 64 * 1024
    x = _randn(_gen(B, H, W, Cc), B, H, W, Cc, prec=0)
    assert torch.equal(bits(_sppf_run(x, 0, 0)), bits(_sppf_ref(x)))  # maxima are exact


SPPF32_CASES = [  # B, H, W, C, coff, form
    (2, 16, 32, 16, 0, ("lds", 4)),   # 512 pixels: V = 4 at exactly 64 KiB
    (2, 19, 27, 16, 0, ("lds", 2)),   # 513 pixels: V = 2 by size
    (2, 20, 13, 8, 0, ("lds", 2)),    # V = 2 by width
    (2, 40, 40, 4, 0, ("lds", 1)),
    (2, 41, 50, 8, 0, ("x4", 0)),     # 2050 pixels: no LDS form fits
    (2, 7, 9, 6, 0, ("scalar", 0)), (2, 7, 9, 8, 1, ("scalar", 0)),
    (2, 3, 9, 16, 0, ("lds", 4)), (2, 9, 4, 16, 0, ("lds", 4)),
]


@pytest.mark.parametrize("B,H,W,Cc,coff,form", SPPF32_CASES)
def test_sppf_pool_f32(B, H, W, Cc, coff, form, monkeypatch):
    ld = 4 * Cc + 8
    assert _sppf32_form(B, H, W, Cc, ld, coff, False) == form
    assert _sppf32_form(B, H, W, Cc, ld, coff, True) == (("scalar", 0) if form[0] == "scalar" else ("x4", 0))
    if (H, W, Cc) == (16, 32, 16):
        assert H * W * 4 * 32 == 65536
    x = _randn(_gen(B, H, W, Cc, coff), B, H, W, Cc, prec=1)
    ref = _sppf_ref(x)
    monkeypatch.delenv("BSY_REF32_SLOW", raising=False)
    fast = _sppf_run(x, coff, 1)
    monkeypatch.setenv("BSY_REF32_SLOW", "1")
    slow = _sppf_run(x, coff, 1)
    monkeypatch.delenv("BSY_REF32_SLOW")
    assert torch.equal(bits(fast), bits(ref)) and torch.equal(bits(slow), bits(ref))


# ------------------------------------------------------------------------------------------------------------
# DWCONV 3x3 (dwconv3x3_kernel; dw32_3x3x4_kernel, dw32x4_kernel, dw32_kernel) and DWCONV_G in f32
# ------------------------------------------------------------------------------------------------------------
def _dw_run(prec, x, w9, bias, act, res, cs, lds):
    """One DWCONV op: x (B, H, W, C) in channels [cs, cs + C) of a NaN-poisoned source, residual and destination with row strides of
    their own.  Returns the (B, H, W, C) output."""
    B, H, W, Cc = x.shape
    ldr, cr, ldd, cd = Cc + 8, 0, Cc + 24, 16 if cs % 4 == 0 else 1
    blob, (w_off, b_off) = weights_blob([w9.numpy(), bias.numpy()])
    src = poisoned((B, H, W, lds), cs, Cc, x, NAN)
    dst = poisoned((B, H, W, ldd), cd, Cc, None, _poison(prec), dtype=_dt(prec))
    ext = [src, dst]
    op = new_op(L.OP_DWCONV, prec, B, H, W)
    op.src0, op.dst, op.act, op.w_off, op.b_off = view(0, lds, cs, Cc), view(1, ldd, cd, Cc), int(act), w_off, b_off
    if res is not None:
        ext.append(poisoned((B, H, W, ldr), cr, Cc, res, NAN))
        op.res = view(2, ldr, cr, Cc)
    run_op(op, ext, blob)
    assert_poison_intact(dst, cd, Cc, _poison(prec))
    return dst[..., cd:cd + Cc].cpu()


DW_SHAPES = [(1, 1), (1, 9), (7, 1), (8, 2), (9, 7), (17, 3)]


@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("H,W", DW_SHAPES)
def test_dwconv3x3_fp16(H, W, Cc):
    """All four of act x residual against fp64 at rtol = atol = 2e-3 (the bound of test_dwconv_matches_oracle: f32 accumulation of
    exact f16 x f32 products, one f16 rounding of an O(1) output)."""
    B = 2
    g = _gen(H, W, Cc)
    x, res = _randn(g, B, H, W, Cc), _randn(g, B, H, W, Cc)
    w9, bias = torch.randn(9, Cc, generator=g) * 0.4, torch.randn(Cc, generator=g) * 0.2
    for act in (False, True):
        for r in (None, res):
            got = _dw_run(0, x, w9, bias, act, r, 8, Cc + 16).double().numpy()
            ref = _dw_ref(x, w9, bias, act, r).numpy()
            err = np.abs(got - ref) / (2e-3 + 2e-3 * np.abs(ref))
            print(f"dwconv3x3 fp16 {H}x{W} C {Cc} act {act} res {r is not None}: worst error / bound {float(err.max()):.3f}")
            np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("Cc,cs", [(8, 8), (24, 8), (6, 1)])  # (6, 1): the scalar form
@pytest.mark.parametrize("H,W", DW_SHAPES + [(9, 3), (9, 4), (9, 5)])  # W = 3, 4, 5: the four-wide window's tail
def test_dwconv3x3_f32(H, W, Cc, cs, monkeypatch):
    """The fast forms and the BSY_REF32_SLOW ones return the same bits (the claim in ref32.hip), and both are within 1e-5 of the output
    range of fp64 (the bound of test_attention32_tiled_equals_generic)."""
    B = 2
    g = _gen(H, W, Cc, cs)
    x, res = _randn(g, B, H, W, Cc, prec=1), _randn(g, B, H, W, Cc, prec=1)
    w9, bias = torch.randn(9, Cc, generator=g) * 0.4, torch.randn(Cc, generator=g) * 0.2
    for act in (False, True):
        for r in (None, res):
            monkeypatch.delenv("BSY_REF32_SLOW", raising=False)
            fast = _dw_run(1, x, w9, bias, act, r, cs, Cc + 16 if cs % 4 == 0 else Cc + 5)
            monkeypatch.setenv("BSY_REF32_SLOW", "1")
            slow = _dw_run(1, x, w9, bias, act, r, cs, Cc + 16 if cs % 4 == 0 else Cc + 5)
            monkeypatch.delenv("BSY_REF32_SLOW")
            assert torch.equal(bits(fast), bits(slow))
            ref = _dw_ref(x, w9, bias, act, r)
            err = float((fast.double() - ref).abs().max()) / (1e-5 * max(float(ref.abs().max()), 1.0))
            print(f"dwconv3x3 f32 {H}x{W} C {Cc} act {act} res {r is not None}: worst error / bound {err:.3f}")
            assert err <= 1.0, err


@pytest.mark.parametrize("Cc", [16, 6])
@pytest.mark.parametrize("kh,kw,stride", [(5, 5, 1), (3, 3, 2), (1, 21, 1)])
def test_dwconv_generic_f32(kh, kw, stride, Cc):
    """DWCONV_G in exact fp32 storage, fields as run_op_f32 reads them: ksize = kh, pad = kw, heads = weight row length, key_dim =
    channel offset into the weight rows and the bias, act = leading SiLU channels.  1e-5 of the range against fp64."""
    B, H, W = 2, 11, 13
    g = _gen(kh, kw, stride, Cc)
    koff, wld, act_c = (4, Cc + 8, Cc // 2) if Cc % 4 == 0 else (3, Cc + 5, Cc // 2)
    cs, lds, cd, ldd = (8, Cc + 16, 16, Cc + 24) if Cc % 4 == 0 else (1, Cc + 5, 1, Cc + 3)
    x = _randn(g, B, H, W, Cc, prec=1)
    wk, bias = torch.randn(kh * kw, Cc, generator=g) * (1.0 / (kh * kw)) ** 0.5, torch.randn(Cc, generator=g) * 0.2
    wfull, bfull = torch.full((kh * kw, wld), NAN), torch.full((koff + Cc,), NAN)
    wfull[:, koff:koff + Cc], bfull[koff:] = wk, bias
    blob, (w_off, b_off) = weights_blob([wfull.numpy(), bfull.numpy()])
    OH, OW = (H + 2 * (kh // 2) - kh) // stride + 1, (W + 2 * (kw // 2) - kw) // stride + 1
    src = poisoned((B, H, W, lds), cs, Cc, x, NAN)
    dst = poisoned((B, OH, OW, ldd), cd, Cc, None, POISON32, dtype=torch.float32)
    op = new_op(L.OP_DWCONV_G, 1, B, H, W)
    op.OH, op.OW, op.ksize, op.pad, op.stride, op.heads, op.key_dim, op.act = OH, OW, kh, kw, stride, wld, koff, act_c
    op.src0, op.dst, op.w_off, op.b_off = view(0, lds, cs, Cc), view(1, ldd, cd, Cc), w_off, b_off
    run_op(op, [src, dst], blob)
    ref = _dw_ref(x, wk, bias, True, None, kh, kw, stride, act_c)
    assert tuple(ref.shape) == (B, OH, OW, Cc)
    err = float((dst[..., cd:cd + Cc].cpu().double() - ref).abs().max()) / (1e-5 * max(float(ref.abs().max()), 1.0))
    print(f"dwconv_g f32 {kh}x{kw} s{stride} C {Cc}: worst error / bound {err:.3f}")
    assert err <= 1.0, err
    assert_poison_intact(dst, cd, Cc, POISON32)


# ------------------------------------------------------------------------------------------------------------
# DECODE (decode_kernel through bsy_detect_decode and BSY_OP_DECODE)
# ------------------------------------------------------------------------------------------------------------
DEC_LEVELS = {3: ([(1, 1), (7, 9), (8, 8)], [8.0, 16.0, 32.0]),  # one anchor, 63, 64: below a tile, one short of it, exactly one
              1: ([(5, 13)], [16.0])}                            # 65: one tile and one anchor


def _decode_inputs(nl, nc, nm, ldb, B, seed):
    g = _gen(nl, nc, nm, ldb, seed)
    hw, strides = DEC_LEVELS[nl]
    box = [torch.randn(B, h * w, 64, generator=g) * 2 for h, w in hw]
    cls = [torch.randn(B, h * w, nc, generator=g) * 3 for h, w in hw]
    msk = [torch.randn(B, h * w, nm, generator=g) * 2 for h, w in hw] if nm else None
    ldc, ldm = ((nc + 3) & ~3) + 4, nm + 8  # class and mask rows wider than their payload
    tb = [poisoned((B * t.shape[1], ldb), 0, 64, t.reshape(-1, 64), NAN) for t in box]
    tc = [poisoned((B * t.shape[1], ldc), 0, nc, t.reshape(-1, nc), NAN) for t in cls]
    tm = [poisoned((B * t.shape[1], ldm), 0, nm, t.reshape(-1, nm), NAN) for t in msk] if nm else None
    return hw, strides, (box, cls, msk), (tb, tc, tm)


def _detect_decode(tb, tc, tm, hw, strides, B, nc, nm, y, odt):
    """bsy_detect_decode on row strides taken from the tensors (ops.detect_decode reads nm off the mask rows' width)."""
    vp, i32, nl = C.c_void_p, C.c_int, len(tb)
    ptrs = lambda ts: (vp * nl)(*[t.data_ptr() for t in ts])  # noqa: E731
    lds = lambda ts: (i32 * nl)(*[t.shape[-1] for t in ts])   # noqa: E731
    L.check(L.lib.bsy_detect_decode(ptrs(tb), lds(tb), ptrs(tc), lds(tc), ptrs(tm) if nm else None, lds(tm) if nm else None,
                                    (i32 * nl)(*[h for h, _ in hw]), (i32 * nl)(*[w for _, w in hw]), (C.c_float * nl)(*strides), nl, B, nc,
                                    nm, y.data_ptr(), L.dtype_code(odt), L.stream_ptr(y.device)))
    torch.cuda.synchronize()


def _decode_ref(box, cls, msk, hw, strides):
    """fp64 DFL expectation + dist2bbox (xywh) * stride, sigmoid of the class logits, mask coefficients as they are: (B, 4 + nc + nm, A)."""
    out = []
    for l, (h, w) in enumerate(hw):
        b = box[l].double()
        d = (torch.softmax(b.reshape(b.shape[0], h * w, 4, 16), -1) * torch.arange(16, dtype=torch.float64)).sum(-1)
        a = torch.arange(h * w)
        ax, ay = (a % w).double() + 0.5, (a // w).double() + 0.5
        x1, y1, x2, y2 = ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]
        rows = [torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), 1) * strides[l], torch.sigmoid(cls[l].double()).transpose(1, 2)]
        if msk:
            rows.append(msk[l].double().transpose(1, 2))
        out.append(torch.cat(rows, 1))
    return torch.cat(out, 2).numpy()


def _decode_check(y, ref, odt, tag):
    got = y.double().cpu().numpy()
    assert np.isfinite(got).all(), "a padding NaN reached the output"
    bound = 2e-4 + 1e-5 * np.abs(ref) + (ulp16(ref) if odt == torch.float16 else 0.0)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"decode {tag}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("odt", [torch.float32, torch.float16])
@pytest.mark.parametrize("ldb", [64, 72])
@pytest.mark.parametrize("nm", [0, 32])
@pytest.mark.parametrize("nc", [1, 5, 80])
@pytest.mark.parametrize("nl", [3, 1])
def test_decode(nl, nc, nm, ldb, odt):
    """rtol = 1e-5, atol = 2e-4 against fp64 (the bound of test_detect_decode_golden), plus one f16 ulp of the reference for f16 output."""
    B = 3
    hw, strides, (box, cls, msk), (tb, tc, tm) = _decode_inputs(nl, nc, nm, ldb, B, 0)
    A = sum(h * w for h, w in hw)
    n = B * (4 + nc + nm) * A
    out = _dense_out(n, odt)
    _detect_decode(tb, tc, tm, hw, strides, B, nc, nm, out, odt)
    y = out[0, :n].reshape(B, 4 + nc + nm, A)
    _decode_check(y, _decode_ref(box, cls, msk, hw, strides), odt, f"nl {nl} nc {nc} nm {nm} ldb {ldb} {odt}")
    assert_poison_intact(out, 0, n, POISON16 if odt == torch.float16 else POISON32)


@pytest.mark.parametrize("odt", [torch.float32, torch.float16])
def test_decode_op_equals_entry_point(odt):
    """BSY_OP_DECODE fills the same launch as bsy_detect_decode: the same bits, and nothing behind the prediction tensor."""
    B, nl, nc, nm, ldb = 3, 3, 5, 32, 72
    hw, strides, (box, cls, msk), (tb, tc, tm) = _decode_inputs(nl, nc, nm, ldb, B, 1)
    A = sum(h * w for h, w in hw)
    n = B * (4 + nc + nm) * A
    out = _dense_out(n, odt)
    op = new_op(L.OP_DECODE, 0, B, 0, 0)
    op.nl, op.nc, op.nm, op.A, op.out_dtype = nl, nc, nm, A, L.dtype_code(odt)
    for l, (h, w) in enumerate(hw):
        op.box[l], op.cls[l], op.msk[l] = view(l, ldb, 0, 64), view(3 + l, tc[l].shape[-1], 0, nc), view(6 + l, tm[l].shape[-1], 0, nm)
        op.lvl_h[l], op.lvl_w[l], op.lvl_stride[l] = h, w, strides[l]
    op.dst = view(9, 0, 0, 4 + nc + nm)
    run_op(op, tb + tc + tm + [out])
    y = out[0, :n].reshape(B, 4 + nc + nm, A)
    direct = torch.empty_like(y)
    _detect_decode(tb, tc, tm, hw, strides, B, nc, nm, direct, odt)
    assert torch.equal(bits(y), bits(direct))
    _decode_check(y, _decode_ref(box, cls, msk, hw, strides), odt, f"op {odt}")
    assert_poison_intact(out, 0, n, POISON16 if odt == torch.float16 else POISON32)


# ------------------------------------------------------------------------------------------------------------
# refusals: layouts every launcher rejects on the host (BSY_ERR_ARG from bsy_plan_run, nothing launched).  Every tensor is large
# enough for the layout it names.
# ------------------------------------------------------------------------------------------------------------
def _z16(*shape):
    return torch.zeros(*shape, dtype=torch.float16, device=DEV)


def _simple(kind, Cc, ld, coff, H=4, W=4, up=0, ldd=None, cd=0):
    """A COPY / MUL / GAP / MSCA_MIX op over zero tensors of (2, H, W, 64) with the given source layout; the destination is sound
    unless told otherwise."""
    op = new_op(kind, 0, 2, H, W)
    t, lg = _z16(2, H, W, 64), torch.zeros(2, 64, device=DEV)
    ldd = 32 if ldd is None else ldd
    op.src0, op.src1, op.dst, op.up0 = view(0, ld, coff, Cc), view(0, ld, coff, Cc), view(1, ldd, cd, Cc), up
    for i in range(3):
        op.box[i], op.cls[i] = view(0, ld, coff, Cc), view(2, 64, 0, Cc)
    op.res, op.msk[0] = view(0, ld, coff, Cc), view(2, 64, 0, Cc)
    return op, [t, _z16(2, H, W, 64), lg]


@pytest.mark.parametrize("kind", ["OP_COPY", "OP_MUL", "OP_MSCA_MIX", "OP_GAP"])
@pytest.mark.parametrize("Cc,ld,coff", [(12, 32, 0), (8, 12, 0), (8, 32, 4)])  # C % 8, row stride % 8, a view 8 bytes into a 16-byte piece
def test_fp16_layout_rules_are_refused(kind, Cc, ld, coff):
    op, ext = _simple(getattr(L, kind), Cc, ld, coff)
    with pytest.raises(L.BsyError):
        run_op(op, ext)


def test_refusals_of_single_ops():
    def refused(op, ext):
        with pytest.raises(L.BsyError):
            run_op(op, ext)
    refused(*_simple(L.OP_COPY, 8, 32, 0, H=3, W=4, up=1))             # nearest x2 onto an odd height
    refused(*_simple(L.OP_GAP, 16, 32, 0, ldd=8))                      # output row shorter than C
    op = new_op(L.OP_MSCA_MIX, 0, 1, 1, 1)                             # C = 2056: more than 256 chunks per pixel
    for i in range(3):
        op.box[i], op.cls[i] = view(0, 2056, 0, 2056), view(1, 2056, 0, 2056)
    op.res, op.msk[0], op.dst = view(0, 2056, 0, 2056), view(1, 2056, 0, 2056), view(2, 2056, 0, 2056)
    refused(op, [_z16(1, 1, 1, 2056), torch.zeros(1, 2056, device=DEV), _z16(1, 1, 1, 2056)])
    for H, W, ldd in ((4, 5, 16), (4, 4, 8)):                          # S2D: odd W; a row stride below the 16 channels it writes
        op = new_op(L.OP_S2D, 0, 1, H, W)
        op.src0, op.dst, op.in_dtype = view(0, W, 0, 3), view(1, ldd, 0, 16), L.BSY_F16
        refused(op, [_z16(1, 3, H, W), _z16(1, H, W, 16)])
    for prec in PREC:                                                  # SPPF: the four slices do not fit the row
        op = new_op(L.OP_SPPF_POOL, prec, 1, 4, 4)
        op.src0 = view(0, 24, 0, 8)
        refused(op, [torch.zeros(1, 4, 4, 32, dtype=_dt(prec), device=DEV)])
    box, cls = torch.zeros(16, 64, device=DEV), torch.zeros(16, 8, device=DEV)
    with pytest.raises(L.BsyError):                                    # decode: nc = 5 needs class rows of 8 floats, told 4
        vp, i32 = C.c_void_p, C.c_int
        y = torch.zeros(1, 9, 16, device=DEV)
        L.check(L.lib.bsy_detect_decode((vp * 1)(box.data_ptr()), (i32 * 1)(64), (vp * 1)(cls.data_ptr()), (i32 * 1)(4), None, None,
                                        (i32 * 1)(4), (i32 * 1)(4), (C.c_float * 1)(8.0), 1, 1, 5, 0, y.data_ptr(), L.BSY_F32,
                                        L.stream_ptr(y.device)))
