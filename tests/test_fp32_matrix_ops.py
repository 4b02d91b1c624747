"""The ops that do the arithmetic of the two fp32-storage modes, each ALONE: CONV, CONV_FIRST and ATTN with prec 1 (exact) and prec 2
(fp32x, split-f16) as one-op plans (op_plan_helpers.run_op) on channel views of poisoned buffers -- NaN around every source and
between the parts of every weight record, 7.77e7 around every destination -- as tests/test_glue_ops.py and tests/test_bsyolo_ops.py do
for the other ops.  This reaches what the stand-alone entry points (bsy_conv2d_f32 / _f32x, bsy_conv_first_f32, bsy_attention_f32)
cannot pass: two sources, nearest x2 on either, dst_scale / dst_dy / dst_dx, a shortcut and a destination that are offset views with
row strides of their own (or the same view), and the routing chain fp32x -> exact MFMA -> scalar on views the matrix kernels refuse.

Two kinds of comparison.  Integer payloads (every partial sum an integer below 2^24) have ONE right answer in both modes and are
compared bit for bit with an fp64 evaluation of integers.  Random payloads are compared with fp64 under a bound derived per output
element from the operands (see _reference), not from the output range; test_cpu_float32_within_half_the_bound shows on the CPU that a
correct fp32 evaluation with another summation order uses less than half of it.

ROUTE below mirrors conv32_mfma_supported (csrc/conv32_mfma.hip), conv32x_mfma_supported and the tile choice of launch_conv32x_mfma
(csrc/conv32x_mfma.hip) / launch_conv32_mfma; it is written from the C++ and test_case_list_reaches_every_kernel_form holds the case
list to it.  The GPU tests are marked ``gpu`` one by one: the two tests about the case list and the bound run anywhere.

Run on the MI355X box with ``pytest -m gpu``.
"""
import math
from dataclasses import dataclass, replace
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from op_plan_helpers import (NAN, POISON32, assert_poison_intact, attn32_op, bits, conv32_op, conv32_record, nchw, nhwc, poisoned,
                             poisoned_blob, run_op, ulp32, view)

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from bs_yolo_amd import lib as L  # noqa: F401  (fails loudly when the .so is missing)

F32, F16, F64 = torch.float32, torch.float16, torch.float64
B, H, W = 3, 10, 14  # M = 420: three full 128-pixel tiles + 36 pixels; one full 256-pixel tile + 164
U = 2.0 ** -24       # unit roundoff of f32
TILE, BK, PATCH = "BSY_CONV32X_TILE", "BSY_CONV32X_BK", "BSY_CONV32X_PATCH"  # read by launch_conv32x_mfma at every call


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# ------------------------------------------------------------------------------------------------------------
# CONV: the layer list
# ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Layer:
    name: str
    k: int = 1
    s: int = 1
    C0: int = 32
    C1: int = 0
    up0: int = 0
    up1: int = 0
    Cout: int = 32
    res: str = ""         # "view": a shortcut view of its own; "self": the destination view (in place)
    env: tuple = ()       # ((switch, value), ...)
    off2: bool = False    # every view at channel offset 2: 8 bytes off a 16-byte boundary
    deconv: bool = False  # the four dst_scale = 2 phases of a ConvTranspose2d(C0, Cout, 2, 2)

    @property
    def K(self):
        return self.k * self.k * (self.C0 + self.C1)

    @property
    def payload(self):
        """The layer without what only places or routes it: layers with equal payloads share inputs and reference."""
        return replace(self, name="", env=(), off2=False)

    @property
    def out_hw(self):
        p = self.k // 2
        return (H + 2 * p - self.k) // self.s + 1, (W + 2 * p - self.k) // self.s + 1


def _layers():
    ls = []
    for c0, c1, u0, u1 in ((8, 24, 0, 0), (64, 32, 1, 0), (24, 8, 0, 1)):  # the second: the YOLO11 head's concat convs
        ls += [Layer("cat1x1-%d+%d-up%d%d-%d" % (c0, c1, u0, u1, co), 1, 1, c0, c1, u0, u1, co) for co in (24, 48, 136)]
    # Cin = 40, K = 360: the 32-deep K-steps straddle the taps and the source boundary
    ls += [Layer("cat3x3-s%d" % s, 3, s, 16, 24, Cout=48) for s in (1, 2)]
    for co, t in ((136, "1"), (264, "2")):  # the fp32x 256-pixel tiles, second source through its own buffer descriptor
        ls.append(Layer("big%s-1x1-%d" % (t, co), 1, 1, 64, 32, 1, 0, co, env=((TILE, t),)))
        ls.append(Layer("big%s-1x1-%d-bk16" % (t, co), 1, 1, 64, 32, 1, 0, co, env=((TILE, t), (BK, "16"))))
        ls.append(Layer("big%s-3x3-%d" % (t, co), 3, 1, 16, 24, Cout=co, env=((TILE, t),)))
    ls.append(Layer("deconv-32", C0=32, Cout=32, deconv=True))
    ls.append(Layer("deconv-136-big1", C0=32, Cout=136, deconv=True, env=((TILE, "1"),)))
    ls.append(Layer("res3x3-view", 3, 1, 32, Cout=32, res="view"))  # fp32x: the patch kernel
    ls.append(Layer("res3x3-view-nopatch", 3, 1, 32, Cout=32, res="view", env=((PATCH, "0"),)))
    ls.append(Layer("res1x1-self", 1, 1, 32, Cout=32, res="self"))  # attn.proj / ffn.1: dst = b, res = b
    # the fall-through: neither MFMA kernel takes these
    ls.append(Layer("off2-cat1x1-64+32-up10-48", 1, 1, 64, 32, 1, 0, 48, off2=True))
    ls.append(Layer("off2-res1x1-self", 1, 1, 32, Cout=32, res="self", off2=True))
    ls.append(Layer("cat1x1-cout6", 1, 1, 8, 24, Cout=6))
    ls.append(Layer("cat1x1-c0-12", 1, 1, 12, 24, Cout=24))
    return ls


LAYERS = _layers()
CONV_CASES = [(p, ly) for ly in LAYERS for p in (1, 2)]
CONV_IDS = ["prec%d-%s" % (p, ly.name) for p, ly in CONV_CASES]


def _geom(ly):
    """Row strides and channel offsets of the four operands.  Every buffer is wider than its view; aligned offsets are multiples of 4
    floats and differ between the operands, ldr != ldd."""
    o = 2 if ly.off2 else 0
    g = SimpleNamespace(c0=o or 8, ld0=ly.C0 + 16, c1=o or 16, ld1=ly.C1 + 24, cd=o or 8, ldd=ly.Cout + 16, cr=o or 4, ldr=ly.Cout + 24)
    if ly.res == "self":
        g.cr, g.ldr = g.cd, g.ldd
    return g


# ---- the routing, mirrored from the C++ (device buffers and weight records start on 256-byte boundaries) ----
def _mfma_supported(ly):
    """conv32_mfma_supported (csrc/conv32_mfma.hip) for a CONV placed by _geom."""
    g = _geom(ly)
    if ly.Cout <= 0 or ly.Cout & 3 or g.ldd & 3 or (ly.res and g.ldr & 3):
        return False
    if g.cd & 3 or (ly.res and g.cr & 3):  # ((uintptr_t)a.w | a.dst | a.res) & 15
        return False
    if ly.C0 & 7 or ly.C1 & 7 or ly.C0 <= 0 or g.ld0 & 3 or (ly.C1 and g.ld1 & 3):
        return False
    if g.c0 & 3 or (ly.C1 and g.c1 & 3):   # ((uintptr_t)a.src0 | a.src1) & 15
        return False
    if (ly.up0 or ly.up1) and (H | W) & 1:
        return False
    return True  # (the 4 GiB limits of the buffer descriptors are far away)


def route(prec, ly):
    """The kernel form run_op_f32 reaches: conv32x_mfma_supported -> launch_conv32x_mfma's choice, else launch_conv32."""
    if not _mfma_supported(ly):
        return "scalar"
    co = ly.Cout
    if prec == 1:  # launch_conv32_mfma
        return "mfma-128" if co > 64 else ("mfma-thin" if co <= 32 else "mfma-64")
    env = dict(ly.env)  # conv32x_mfma_supported adds: 16-byte aligned planes, Kpad >= K -- conv32_record's layout
    force, bk = int(env.get(TILE, -1)), int(env.get(BK, 32))
    oh, ow = ly.out_hw
    M = B * oh * ow
    patch_ok = ly.k == 3 and ly.s == 1 and not ly.C1 and not ly.up0 and not ly.deconv and ly.C0 % 16 == 0
    if patch_ok and force < 0 and int(env.get(PATCH, 1)) != 0:
        return "patch"
    big, ptiles = 0, (M + 255) // 256
    if co >= 256 and ptiles * math.ceil(co / 256) >= 128:
        big = 2
    elif co >= 128 and ptiles * math.ceil(co / 128) >= 128:
        big = 1
    if force >= 0:
        big = (2 if co >= 256 else (1 if co >= 128 else 0)) if force == 2 else ((1 if co >= 128 else 0) if force == 1 else 0)
    if big:
        return "x-big%d-bk%d" % (256 if big == 2 else 128, 16 if bk == 16 else 32)
    return "x-128" if co > 64 else ("x-thin" if co <= 32 else "x-64")


def test_case_list_reaches_every_kernel_form():
    """Every form of the three conv files runs on two sources at least once (the patch kernel takes one source by its rule), the
    shortcut cases reach the patch kernel and the thin tile, the dst_scale cases a 256-pixel tile, and the fall-through cases the
    scalar kernel in both modes."""
    two = {route(p, ly) for p, ly in CONV_CASES if ly.C1}
    want = {"scalar", "mfma-thin", "mfma-64", "mfma-128", "x-thin", "x-64", "x-128", "x-big128-bk16", "x-big128-bk32", "x-big256-bk16",
            "x-big256-bk32"}
    assert want <= two, sorted(want - two)
    by = {ly.name: ly for ly in LAYERS}
    assert route(2, by["res3x3-view"]) == "patch" and route(2, by["res3x3-view-nopatch"]) == "x-thin"
    assert route(2, by["deconv-136-big1"]) == "x-big128-bk32" and route(1, by["deconv-136-big1"]) == "mfma-128"
    for n in ("off2-cat1x1-64+32-up10-48", "off2-res1x1-self", "cat1x1-cout6", "cat1x1-c0-12"):
        assert route(1, by[n]) == route(2, by[n]) == "scalar"
    for ly in LAYERS:
        assert ly.K <= 360 and (not (ly.up0 or ly.up1) or (H % 2 == 0 and W % 2 == 0))
        if ly.off2:
            assert route(1, replace(ly, off2=False)) != "scalar"


# ------------------------------------------------------------------------------------------------------------
# payloads, fp64 references and the bound
# ------------------------------------------------------------------------------------------------------------
def _reference(lin, xs, w, b, res, act, K):
    """fp64 evaluation of y = act(lin(xs, w, b)) + res and, for act = SiLU, the two error bounds per output element.  lin is linear in
    (xs, b) and in (w, b); with S = |b| + sum |x_i| |w_i| over the taps inside the map, v the pre-activation:

      prec 1:  1.1 (K + 1) 2^-24 S  +  8 * 2^-24 |silu(v)|  +  2^-24 |y|
               the order-independent bound of a length-K fp32 sum that starts at the bias (K + 1 roundings, gamma_n <= 1.1 n u
               here), carried through SiLU, whose slope lies in (-0.1, 1.1); x / (1 + expf(-x)); the rounding of the shortcut add.
      prec 2:  that + 2^-20 S + 2^-25 (sum |w_i| + sum |x_i|)
               four times 2^-22 for the pixel split, the weight split, the dropped lo * lo product and one spare; an absolute 2^-25
               per operand whose lo part falls into f16's subnormal range."""
    d = lambda t: None if t is None else t.to(F64)
    xs64, w64, b64 = tuple(d(x) for x in xs), d(w), d(b)
    v = lin(xs64, w64, b64)
    y = F.silu(v) if act else v
    if res is not None:
        y = y + d(res)
    out = SimpleNamespace(xs=xs, w=w, b=b, res=res, act=act, K=K, lin=lin, ref=y, b1=None, b2=None)
    if act:
        ab = lambda t: None if t is None else t.abs()
        one = lambda t: None if t is None else torch.ones_like(t)
        zero = torch.zeros_like(b64)
        S = lin(tuple(ab(x) for x in xs64), w64.abs(), b64.abs())
        sw = lin(tuple(one(x) for x in xs64), w64.abs(), zero)
        sx = lin(tuple(ab(x) for x in xs64), torch.ones_like(w64), zero)
        out.b1 = 1.1 * (K + 1) * U * S + 8 * U * F.silu(v).abs() + U * y.abs()
        out.b2 = out.b1 + 2.0 ** -20 * S + 2.0 ** -25 * (sw + sx)
    else:  # integer payload: exact in fp64, and every partial sum an integer below 2^24
        assert bool((y == y.round()).all())
        S = lin(tuple(None if x is None else x.abs() for x in xs64), w64.abs(), b64.abs())
        assert float(S.max()) + 8 < 2 ** 24
        out.ref = y + 0.0  # no kernel returns -0 here: the chains start at a +0 or non-zero bias
    return out


def _conv_lin(ly):
    def lin(xs, w, b):
        if ly.deconv:
            return nhwc(F.conv_transpose2d(nchw(xs[0]), w, b, stride=2))
        maps = [F.interpolate(nchw(x), scale_factor=2.0, mode="nearest") if up else nchw(x)
                for x, up in zip(xs, (ly.up0, ly.up1)) if x is not None]
        return nhwc(F.conv2d(torch.cat(maps, 1), w, b, ly.s, ly.k // 2))
    return lin


@lru_cache(maxsize=None)
def _conv_case(pl, kind):
    """Inputs and reference of a layer payload (Layer.payload), drawn once.  "int": inputs in [-8, 8], weights in [-4, 4], integer bias
    and shortcut, no activation.  "rand": randn inputs with every third channel scaled by 1e-3 (lo parts in f16's subnormal range),
    weights randn * sqrt(2 / K), bias randn / 2, shortcut randn, SiLU."""
    g = _gen(pl.k, pl.s, pl.C0, pl.C1, pl.up0, pl.up1, pl.Cout, len(pl.res), pl.deconv, kind == "int")
    oh, ow = pl.out_hw
    shapes = [(B, H >> pl.up0, W >> pl.up0, pl.C0), (B, H >> pl.up1, W >> pl.up1, pl.C1) if pl.C1 else None]
    wshape = (pl.C0, pl.Cout, 2, 2) if pl.deconv else (pl.Cout, pl.C0 + pl.C1, pl.k, pl.k)
    rshape = (B, oh, ow, pl.Cout) if pl.res else None
    if kind == "int":
        draw = lambda shp, lim: torch.randint(-lim, lim + 1, shp, generator=g).float()
        xs = tuple(None if s is None else draw(s, 8) for s in shapes)
        w, b = draw(wshape, 4), draw((pl.Cout,), 8)
        res = draw(rshape, 8) if rshape else None
    else:
        xs = []
        for s in shapes:
            x = None if s is None else torch.randn(s, generator=g)
            if x is not None:
                x[..., ::3] *= 1e-3
            xs.append(x)
        xs = tuple(xs)
        w, b = torch.randn(wshape, generator=g) * (2.0 / pl.K) ** 0.5, torch.randn(pl.Cout, generator=g) * 0.5
        res = torch.randn(rshape, generator=g) if rshape else None
    return _reference(_conv_lin(pl), xs, w, b, res, kind != "int", pl.K)


def _worst(got, ref, bound):
    """worst |got - ref| / bound; inf when got is not finite (a NaN from outside a view or between the weight parts reached it)."""
    got = got.to(F64)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - ref).abs() / bound).max())


def _set_env(monkeypatch, env):
    for n in (TILE, BK, PATCH):
        monkeypatch.delenv(n, raising=False)
    for n, v in env:
        monkeypatch.setenv(n, v)


PHASES = ((0, 0), (0, 1), (1, 0), (1, 1))


def _run_conv(prec, ly, c, monkeypatch, phases=PHASES):
    """The layer as one-op plans (a deconv: one per phase in `phases`, each with its own weight record cut as weights.pack_record cuts a
    "deconv" record) on poisoned views -> (destination payload on the host, the whole destination buffer)."""
    _set_env(monkeypatch, ly.env)
    g = _geom(ly)
    oh, ow = ly.out_hw
    sc = 2 if ly.deconv else 1
    s0 = poisoned((B, H >> ly.up0, W >> ly.up0, g.ld0), g.c0, ly.C0, c.xs[0], NAN)
    s1 = poisoned((B, H >> ly.up1, W >> ly.up1, g.ld1), g.c1, ly.C1, c.xs[1], NAN) if ly.C1 else None
    dst = poisoned((B, oh * sc, ow * sc, g.ldd), g.cd, ly.Cout, c.res if ly.res == "self" else None, POISON32, dtype=F32)
    rbuf = poisoned((B, oh, ow, g.ldr), g.cr, ly.Cout, c.res, NAN) if ly.res == "view" else None
    vres = {"": None, "self": view(2, g.ldd, g.cd, ly.Cout), "view": view(3, g.ldr, g.cr, ly.Cout)}[ly.res]
    if ly.deconv:
        recs = [(dy, dx, c.w[:, :, dy, dx].t().contiguous()[:, :, None, None]) for dy, dx in phases]
    else:
        recs = [(0, 0, c.w)]
    arrays = []
    for _, _, wp in recs:
        arrays += conv32_record(wp, c.b, prec)
    blob, offs = poisoned_blob(arrays)
    for i, (dy, dx, _) in enumerate(recs):
        op = conv32_op(prec, B, H, W, ly.k, ly.s, ly.k // 2, view(0, g.ld0, g.c0, ly.C0), view(2, g.ldd, g.cd, ly.Cout), offs[2 * i],
                       offs[2 * i + 1], src1=view(1, g.ld1, g.c1, ly.C1) if ly.C1 else None, up0=ly.up0, up1=ly.up1, res=vres,
                       act=int(c.act), dst_scale=sc, dst_dy=dy, dst_dx=dx)
        run_op(op, [s0, s1, dst, rbuf], blob)
    assert_poison_intact(dst, g.cd, ly.Cout, POISON32)
    return dst[..., g.cd:g.cd + ly.Cout].cpu(), dst


# ------------------------------------------------------------------------------------------------------------
# 1. CONV, integer payloads: bit for bit in both modes
# ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("prec,ly", CONV_CASES, ids=CONV_IDS)
def test_conv_integers_bit_for_bit(prec, ly, monkeypatch):
    """Integers (in fp32x: hi = x, lo = 0 exactly) leave one right answer whatever the kernel and its summation order: a wrong row
    stride, source boundary, upsampling shift, phase or shortcut index changes bits.  A deconv layer runs its four phases into one
    (B, 2H, 2W) view and is compared with F.conv_transpose2d."""
    c = _conv_case(ly.payload, "int")
    got, _ = _run_conv(prec, ly, c, monkeypatch)
    assert torch.equal(bits(got), bits(c.ref.to(F32))), route(prec, ly)


@gpu
@pytest.mark.parametrize("prec", [1, 2])
def test_conv_single_phase_touches_only_its_pixels(prec, monkeypatch):
    """dst_scale = 2 with (dy, dx) = (1, 0): only the pixels (2i + 1, 2j) of the view change, and they hold the phase's 1x1 conv."""
    ly = next(l for l in LAYERS if l.name == "deconv-32")
    c = _conv_case(ly.payload, "int")
    got, _ = _run_conv(prec, ly, c, monkeypatch, phases=((1, 0),))
    want = torch.full_like(got, POISON32)
    want[:, 1::2, 0::2] = c.ref.to(F32)[:, 1::2, 0::2]
    assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------------------------
# 2. CONV, random payloads with SiLU: fp64 under the derived bound
# ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("prec,ly", CONV_CASES, ids=CONV_IDS)
def test_conv_random_within_derived_bound(prec, ly, monkeypatch):
    """|got - fp64| <= the bound of _reference for the mode the case runs in (a prec 2 case that falls through to the exact kernels: the
    prec 1 bound).  The misaligned placements must return the aligned run's bits in prec 1: scalar = MFMA on two sources, upsampling
    and the in-place shortcut."""
    c = _conv_case(ly.payload, "rand")
    form = route(prec, ly)
    got, _ = _run_conv(prec, ly, c, monkeypatch)
    r = _worst(got, c.ref, c.b2 if form.startswith(("x-", "patch")) else c.b1)
    print("conv prec %d %s [%s]: worst error / bound = %.3f" % (prec, ly.name, form, r))
    assert r <= 1.0
    if ly.off2 and prec == 1:
        twin = replace(ly, off2=False)
        assert route(1, twin).startswith("mfma")
        aligned, _ = _run_conv(1, twin, c, monkeypatch)
        assert torch.equal(bits(got), bits(aligned))


# ------------------------------------------------------------------------------------------------------------
# 3. CONV_FIRST
# ------------------------------------------------------------------------------------------------------------
FH, FW = 14, 22  # 3x3 / 6x6 stride 2: 7 x 11 outputs, M = 231 (ragged against the 128-pixel tile)
# launch_first switches on ceil(Cout / 32) = 1, 2, 3, >= 4: 16, 48, 80, 128
FIRST_CASES = [(3, 1, co) for co in (16, 48, 80, 128)] + [(6, 2, 16)]
FIRST_GRID = [(p, dt, k, pad, co) for p in (1, 2) for dt in (F16, F32) for k, pad, co in FIRST_CASES]
FIRST_IDS = ["prec%d-%s-%dx%d-%d" % (p, "f16" if dt == F16 else "f32", k, k, co) for p, dt, k, pad, co in FIRST_GRID]


@lru_cache(maxsize=None)
def _first_case(k, pad, cout, dt, kind):
    """"int": an image of 0 .. 255 (exact in f16), weights in [-2, 2], integer bias, no activation.  "rand": a rand image rounded to
    `dt`, weights randn * sqrt(2 / K), bias randn / 2, SiLU."""
    g = _gen(k, pad, cout, dt == F16, kind == "int")
    K = 3 * k * k
    if kind == "int":
        img = torch.randint(0, 256, (B, 3, FH, FW), generator=g).to(dt)
        w = torch.randint(-2, 3, (cout, 3, k, k), generator=g).float()
        b = torch.randint(-8, 9, (cout,), generator=g).float()
    else:
        img = torch.rand(B, 3, FH, FW, generator=g).to(dt)
        w, b = torch.randn(cout, 3, k, k, generator=g) * (2.0 / K) ** 0.5, torch.randn(cout, generator=g) * 0.5
    return _reference(lambda xs, w_, b_: nhwc(F.conv2d(xs[0], w_, b_, 2, pad)), (img,), w, b, None, kind != "int", K)


def _first_supported(prec, k, cout, cd):
    """The image-conv branches of conv32x_mfma_supported / conv32_mfma_supported for a destination of cout + 16 floats per row."""
    exact = cout % 4 == 0 and (cout + 16) % 4 == 0 and cd % 4 == 0
    return ("x-first" if prec == 2 and exact and k == 3 and cout <= 128 else "mfma-first") if exact else "scalar"


def _run_first(prec, k, pad, cout, c, cd=8):
    ldd = cout + 16
    oh, ow = (FH + 2 * pad - k) // 2 + 1, (FW + 2 * pad - k) // 2 + 1
    img = c.xs[0].to("cuda:0")
    dst = poisoned((B, oh, ow, ldd), cd, cout, None, POISON32, dtype=F32)
    blob, offs = poisoned_blob(conv32_record(c.w, c.b, prec))
    op = conv32_op(prec, B, FH, FW, k, 2, pad, view(0, 3, 0, 3), view(1, ldd, cd, cout), offs[0], offs[1], act=int(c.act),
                   in_dtype=L.BSY_F16 if img.dtype == F16 else L.BSY_F32, first=True)
    run_op(op, [img, dst], blob)
    assert_poison_intact(dst, cd, cout, POISON32)
    return dst[..., cd:cd + cout].cpu()


@gpu
@pytest.mark.parametrize("prec,dt,k,pad,cout", FIRST_GRID, ids=FIRST_IDS)
def test_conv_first_integers_bit_for_bit(prec, dt, k, pad, cout):
    c = _first_case(k, pad, cout, dt, "int")
    assert torch.equal(bits(_run_first(prec, k, pad, cout, c)), bits(c.ref.to(F32)))


@gpu
@pytest.mark.parametrize("prec,dt,k,pad,cout", FIRST_GRID, ids=FIRST_IDS)
def test_conv_first_random_within_derived_bound(prec, dt, k, pad, cout):
    """The bounds of _reference with K = 27 (108 for the 6x6 stem of YOLOv5u, which fp32x hands to the exact image kernel)."""
    c = _first_case(k, pad, cout, dt, "rand")
    form = _first_supported(prec, k, cout, 8)
    r = _worst(_run_first(prec, k, pad, cout, c), c.ref, c.b2 if form == "x-first" else c.b1)
    print("conv_first prec %d %s %dx%d cout %d [%s]: worst error / bound = %.3f" % (prec, dt, k, k, cout, form, r))
    assert r <= 1.0


@gpu
@pytest.mark.parametrize("dt", [F16, F32], ids=["f16", "f32"])
def test_conv_first_6x6_fp32x_is_the_exact_kernel(dt):
    c = _first_case(6, 2, 16, dt, "rand")
    assert _first_supported(2, 6, 16, 8) == "mfma-first"
    assert torch.equal(bits(_run_first(2, 6, 2, 16, c)), bits(_run_first(1, 6, 2, 16, c)))


@gpu
@pytest.mark.parametrize("dt", [F16, F32], ids=["f16", "f32"])
def test_conv_first_misaligned_destination_equals_aligned(dt):
    """A destination view at channel offset 2 takes the scalar kernel (both modes) and returns the exact MFMA kernel's bits."""
    c = _first_case(3, 1, 16, dt, "rand")
    assert _first_supported(1, 3, 16, 2) == _first_supported(2, 3, 16, 2) == "scalar"
    aligned = _run_first(1, 3, 1, 16, c)
    for prec in (1, 2):
        got = _run_first(prec, 3, 1, 16, c, cd=2)
        assert torch.equal(bits(got), bits(aligned)), prec
    assert _worst(aligned, c.ref, c.b1) <= 1.0


# ------------------------------------------------------------------------------------------------------------
# the bound on the CPU
# ------------------------------------------------------------------------------------------------------------
def test_cpu_float32_within_half_the_bound():
    """A float32 evaluation of every random case by torch on the CPU (another summation order than either kernel's) stays within
    half of the prec 1 bound: the bound passes a correct fp32 implementation with room to spare."""
    cases = [_conv_case(pl, "rand") for pl in dict.fromkeys(ly.payload for ly in LAYERS)]
    cases += [_first_case(k, pad, co, dt, "rand") for dt in (F16, F32) for k, pad, co in FIRST_CASES]
    worst = 0.0
    for c in cases:
        y = F.silu(c.lin(tuple(None if x is None else x.float() for x in c.xs), c.w, c.b))
        if c.res is not None:
            y = y + c.res
        assert y.dtype == F32
        worst = max(worst, _worst(y, c.ref, c.b1))
    print("CPU float32: worst error / prec 1 bound = %.3f over %d cases" % (worst, len(cases)))
    assert worst <= 0.5


# ------------------------------------------------------------------------------------------------------------
# 4. ATTN
# ------------------------------------------------------------------------------------------------------------
AB, HEADS = 2, 2
ATTN_HW = {37: (1, 37), 129: (3, 43), 260: (13, 20), 64: (8, 8)}  # a ragged key tile; one query past 128; two 256-query blocks
ATTN_TOL = {1: 1e-5, 2: 3e-6}  # of the output range: test_attention32_tiled_equals_generic / test_attention32x_matches_fp64_softmax_attention


@lru_cache(maxsize=None)
def _attn_case(N, kd, hd, qscale):
    g = _gen(N, kd, hd, qscale)
    qkv = torch.randn(AB, N, HEADS * (2 * kd + hd), generator=g)
    qkv[..., :HEADS * kd] *= qscale
    return SimpleNamespace(qkv=qkv, ref=_attn_ref(qkv, kd, hd))


def _attn_ref(qkv, kd, hd):
    """Softmax attention in fp64 on the [q | k | v]-by-heads layout of the ATTN op."""
    N = qkv.shape[1]
    x = qkv.double()
    q = x[..., :HEADS * kd].view(AB, N, HEADS, kd).permute(0, 2, 1, 3)
    k = x[..., HEADS * kd:2 * HEADS * kd].view(AB, N, HEADS, kd).permute(0, 2, 1, 3)
    v = x[..., 2 * HEADS * kd:].view(AB, N, HEADS, hd).permute(0, 2, 1, 3)
    return (torch.softmax((q @ k.transpose(-1, -2)) * kd ** -0.5, -1) @ v).permute(0, 2, 1, 3).reshape(AB, N, HEADS * hd)


def _run_attn(prec, qkv, kd, hd, cs=8, cd=8):
    """qkv in channels [cs, cs + C) of rows of C + 24 floats of NaN, the output in [cd, cd + heads * hd) of rows of heads * hd + 16."""
    N, Cq, Co = qkv.shape[1], qkv.shape[2], HEADS * hd
    h, w = ATTN_HW[N]
    lds, ldo = Cq + 24, Co + 16
    src = poisoned((AB, h, w, lds), cs, Cq, qkv.view(AB, h, w, Cq), NAN)
    dst = poisoned((AB, h, w, ldo), cd, Co, None, POISON32, dtype=F32)
    run_op(attn32_op(prec, AB, h, w, view(0, lds, cs, Cq), view(1, ldo, cd, Co), HEADS, kd, hd, kd ** -0.5), [src, dst])
    assert_poison_intact(dst, cd, Co, POISON32)
    return dst[..., cd:cd + Co].cpu().view(AB, N, Co)


def _attn_ratio(got, ref, prec):
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float((got.double() - ref).abs().max()) / (ATTN_TOL[prec] * max(float(ref.abs().max()), 1.0))


@gpu
@pytest.mark.parametrize("prec", [1, 2])
@pytest.mark.parametrize("qscale", [1, 3])
@pytest.mark.parametrize("N", [37, 129, 260])
def test_attention_matches_fp64(N, qscale, prec):
    """kd / hd = 32 / 64 on aligned views: the tiled exact kernel (prec 1), attention32x_kernel (prec 2).  q scaled by 3 makes the
    softmax peaky, so the running maximum moves from tile to tile."""
    c = _attn_case(N, 32, 64, qscale)
    r = _attn_ratio(_run_attn(prec, c.qkv, 32, 64), c.ref, prec)
    print("attn prec %d N %d q x %d: worst error / bound = %.3f" % (prec, N, qscale, r))
    assert r <= 1.0


@gpu
@pytest.mark.parametrize("N", [37, 129, 260])
def test_attention_misaligned_views_take_the_generic_kernel(N):
    """qkv and the destination at channel offset 2: attn32_kernel in both modes.  prec 1 must return the aligned (tiled) run's bits,
    prec 2 the same bits again."""
    c = _attn_case(N, 32, 64, 3)
    aligned = _run_attn(1, c.qkv, 32, 64)
    got1, got2 = (_run_attn(p, c.qkv, 32, 64, cs=2, cd=2) for p in (1, 2))
    assert torch.equal(bits(got1), bits(aligned)) and torch.equal(bits(got2), bits(got1))
    assert _attn_ratio(got1, c.ref, 1) <= 1.0


@gpu
def test_attention_16_32_takes_the_generic_kernel_in_both_modes():
    c = _attn_case(37, 16, 32, 1)
    got1, got2 = (_run_attn(p, c.qkv, 16, 32) for p in (1, 2))
    assert torch.equal(bits(got2), bits(got1))
    r = _attn_ratio(got1, c.ref, 1)
    print("attn 16/32 N 37: worst error / bound = %.3f" % r)
    assert r <= 1.0


@gpu
@pytest.mark.parametrize("prec", [1, 2])
def test_attention_uniform_softmax_is_the_mean(prec):
    """All keys of a head equal: every logit of a query is the same, the softmax is 1 / 64 exactly and each output the mean of 64
    integers -- exact in fp32.  Within 2 ulp32 instead of a share of the range."""
    g = _gen(64, prec)
    kd, hd, N = 32, 64, 64
    qkv = torch.randn(AB, N, HEADS * (2 * kd + hd), generator=g)
    qkv[..., HEADS * kd:2 * HEADS * kd] = torch.randn(AB, 1, HEADS * kd, generator=g)
    v = torch.randint(-8, 9, (AB, N, HEADS * hd), generator=g).float()
    qkv[..., 2 * HEADS * kd:] = v
    ref = v.double().mean(1, keepdim=True).expand(AB, N, HEADS * hd)
    got = _run_attn(prec, qkv, kd, hd).double()
    assert bool(torch.isfinite(got).all())
    assert bool(((got - ref).abs().numpy() <= 2 * ulp32(ref.numpy())).all()), float((got - ref).abs().max())


# ------------------------------------------------------------------------------------------------------------
# 5. refusals (host-side, before any launch)
# ------------------------------------------------------------------------------------------------------------
def _plain_conv(prec):
    ly = Layer("refuse", 1, 1, 8, 24, Cout=24)
    c = _conv_case(ly.payload, "int")
    g = _geom(ly)
    s0 = poisoned((B, H, W, g.ld0), g.c0, ly.C0, c.xs[0], NAN)
    s1 = poisoned((B, H, W, g.ld1), g.c1, ly.C1, c.xs[1], NAN)
    dst = poisoned((B, H, W, g.ldd), g.cd, ly.Cout, None, POISON32, dtype=F32)
    blob, offs = poisoned_blob(conv32_record(c.w, c.b, 2))
    op = conv32_op(prec, B, H, W, 1, 1, 0, view(0, g.ld0, g.c0, ly.C0), view(2, g.ldd, g.cd, ly.Cout), offs[0], offs[1],
                   src1=view(1, g.ld1, g.c1, ly.C1))
    return op, [s0, s1, dst], blob, (g.cd, ly.Cout)


@gpu
@pytest.mark.parametrize("what", ["out_f32=2,prec=1", "out_f32=3,prec=2", "src1 unbound,prec=1", "src1 unbound,prec=2", "prec=3"])
def test_refusals(what):
    prec = 3 if what == "prec=3" else int(what[-1])
    op, ext, blob, (cd, co) = _plain_conv(prec)
    if what.startswith("out_f32"):
        op.out_f32 = int(what[8])
    if what.startswith("src1"):
        ext[1] = None
    with pytest.raises(L.BsyError):
        run_op(op, ext, blob)
    assert_poison_intact(ext[2], cd, 0, POISON32)  # nothing ran: the whole destination still holds the poison
