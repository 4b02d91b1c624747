"""The image and fused block ops ALONE: BSY_OP_CONV_FIRST (csrc/conv_first.hip), BSY_OP_STEM (csrc/stem_fused.hip), BSY_OP_BNECK
(csrc/bneck_fused.hip) and BSY_OP_C3K2 (csrc/c3k2_fused.hip) with prec 0 as one-op plans (op_plan_helpers.conv_first16_op, stem_op,
bneck_op, c3k2_op, run_ops), fields as Plan._emit sets them and build_conv_first / build_stem / build_bneck / build_c3k2
(csrc/op_args.h) read them.  Every tensor is an external slot.

Poison.  The image is a whole tensor cut out of a larger f16 / f32 NaN allocation with at least one image row of NaN on either side
(poisoned_image): a halo read outside the image reaches the output.  Sources are channel views of f16 NaN buffers with ld > C, the
weight records lie in one blob with NaN behind every record (conv16_records), destinations are views coff > 0, ld > coff + C of
buffers filled with 777, compared bit for bit outside the view after every run.  BNECK also runs in the planner's own placement:
source = channels [c, 2c) and destination = [2c, 3c) of ONE buffer, everything outside the destination bit-identical to before.

Comparison 1, dyadic payloads with act = 0 (CONV_FIRST, STEM, BNECK: `if (p.act)` at every epilogue, never run before).  Without SiLU
the ops are linear.  Inputs are multiples of 1/8, the first conv of an op has weights in {-1, 0, 1} and a bias in eighths (its map: a
multiple of 1/8), the second one weights in {-1/4, 0, 1/4} and a bias in 1/32; the 3x3 convs over 144 .. 576 products are sparse.
Asserted on the CPU (test_payloads_are_exact_and_cases_reach_every_edge): every intermediate map and every result is a multiple of
2^-5 below 64 in magnitude and every sum |x||w| 2^5 < 2^24 -- so every value is exact in f32 in ANY summation order and exact in f16:
there is one right answer, it is computed in fp64 and compared bit for bit, and it depends neither on the unfused kernels nor on
image_conv.h.  The values differ per tap and per channel and the image and map borders are non-zero.

Comparison 2, random payloads with act = 1 (all four kinds; `randn` inputs, `rand` images, weights randn sqrt(2 / K) rounded to f16,
bias 0.2 randn).
  a. the contract: the fused op returns bit for bit what the chain of plain ops returns on the same poisoned blob and views, run as a
     plan under the heuristic configuration --
       STEM  = CONV_FIRST into an f16 map, then CONV 3x3 s2;
       BNECK = CONV 3x3, then CONV 3x3 with res = the source view;
       C3K2  = CONV 1x1 into channels [0, 2c) of a 3c concat buffer, BNECK on [c, 2c) -> [2c, 3c), CONV 1x1 over the buffer
               (and that BNECK stage again equals its own two-CONV chain on the y1 map read back);
  b. the bound: every stage of the chain lies within op_plan_helpers._bound of an fp64 evaluation whose INPUT is that stage's input
     read back from the GPU, so no bound is carried through an f16 rounding: 1.1 (K + 1) 2^-24 S + 8 2^-24 |a|, plus half an f16 ulp of
     y.  Rounding forms, read from the kernels: conv_first.hip, both stem epilogues, the 1x1 convs and both hidden maps round
     f16(SiLU(v)) once, no shortcut; the second conv of a Bottleneck rounds TWICE -- `(half)((float)(half)SiLU(v) + x)` in
     bneck_fused.hip (both kernels) and c3k2_fused.hip's S3, as conv_epilogue_lds and the patch kernel do -- so that stage is allowed
     half an f16 ulp of a more.  K = 27 for the image conv, whose reference takes the image rounded to f16 (round to nearest even, what
     the kernel parks: a truncating conversion of an f32 image would miss the bound by orders of magnitude).
test_cpu_float32_within_half_the_bound shows that a float32 evaluation on the CPU uses at most half of the arithmetic part.

The persistent walk (xcd_tile_walk, make_tile_grid of csrc/common.h).  The launchers cap the grid at 768 (stem f16, narrow Bottleneck,
C3k2), 512 (stem f32) and 256 (wide Bottleneck) workgroups.  One case per kernel has at least 2.5 x cap tiles, ALL inside a map (H and
W multiples of the tile, at least two tiles per side), a tile count that is no multiple of 8 (the remainder branch of the walk) and
more tiles per image than a workgroup's step cap / 8, so that fetch(tile + tw.step) continues inside the image it is in.  The case ids
carry tile count and cap.  One more case per kernel has 4 tiles (X = G < 8).

The GPU tests are marked ``gpu`` one by one: the two tests about the payloads and the bound run anywhere.

Run on the MI355X box with ``pytest -m gpu``.
"""
from dataclasses import dataclass, replace
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from op_plan_helpers import (DEV, NAN, POISON16, _bound, _worst, assert_outside_views_intact, assert_poison_intact, bits, bneck_op, c3k2_op,
                             conv1x1_op, conv16_op, conv16_records, conv_first16_op, nchw, nhwc, poisoned, poisoned_image, run_ops,
                             stem_op, view)

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from bs_yolo_amd import lib as L  # noqa: F401  (fails loudly when the .so is missing)

F32, F16, F64 = torch.float32, torch.float16, torch.float64
TILE = {"first": (4, 64), "stem": (4, 16), "bneck": (8, 16), "c3k2": (4, 16)}  # output tile of each kernel


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 15485863 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# ------------------------------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    kind: str            # "first" | "stem" | "bneck" | "c3k2"
    name: str
    B: int
    H: int               # first / stem: the image; bneck / c3k2: the map
    W: int
    widths: tuple        # first: (Cout,); stem: (C0, C1); bneck: (C, hidden); c3k2: (Cin, c, C2)
    idt: torch.dtype = F16  # first / stem: the image's dtype
    place: str = "sep"   # bneck: "one" = source [c, 2c) and destination [2c, 3c) of one buffer; "sep" = two buffers, ld differ
    mis: int = 0         # first: the image's first element lies this many elements past a 16-byte boundary
    walk: bool = False   # a persistent-walk case: random payload against the chain only

    @property
    def out_hw(self):
        """The op's output map (first: layer 0; stem: layer 1)."""
        h, w = self.H, self.W
        for _ in range({"first": 1, "stem": 2}.get(self.kind, 0)):
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        return h, w

    @property
    def cap(self):
        """The launcher's grid cap (launch_stem_fused, launch_bneck_fused, launch_c3k2_fused); conv_first is not persistent."""
        if self.kind == "stem":
            return 512 if self.idt == F32 else 768
        return {"bneck": 256 if self.widths[0] == 64 else 768, "c3k2": 768}.get(self.kind)

    @property
    def tiles(self):
        """make_tile_grid: (tiles per image, tiles) -- each side padded to two tiles."""
        th, tw = TILE[self.kind]
        oh, ow = self.out_hw
        per = max(2, -(-oh // th)) * max(2, -(-ow // tw))
        return per, self.B * per

    @property
    def payload(self):
        """What the operands depend on: cases with equal payloads share them and their references."""
        return (self.kind, self.B, self.H, self.W, self.widths)

    @property
    def exact(self):
        return self.kind != "c3k2"  # the C3k2 kernel has no act = 0 form


def _dt(dt):
    return "f16" if dt == F16 else "f32"


def _walk(kind, B, H, W, widths, idt=F16, tag=""):
    cs = Case(kind, "", B, H, W, widths, idt, walk=True)
    return replace(cs, name="walk-%s%s-%dx%dx%d-%dtiles-cap%d" % (kind, tag, B, H, W, cs.tiles[1], cs.cap))


def _cases():
    cs = []
    # CONV_FIRST, output tile 4 x 64.  22 x 140 -> 11 x 70: ragged row and column tiles; Cout 8 .. 128: NT 1 .. 4, the cc >= Cout guard
    # at 8 and 48.  22 x 70 and 9 x 37: W % 4 = 2 and 1, the element-wise load with f16 rows on 2-byte alignment, here with NT = 3 and 4
    # and a Cout that is no multiple of 32.  mis = 1: the element-wise load chosen by the pointer.  1 x 1 and 3 x 5: smaller than a tap row
    for dt in (F16, F32):
        for co in (8, 32, 48, 96, 128):
            cs.append(Case("first", "first-%s-22x140-c%d" % (_dt(dt), co), 2, 22, 140, (co,), dt))
        cs.append(Case("first", "first-%s-22x70-c72" % _dt(dt), 2, 22, 70, (72,), dt))
        cs.append(Case("first", "first-%s-9x37-c104" % _dt(dt), 3, 9, 37, (104,), dt))
        cs.append(Case("first", "first-%s-22x140-c48-mis1" % _dt(dt), 2, 22, 140, (48,), dt, mis=1))
        cs.append(Case("first", "first-%s-1x1-c32" % _dt(dt), 2, 1, 1, (32,), dt))
        cs.append(Case("first", "first-%s-3x5-c32" % _dt(dt), 3, 3, 5, (32,), dt))
    # STEM, tile 4 x 16 layer-1 pixels = 16 x 64 image pixels.  37 x 52: odd H (layer 0: 19 rows, layer 1: 10); 4 x 4: the minimum; 16 x 132:
    # OW1 = 33, one column into a third tile
    for dt in (F16, F32):
        for wd in ((32, 64), (16, 32)):
            for h, w in ((38, 52), (37, 52), (4, 4), (7, 8), (70, 36), (16, 132)):
                cs.append(Case("stem", "stem-%s-%d-%d-%dx%d" % (_dt(dt), wd[0], wd[1], h, w), 2, h, w, wd, dt))
    cs.append(_walk("stem", 19, 240, 448, (32, 64), F16, "-f16"))   # 19 x 15 x 7 tiles
    cs.append(_walk("stem", 18, 240, 320, (16, 32), F32, "-f32"))   # 18 x 15 x 5
    cs.append(Case("stem", "stem-f16-32-64-1x8x8-4tiles", 1, 8, 8, (32, 64), F16))
    # BNECK, tile 8 x 16.  17 x 33: one row and one column into a new tile, tiles_x = 3 (a non-power-of-two magic)
    for wd in ((32, 16), (64, 32)):
        for h, w in ((3, 5), (9, 13), (17, 33)):
            for place in ("one", "sep"):
                cs.append(Case("bneck", "bneck-%d-%d-%dx%d-%s" % (wd[0], wd[1], h, w, place), 3 if (h, w) == (9, 13) else 2, h, w, wd, place=place))
        cs.append(Case("bneck", "bneck-%d-%d-1x3x5-4tiles" % wd, 1, 3, 5, wd, place="one"))
    cs.append(_walk("bneck", 19, 120, 112, (32, 16), tag="-narrow"))  # 19 x 15 x 7
    cs.append(_walk("bneck", 15, 72, 80, (64, 32), tag="-wide"))      # 15 x 9 x 5
    # C3K2, tile 4 x 16; source on channels [8, 72) of ld 80, destination on [16, 144) of ld 168
    for b, h, w in ((2, 3, 5), (3, 9, 13), (2, 5, 33)):
        cs.append(Case("c3k2", "c3k2-%dx%d" % (h, w), b, h, w, (64, 32, 128)))
    cs.append(Case("c3k2", "c3k2-1x3x5-4tiles", 1, 3, 5, (64, 32, 128)))
    cs.append(_walk("c3k2", 19, 60, 112, (64, 32, 128)))              # 19 x 15 x 7
    return cs


CASES = _cases()
EXACT = [cs for cs in CASES if cs.exact]
_ids = lambda cases: [cs.name for cs in cases]  # noqa: E731


# ------------------------------------------------------------------------------------------------------------
# payloads and fp64 references
# ------------------------------------------------------------------------------------------------------------
def _stage(x, w, b, s, act, res=None):
    """One conv of a chain in fp64: x (B, C, H, W) = the values the kernel reads, w (Cout, C, k, k), stride s, padding k // 2, `res`
    (B, OH, OW, Cout) the shortcut -> v (pre-activation), a = act(v), ref = a + res, S = |b| + sum |x||w| over the taps inside the
    map, all (B, OH, OW, Cout); K = the length of the sum."""
    x, w, b, p = x.to(F64), w.to(F64), b.to(F64), w.shape[-1] // 2
    v = nhwc(F.conv2d(x, w, b, s, p))
    a = F.silu(v) if act else v
    ref = a + res.to(F64) if res is not None else a
    S = nhwc(F.conv2d(x.abs(), w.abs(), b.abs(), s, p))
    return SimpleNamespace(v=v, a=a, ref=ref, S=S, act=act, res=res, K=w[0].numel(), nsl=1, out_f32=False)


def _border_nonzero(x, hdim, wdim, val):
    """Zeros on the border of the map are replaced by `val`: a shifted or transposed tap cannot hide behind a zero edge."""
    m = torch.zeros_like(x, dtype=torch.bool)
    for d in (hdim, wdim):
        m.index_fill_(d, torch.tensor([0, x.shape[d] - 1]), True)
    x[m & (x == 0)] = val
    return x


@lru_cache(maxsize=None)
def _payload(pl, exact):
    """Operands of a case's payload as f32 tensors: x (first / stem: the BCHW image; bneck / c3k2: the NHWC map, f16-representable) and
    convs = [(w, b), ...] in the chain's order (weights f16-representable, biases any f32)."""
    kind, B, H, W, widths = pl
    g = _gen(B, H, W, *widths, exact, len(kind))
    image = kind in ("first", "stem")
    if kind == "first":
        shapes = [(widths[0], 3, 3)]
    elif kind == "stem":
        shapes = [(widths[0], 3, 3), (widths[1], widths[0], 3)]
    elif kind == "bneck":
        shapes = [(widths[1], widths[0], 3), (widths[0], widths[1], 3)]
    else:
        cin, c, c2 = widths
        shapes = [(2 * c, cin, 1), (c // 2, c, 3), (c, c // 2, 3), (c2, 3 * c, 1)]
    xshape = (B, 3, H, W) if image else (B, H, W, widths[0])
    if not exact:
        h = lambda t: t.to(F16).to(F32)
        x = torch.rand(xshape, generator=g) if image else h(torch.randn(xshape, generator=g))
        convs = [(h(torch.randn((co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5), torch.randn(co, generator=g) * 0.2) for co, ci, k in shapes]
        return SimpleNamespace(x=x, convs=convs)
    draw = lambda shp, lim: torch.randint(-lim, lim + 1, shp, generator=g).float()
    x = _border_nonzero(draw(xshape, 8 if image else 3) / 8, 2 if image else 1, 3 if image else 2, 0.375)
    convs = []
    for i, (co, ci, k) in enumerate(shapes):
        K = ci * k * k
        if i == 0:  # weights in {-1, 0, 1}, bias in eighths: the map is a multiple of 1/8.  Dense over the image's 27 taps, 32 of K beyond
            keep = (torch.rand((co, ci, k, k), generator=g) < min(1.0, 32.0 / K)).float() if K > 27 else 1.0
            convs.append((draw((co, ci, k, k), 1) * keep, draw((co,), 8) / 8))
        else:       # weights in {-1/4, 0, 1/4}, 16 of K, bias in 1/32
            keep = (torch.rand((co, ci, k, k), generator=g) < 16.0 / K).float()
            convs.append(((2 * torch.randint(0, 2, (co, ci, k, k), generator=g).float() - 1) * keep / 4, draw((co,), 16) / 32))
    return SimpleNamespace(x=x, convs=convs)


def _dyadic(v, step, lim):
    return bool((v / step == (v / step).round()).all()) and float(v.abs().max()) < lim


@lru_cache(maxsize=None)
def _exact_ref(pl):
    """The fp64 stages of a dyadic payload with act = 0 -> [stage, ...]; the last one's ref is the op's one right answer.  Asserted:
    every map is a multiple of 2^-5 below 64 in magnitude and every S 2^5 < 2^24."""
    kind = pl[0]
    p = _payload(pl, True)
    if kind in ("first", "stem"):
        st = [_stage(p.x, *p.convs[0], 2, 0)]
        if kind == "stem":
            st.append(_stage(nchw(st[0].ref), *p.convs[1], 2, 0))
    else:
        st = [_stage(nchw(p.x), *p.convs[0], 1, 0)]
        st.append(_stage(nchw(st[0].ref), *p.convs[1], 1, 0, res=p.x))
    assert _dyadic(p.x, 1 / 8, 64)
    for s in st:
        assert _dyadic(s.v, 1 / 32, 64) and _dyadic(s.ref, 1 / 32, 64) and float(s.S.max()) * 32 < 2 ** 24, pl
        s.ref = s.ref + 0.0  # no kernel returns -0 here: the chains start at a +0 or non-zero bias
    return st


# ------------------------------------------------------------------------------------------------------------
# one op, or the chain it stands for, as a plan on poisoned buffers
# ------------------------------------------------------------------------------------------------------------
LDX = 24  # a destination or intermediate view: channels [8, 8 + C) of rows of C + 24 elements


def _dst(B, h, w, C_, coff=8, ld=None):
    ld = C_ + LDX if ld is None else ld
    return poisoned((B, h, w, ld), coff, C_, None, POISON16, dtype=F16), view(1, ld, coff, C_), (coff, C_)


def _take(t, rng):
    """The view `rng` = (coff, C) of a 777 buffer on the host, the rest of the buffer checked bit for bit."""
    assert_poison_intact(t, rng[0], rng[1], POISON16)
    return t[..., rng[0]:rng[0] + rng[1]].cpu()


def _go_image(cs, p, act, chain=False, spoil=None):
    """CONV_FIRST or STEM (chain: CONV_FIRST into an f16 map, slot 2, then CONV 3x3 s2) -> (output view, [intermediate views])."""
    B, H, W = cs.B, cs.H, cs.W
    oh0, ow0 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    oh, ow = cs.out_hw
    keep, img = poisoned_image(p.x, cs.idt, cs.mis)
    dst, dv, drng = _dst(B, oh, ow, cs.widths[-1])
    blob, recs = conv16_records(p.convs)
    idt, ext, mids = L.dtype_code(cs.idt), [img, dst], []
    if cs.kind == "first":
        ops = [conv_first16_op(B, H, W, dv, *recs[0], idt, act)]
    elif not chain:
        ops = [stem_op(B, H, W, dv, cs.widths[0], recs[0], recs[1], idt, act)]
    else:
        C0 = cs.widths[0]
        mid = poisoned((B, oh0, ow0, C0 + LDX), 8, C0, None, POISON16, dtype=F16)
        mv = view(2, C0 + LDX, 8, C0)
        ops = [conv_first16_op(B, H, W, mv, *recs[0], idt, act), conv16_op(B, oh0, ow0, 3, 2, 1, mv, dv, *recs[1], act=act)]
        ext, mids = ext + [mid], [(mid, (8, C0))]
    if spoil is not None:
        spoil(SimpleNamespace(op=ops[0], ext=ext, dst=dst))
    before = keep.clone()
    run_ops(ops, ext, blob)
    assert torch.equal(bits(keep), bits(before)), "a store reached the image's allocation"
    return _take(dst, drng), [_take(m, r) for m, r in mids]


def _go_bneck(cs, p, act, chain=False, spoil=None):
    """BNECK (chain: CONV 3x3 into a hidden map, slot 2, then CONV 3x3 with res = the source view) -> (output, [hidden map])."""
    B, H, W = cs.B, cs.H, cs.W
    C_, CH = cs.widths
    x16 = p.x.to(F16)
    if cs.place == "one":
        ld = 3 * C_ + 8
        buf = poisoned((B, H, W, ld), C_, C_, x16, NAN)
        buf[..., 2 * C_:3 * C_] = POISON16
        src, dst, sv, dv, drng, ext = buf, buf, view(0, ld, C_, C_), view(0, ld, 2 * C_, C_), (2 * C_, C_), [buf]
    else:
        src = poisoned((B, H, W, C_ + 16), 8, C_, x16, NAN)
        dst, dv, drng = _dst(B, H, W, C_, 16, C_ + 40)
        sv, ext = view(0, C_ + 16, 8, C_), [src, dst]
    blob, recs = conv16_records(p.convs)
    mids = []
    if not chain:
        ops = [bneck_op(B, H, W, sv, dv, CH, recs[0], recs[1], act)]
    else:
        hid = poisoned((B, H, W, CH + LDX), 8, CH, None, POISON16, dtype=F16)
        hv = view(2, CH + LDX, 8, CH)
        ops = [conv16_op(B, H, W, 3, 1, 1, sv, hv, *recs[0], act=act), conv16_op(B, H, W, 3, 1, 1, hv, dv, *recs[1], res=sv, act=act)]
        ext, mids = ext + [None] * (2 - len(ext)) + [hid], [(hid, (8, CH))]
    if spoil is not None:
        spoil(SimpleNamespace(op=ops[0], ext=ext, dst=dst))
    before = dst.cpu()
    sbefore = src.cpu()
    run_ops(ops, ext, blob)
    assert_outside_views_intact(dst, before, [drng])  # "one": the source and the NaN around it included
    assert cs.place == "one" or torch.equal(bits(src), bits(sbefore)), "a store reached the source buffer"
    return dst[..., drng[0]:drng[0] + drng[1]].cpu(), [_take(m, r) for m, r in mids]


def _go_c3k2(cs, p, chain=False, spoil=None):
    """C3K2 (chain: CONV 1x1 into [8, 8 + 2c) of a concat buffer of ld 3c + 16, slot 2, BNECK [8 + c, 8 + 2c) -> [8 + 2c, 8 + 3c), CONV
    1x1 over [8, 8 + 3c)) -> (output, [the concat view (B, H, W, 3c)])."""
    B, H, W = cs.B, cs.H, cs.W
    cin, c, c2 = cs.widths
    src = poisoned((B, H, W, cin + 16), 8, cin, p.x.to(F16), NAN)
    dst, dv, drng = _dst(B, H, W, c2, 16, c2 + 40)
    sv = view(0, cin + 16, 8, cin)
    blob, recs = conv16_records(p.convs)
    ext, mids = [src, dst], []
    if not chain:
        ops = [c3k2_op(B, H, W, sv, dv, c, recs)]
    else:
        ldc = 3 * c + 16
        cat = poisoned((B, H, W, ldc), 8, 3 * c, None, POISON16, dtype=F16)
        ops = [conv1x1_op(B, H, W, sv, view(2, ldc, 8, 2 * c), *recs[0]),
               bneck_op(B, H, W, view(2, ldc, 8 + c, c), view(2, ldc, 8 + 2 * c, c), c // 2, recs[1], recs[2], 1),
               conv1x1_op(B, H, W, view(2, ldc, 8, 3 * c), dv, *recs[3])]
        ext, mids = ext + [cat], [(cat, (8, 3 * c))]
    if spoil is not None:
        spoil(SimpleNamespace(op=ops[0], ext=ext, dst=dst))
    sbefore = src.cpu()
    run_ops(ops, ext, blob)
    assert torch.equal(bits(src), bits(sbefore)), "a store reached the source buffer"
    return _take(dst, drng), [_take(m, r) for m, r in mids]


def _go(cs, p, act, chain=False, spoil=None):
    if cs.kind in ("first", "stem"):
        return _go_image(cs, p, act, chain, spoil)
    if cs.kind == "bneck":
        return _go_bneck(cs, p, act, chain, spoil)
    assert act == 1
    return _go_c3k2(cs, p, chain, spoil)


# ------------------------------------------------------------------------------------------------------------
# the payloads, the case list and the bound, anywhere
# ------------------------------------------------------------------------------------------------------------
def test_payloads_are_exact_and_cases_reach_every_edge():
    """Every dyadic payload meets the conditions of _exact_ref (one right answer in f32 and f16), with non-zero image and map borders;
    the case list holds what the module's docstring promises: the persistent-walk cases (tiles >= 2.5 x cap, every tile inside a map,
    no multiple of 8, more tiles per image than a workgroup's step), a case of fewer than 8 tiles per persistent kernel, the load
    paths and NT values of conv_first, the tile edges of the fused kernels."""
    assert len(set(_ids(CASES))) == len(CASES)
    for pl in dict.fromkeys(cs.payload for cs in EXACT):
        st, p = _exact_ref(pl), _payload(pl, True)
        hd, wd = (2, 3) if pl[0] in ("first", "stem") else (1, 2)
        for d in (hd, wd):
            for i in (0, p.x.shape[d] - 1):
                assert bool((p.x.select(d, i) != 0).all()), pl
        assert all(float(s.ref.abs().max()) > 0 for s in st)
        ws = [w for w, _ in p.convs]
        assert all(len({tuple(w[:, :, i, j].flatten().tolist()) for i in range(3) for j in range(3)}) == 9 for w in ws), "taps differ"
    walks = [cs for cs in CASES if cs.walk]
    assert [(cs.kind, cs.cap) for cs in walks] == [("stem", 768), ("stem", 512), ("bneck", 768), ("bneck", 256), ("c3k2", 768)]
    for cs in walks:
        th, tw = TILE[cs.kind]
        oh, ow = cs.out_hw
        per, n = cs.tiles
        assert oh % th == 0 and ow % tw == 0 and oh // th >= 2 and ow // tw >= 2 and per == (oh // th) * (ow // tw), cs.name
        assert n >= 2.5 * cs.cap and n % 8 and per > cs.cap // 8 and oh // th > 2, cs.name
        assert "%dtiles-cap%d" % (n, cs.cap) in cs.name
    for kind, wd in (("stem", (32, 64)), ("bneck", (32, 16)), ("bneck", (64, 32)), ("c3k2", (64, 32, 128))):
        assert any(cs.kind == kind and cs.widths == wd and cs.tiles[1] < 8 for cs in CASES), (kind, wd)
    fi = [cs for cs in CASES if cs.kind == "first"]
    for dt in (F16, F32):
        f = [cs for cs in fi if cs.idt == dt]
        assert {cs.widths[0] for cs in f if (cs.H, cs.W, cs.mis) == (22, 140, 0)} == {8, 32, 48, 96, 128}
        slow = [cs for cs in f if cs.W % 4 or cs.mis]
        assert {cs.W % 4 for cs in slow} == {0, 1, 2} and {-(-cs.widths[0] // 32) for cs in slow} >= {2, 3, 4}
        assert all(cs.widths[0] % 32 for cs in slow if cs.widths[0] > 32) and {(cs.H, cs.W) for cs in f} >= {(1, 1), (3, 5)}
        assert any(cs.mis == 1 and replace(cs, mis=0, name=cs.name[:-5]) in f for cs in f)
    st = [cs for cs in CASES if cs.kind == "stem" and not cs.walk]
    assert {(cs.H, cs.W) for cs in st} >= {(38, 52), (37, 52), (4, 4), (7, 8), (70, 36), (16, 132)} and all(cs.W % 4 == 0 for cs in st)
    assert {(cs.widths, cs.idt) for cs in st} == {((32, 64), F16), ((32, 64), F32), ((16, 32), F16), ((16, 32), F32)}
    bn = [cs for cs in CASES if cs.kind == "bneck" and not cs.walk]
    assert {(cs.widths, cs.H, cs.W, cs.place) for cs in bn} >= {(wd, h, w, pc) for wd in ((32, 16), (64, 32)) for h, w in ((3, 5), (9, 13), (17, 33))
                                                               for pc in ("one", "sep")}
    assert {(cs.H, cs.W) for cs in CASES if cs.kind == "c3k2" and not cs.walk} >= {(3, 5), (9, 13), (5, 33)}
    assert all(cs.B <= 3 for cs in CASES if not cs.walk)
    print("block16: %d cases (%d with a dyadic payload), %d payloads" % (len(CASES), len(EXACT), len({cs.payload for cs in CASES})))


def _cpu_chain(pl):
    """The stages of a random payload's chain on the CPU -> [(name, x (B, C, H, W), w, b, stride, shortcut or None), ...]: every stage's
    input is the f16 rounding of a float32 evaluation of the stage before (on the GPU: the map read back from the device)."""
    kind, p = pl[0], _payload(pl, False)
    h = lambda t: t.to(F16).to(F32)
    ev = lambda x, w, b, s: h(F.silu(F.conv2d(x, w, b, s, w.shape[-1] // 2)))
    cv = p.convs
    if kind in ("first", "stem"):
        x0 = h(p.x)
        st = [("image conv", x0, *cv[0], 2, None)]
        return st + ([("3x3 s2", ev(x0, *cv[0], 2), *cv[1], 2, None)] if kind == "stem" else [])
    x0 = nchw(p.x)
    if kind == "bneck":
        return [("cv1", x0, *cv[0], 1, None), ("cv2 + x", ev(x0, *cv[0], 1), *cv[1], 1, p.x)]
    c = pl[4][1]
    y01 = ev(x0, *cv[0], 1)
    y1 = y01[:, c:].contiguous()
    hid = ev(y1, *cv[1], 1)
    y2 = h(ev(hid, *cv[2], 1) + y1)
    return [("cv1", x0, *cv[0], 1, None), ("m.cv1", y1, *cv[1], 1, None), ("m.cv2 + y1", hid, *cv[2], 1, nhwc(y1)),
            ("cv2", torch.cat((y01, y2), 1), *cv[3], 1, None)]


def test_cpu_float32_within_half_the_bound():
    """A float32 evaluation by torch on the CPU (another summation order than any kernel's) of every stage of every random payload
    that is held to the bound uses, before the rounding to f16, at most half of the bound's arithmetic part."""
    worst = {}
    for pl in dict.fromkeys(cs.payload for cs in CASES if not cs.walk):
        for name, x, w, b, s, res in _cpu_chain(pl):
            a32 = nhwc(F.silu(F.conv2d(x, w, b, s, w.shape[-1] // 2)))
            assert a32.dtype == F32
            st = _stage(x, w, b, s, 1, res)
            r = _worst(a32, st.a, _bound(st, st, res is not None)[0])
            assert r <= 0.5, (pl, name, r)
            worst[(pl[0], name)] = max(worst.get((pl[0], name), 0.0), r)
    for (kind, name), r in worst.items():
        print("CPU float32 %s %s: worst error / arithmetic part of the bound = %.3f" % (kind, name, r))


# ------------------------------------------------------------------------------------------------------------
# 1. dyadic payloads, act = 0: bit for bit against fp64
# ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cs", EXACT, ids=_ids(EXACT))
def test_block_exact(cs):
    """The op with act = 0 returns the fp64 answer's bits: a wrong tap, halo pixel, weight row or record, a hidden map that is not
    zero outside the map or a dropped shortcut shows as another dyadic number, a read outside the image, a view or a record as NaN.
    An image one element off a 16-byte boundary returns the aligned run's bits."""
    p = _payload(cs.payload, True)
    got, _ = _go(cs, p, 0)
    want = _exact_ref(cs.payload)[-1].ref.to(F16)
    assert got.shape == want.shape
    bad = bits(got) != bits(want)
    assert not bool(bad.any()), "%s: %d of %d elements differ, first at %s" % (cs.name, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
    if cs.mis:
        assert torch.equal(bits(got), bits(_go(replace(cs, mis=0), p, 0)[0]))


# ------------------------------------------------------------------------------------------------------------
# 2. random payloads, act = 1: the chain's bits, every stage of the chain within the derived bound
# ------------------------------------------------------------------------------------------------------------
def _held(cs, name, got, x, w, b, s, res=None):
    """One stage against fp64 with `x` (B, C, H, W), the values it read, under _bound; prints the figure, then asserts."""
    st = _stage(x, w, b, s, 1, res)
    arith, rnd = _bound(st, st, res is not None)
    r = _worst(got, st.ref, arith + rnd)
    over = float((((got.to(F64) - st.ref).abs() - rnd) / arith).clamp(min=0).max()) if r <= 1.0 else float("inf")
    print("block16 %s [%s / %s]: worst error / bound = %.3f, past the rounding part: %.3f of the arithmetic part" % (cs.name, cs.kind, name, r, over))
    assert r <= 1.0, "%s %s: %.3f of the bound" % (cs.name, name, r)


@gpu
@pytest.mark.parametrize("cs", CASES, ids=_ids(CASES))
def test_block_random(cs):
    """a. The fused op returns the bits of its chain of plain ops (CONV_FIRST: there is no chain).  b. Every stage of the chain lies
    within _bound of the fp64 evaluation of the stage's input, read back (not for the persistent-walk cases: the chain only)."""
    p = _payload(cs.payload, False)
    cv = p.convs
    got, _ = _go(cs, p, 1)
    assert bool(torch.isfinite(got.float()).all()), "a NaN from outside the image, a view or a weight record reached the output"
    if cs.kind == "first":
        if cs.mis:
            assert torch.equal(bits(got), bits(_go(replace(cs, mis=0), p, 1)[0]))
        return _held(cs, "image conv", got, p.x.to(F16), *cv[0], 2)
    two, mids = _go(cs, p, 1, chain=True)
    bad = bits(got) != bits(two)
    assert not bool(bad.any()), "%s: fused op and chain differ in %d of %d elements, first at %s" % (cs.name, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
    if cs.walk:
        return
    mid = mids[0]
    if cs.kind == "stem":
        _held(cs, "image conv", mid, p.x.to(F16), *cv[0], 2)
        _held(cs, "3x3 s2", two, nchw(mid), *cv[1], 2)
    elif cs.kind == "bneck":
        _held(cs, "cv1", mid, nchw(p.x), *cv[0], 1)
        _held(cs, "cv2 + x", two, nchw(mid), *cv[1], 1, res=p.x)
    else:
        c = cs.widths[1]
        _held(cs, "cv1", mid[..., :2 * c], nchw(p.x), *cv[0], 1)
        # the BNECK stage again as its own chain on y1, read back: the same bits, its two stages within the bound
        y1 = mid[..., c:2 * c].contiguous()
        bn = Case("bneck", cs.name, cs.B, cs.H, cs.W, (c, c // 2), place="sep")
        y2, (hid,) = _go_bneck(bn, SimpleNamespace(x=y1.float(), convs=cv[1:3]), 1, chain=True)
        assert torch.equal(bits(y2), bits(mid[..., 2 * c:])), "%s: the BNECK stage and its two-CONV chain differ" % cs.name
        _held(cs, "m.cv1", hid, nchw(y1), *cv[1], 1)
        _held(cs, "m.cv2 + y1", y2, nchw(hid), *cv[2], 1, res=y1)
        _held(cs, "cv2", two, nchw(mid), *cv[3], 1)


# ------------------------------------------------------------------------------------------------------------
# 3. refusals through the plan interface
# ------------------------------------------------------------------------------------------------------------
def _set(**kw):
    return lambda t: [setattr(t.op, k, v) for k, v in kw.items()]


def _dst_view(ld=None, coff=None):
    def spoil(t):
        d = t.op.dst
        t.op.dst = type(d)(d.buf, d.ld if ld is None else ld, d.coff if coff is None else coff, d.C)
    return spoil


def _off_by_2_bytes(t):
    raw = t.ext[0]
    flat = torch.full((raw.numel() + 8,), NAN, dtype=raw.dtype, device=raw.device)
    t.ext[0] = flat[1:1 + raw.numel()].view(raw.shape).copy_(raw)
    assert t.ext[0].data_ptr() % 16 == 2


_STEM = Case("stem", "", 2, 16, 16, (32, 64))
_BN = Case("bneck", "", 2, 9, 13, (32, 16))
_C3 = Case("c3k2", "", 2, 9, 13, (64, 32, 128))
_FI = Case("first", "", 2, 22, 40, (32,))
REFUSALS = {
    "stem: W % 4 != 0": (replace(_STEM, W=18), None, None),
    "stem: H = 3": (replace(_STEM, H=3), None, None),
    "stem: widths (64, 128)": (replace(_STEM, widths=(64, 128)), None, None),
    "stem: OH off by one": (_STEM, lambda t: setattr(t.op, "OH", t.op.OH + 1), None),
    "stem: in_dtype neither F16 nor F32": (_STEM, _set(in_dtype=2), None),
    "stem: image pointer 2 bytes off": (_STEM, _off_by_2_bytes, None),
    "bneck: widths (64, 64)": (replace(_BN, widths=(64, 64)), None, None),
    "c3k2: widths (128, 64, 256)": (replace(_C3, widths=(128, 64, 256)), None, None),
    "stem: dst.ld % 8 != 0": (_STEM, _dst_view(ld=64 + LDX - 4), None),
    "bneck: dst.ld % 8 != 0": (_BN, _dst_view(ld=32 + 40 - 4), None),
    "c3k2: dst.ld % 8 != 0": (_C3, _dst_view(ld=128 + 40 - 4), None),
    "first: dst.ld % 8 != 0": (_FI, _dst_view(ld=32 + LDX - 4), None),
    "stem: dst.coff % 8 != 0": (_STEM, _dst_view(coff=4), None),
    "bneck: dst.coff % 8 != 0": (_BN, _dst_view(coff=12), None),
    "c3k2: dst.coff % 8 != 0": (_C3, _dst_view(coff=12), None),
    "first: dst.coff % 8 != 0": (_FI, _dst_view(coff=4), None),
    "first: Cout 12": (replace(_FI, widths=(12,)), None, None),
    "first: Cout 136": (replace(_FI, widths=(136,)), None, None),
    "first: ksize 5": (_FI, _set(ksize=5, pad=2, OH=11, OW=20), None),
    "stem: prec 1": (_STEM, _set(prec=1), "fused kinds are fp16-only"),
    "bneck: prec 1": (_BN, _set(prec=1), "fused kinds are fp16-only"),
    "c3k2: prec 1": (_C3, _set(prec=1), "fused kinds are fp16-only"),
}


@gpu
@pytest.mark.parametrize("what", list(REFUSALS))
def test_block_refusals(what):
    """bsy_plan_create or bsy_plan_run refuses the op with a BsyError before anything is launched: the whole destination buffer still
    holds its poison."""
    cs, spoil, match = REFUSALS[what]
    kept = []

    def hook(t):
        if spoil is not None:
            spoil(t)
        kept.append((t.dst, t.dst.clone()))

    with pytest.raises(L.BsyError, match=match):
        _go(cs, _payload(cs.payload, False), 1, spoil=hook)
    torch.cuda.synchronize()
    dst, before = kept[0]
    assert torch.equal(bits(dst), bits(before)), "a refused op stored"
    assert_poison_intact(dst, 0, 0, POISON16)


# ------------------------------------------------------------------------------------------------------------
# 4. the engine on an image off a 16-byte boundary
# ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", [F16, F32], ids=_dt)
def test_engine_takes_an_image_off_a_16_byte_boundary(dt):
    """YoloEngine.forward keeps a contiguous tensor as it is, whatever its storage offset; launch_stem_fused wants the image on an
    8-byte (f16) or 16-byte (f32) boundary.  A default yolo11n engine (stem fused) on a contiguous (2, 3, 64, 64) view whose first
    element lies one element past a 16-byte boundary returns the bits it returns on an aligned copy."""
    from bs_yolo_amd.engine import YoloEngine
    from bs_yolo_amd.graphs import stock_cfg
    from oracle import yolo_ref as R
    m = R.Model("yolo11", "n", 80, "detect")
    eng = YoloEngine(stock_cfg("yolo11", "n"), R.synth_params(m, 0), device=0)
    try:
        plan, _ = eng.plan_for(2, 64, 64, dt, dt)
        assert plan.ops[0]["kind"] == L.OP_STEM
        x = torch.rand(2, 3, 64, 64, generator=_gen(6)).to(dt)
        flat = torch.zeros(x.numel() + 16, dtype=dt, device=DEV)
        off = flat[9:9 + x.numel()].view(x.shape).copy_(x)
        al = x.to(DEV)
        assert off.is_contiguous() and off.data_ptr() % 16 == off.element_size() and al.data_ptr() % 16 == 0
        y0, r0 = eng(al)
        y0, r0 = y0.clone(), [r.clone() for r in r0]
        y1, r1 = eng(off)
        torch.cuda.synchronize()
        assert torch.equal(bits(y0), bits(y1)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(r0, r1))
    finally:
        eng.close()
