"""The fused Detect head ops ALONE: BSY_OP_CONV with prec 0 and out_f32 = 2 (class scores) or 3 (DFL boxes) as one-op plans
(op_plan_helpers.head16_op, run_conv_cfgs) on poisoned buffers, under EVERY kernel configuration id that conv_cfg_valid admits -- the
three pieces of code through which every detection of a default fp16 Detect plan leaves the device:

  * conv_epilogue_head with epi 2 and its LDS twin conv_epilogue_cls_lds (csrc/conv_kernels.h): sigmoid into rows 4 + c of y;
  * dfl_decode_store: the DFL expectation over a lane pair, dist2bbox * stride into rows 0..3;
  * the CONV_TAIL rows of kConvCfgs (conv3x3_patch_kernel<.., TAIL = true>, csrc/conv_patch.hip): 3x3 conv + 1x1 conv + decoder.

Poison: the source is a channel view of an f16 NaN buffer, the weight records lie in a blob with NaN between them, y is a
(B, 4 + nc + 3, A) tensor with anchors on both sides of the level's [a0, a0 + h w) and the raw map a (B, 64 + nc + 5, h, w) tensor,
both filled with 777 (f16) or 7.77e7 (f32); after every run everything outside what the op owns is compared bit for bit.

Two payload kinds.  Dyadic payloads make every logit exact in f32 (whatever the summation order) and in f16: the raw map must hold
the fp64 logits bit for bit, y must lie within the project's own decode bound (test_glue_ops._decode_check) of the fp64 decode, and
all ids -- and both class epilogues -- must return the same bits.  Random payloads are held to a bound derived per element from the
operands (_bounds); the tail is pinned, bit for bit, to the two launches it replaces (the plain 3x3 CONV op at the same patch id into
an f16 map, then the 1x1 decoding op on that map), and those to the derived bound with the map read back as the reference's input.

head_cfg_valid mirrors conv_cfg_valid (csrc/conv_select.hip) including its epi rules; cfg_row and TABLE come from
test_fp16_conv_ops.  The GPU tests are marked ``gpu`` one by one: the tests about the case table and the bound run anywhere.

Run on the MI355X box with ``pytest -m gpu``.
"""
import math
import re
from dataclasses import dataclass, replace
from functools import lru_cache
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from op_plan_helpers import (NAN, POISON16, POISON32, bits, conv16_op, conv16_records, head16_op, nchw, nhwc, poisoned, run_conv_cfgs,
                             run_op, ulp16, view)
from test_fp16_conv_ops import TABLE, cfg_row

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from bs_yolo_amd import lib as L  # noqa: F401  (fails loudly when the .so is missing)

F32, F16, F64 = torch.float32, torch.float16, torch.float64
U = 2.0 ** -24  # unit roundoff of f32
GEMM_TM = {0: 256, 1: 256, 2: 128, 3: 128, 4: 256, 5: 64, 6: 64, 7: 256}  # pixel tile of the implicit-GEMM tiles 0x0x .. 0x7x


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 104729 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _u16(t):
    return torch.from_numpy(ulp16(t.numpy()))


def _tail_ids():
    """The ids that have a second row with the box-branch tail in kConvCfgs, from the text of csrc/conv_select.hip."""
    src = (Path(__file__).resolve().parents[1] / "bs_yolo_amd" / "csrc" / "conv_select.hip").read_text()
    body = src[src.index("kConvCfgs[] = {"):]
    body = body[:body.index("};")]
    return tuple(sorted(int(m, 16) for m in re.findall(r"patch_row<[^>]*true>\((0x[0-9A-Fa-f]+)\)", body)))


TAIL_IDS = _tail_ids()


# ------------------------------------------------------------------------------------------------------------
# the case list and conv_cfg_valid with its epi rules
# ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Head:
    name: str
    mode: int             # out_f32 of the op: 2 = class scores, 3 = DFL boxes
    h: int
    w: int
    a0: int               # first anchor of the level in y ...
    A: int                # ... which holds A anchors
    stride: float = 8.0
    Cin: int = 64
    nc: int = 5           # a box op: only the size of y and of the raw map
    tail: bool = False    # the box-branch tail: this op is the 3x3 conv 64 -> 64, the 1x1 conv 64 -> 64 and the decoder follow in the launch
    B: int = 3
    refused: tuple = ()   # ids bsy_plan_check_tuning must answer 0 for (every valid id runs)

    @property
    def Cout(self):
        return self.nc if self.mode == 2 else 64

    @property
    def k(self):
        return 3 if self.tail else 1

    @property
    def nrows(self):
        return 4 + self.nc + 3

    @property
    def rawC(self):
        return 64 + self.nc + 5

    @property
    def hw(self):
        return self.h * self.w

    @property
    def M(self):
        return self.B * self.hw

    @property
    def payload(self):
        """What the operands and the logits depend on: cases with equal payloads share them."""
        return (self.mode, self.tail, self.B, self.h, self.w, self.Cin, self.Cout)


def head_cfg_valid(hc, cfg):
    """conv_cfg_valid (csrc/conv_select.hip) for a decoding op: one source, stride 1, no shortcut, no split-K; epi = hc.mode.
    An op with tail weights has only the six tail rows; every other op only the plain rows."""
    if cfg & ~4 not in TABLE:
        return False
    if hc.tail and cfg & ~4 not in TAIL_IDS:
        return False  # conv_cfg_row(cfg, tail = true) finds no row
    r, t = cfg_row(cfg), (cfg & ~4) >> 4
    aligned, aligned64 = not hc.Cin & 31, not hc.Cin & 63
    ko = 1 if hc.k == 3 and aligned else 0  # conv_korder: 3x3 stride 1 on 32-channel chunks
    if (r.aligned and not aligned) or (r.bk == 64 and not aligned64):
        return False
    if r.fam == "gemm":  # (never a tail op: those rows are patch rows)
        if bool(cfg & 4) != bool(ko):
            return False
        if ko and (not r.aligned or r.bk == 64):
            return False
        if hc.mode == 3 and (GEMM_TM[t] != 256 or r.tn != 64):
            return False  # DFL needs all 64 box couts in one wave
        return r.tn != 256 or not hc.Cout & 255
    if cfg & 4:
        return False
    if not hc.tail:
        return False  # epi != 0: refused by every persistent, weights-resident and plain patch id
    return hc.mode == 3 and hc.Cout == 64 and ko == 1 and hc.k == 3


def valid_ids(hc):
    return tuple(i for i in TABLE if head_cfg_valid(hc, i))


def _heads():
    cs = []
    # class ops.  9 x 13 x 3 = 351 pixels: a ragged second 256-pixel tile; h w = 117, a0 = 11, A = 137: the y rows of successive images
    # and classes start on every residue mod 8, 8-anchor pieces straddle two images
    cs.append(Head("cls-9x13-c64-nc80", 2, 9, 13, 11, 137, nc=80, refused=(0x71, 0x73, 0x81, 0x93, 0xB1, 0xD2, 0xE1, 0xF2, 0xA1)))
    cs.append(Head("cls-9x13-c64-nc5", 2, 9, 13, 11, 137, nc=5, refused=(0x72, 0x91, 0xB2)))
    cs.append(Head("cls-9x13-c64-nc1", 2, 9, 13, 11, 137, nc=1, refused=(0x71, 0xF1)))
    cs.append(Head("cls-9x13-c64-nc256", 2, 9, 13, 11, 137, nc=256, refused=(0x40, 0x82, 0xC1, 0xE2)))
    cs.append(Head("cls-9x13-c40-nc5", 2, 9, 13, 11, 137, Cin=40, nc=5, refused=(0x01, 0x13, 0x21, 0x41, 0x62, 0x91)))
    cs.append(Head("cls-5x5-c64-nc80", 2, 5, 5, 7, 41, nc=80, refused=(0x71, 0xD1)))
    cs.append(Head("cls-3x5-c64-nc5", 2, 3, 5, 3, 23, nc=5, refused=(0x83,)))
    # h w, a0 and A multiples of 8: every 8-anchor piece takes the vector store
    cs.append(Head("cls-8x16-c64-nc80-al8", 2, 8, 16, 8, 144, nc=80, refused=(0x72, 0xB3)))
    cs.append(Head("cls-8x16-c40-nc80-al8", 2, 8, 16, 8, 144, Cin=40, nc=80, refused=(0x02, 0x33)))
    # box ops: the 256 x 64 tiles only
    cs.append(Head("box-9x13-c64", 3, 9, 13, 11, 137, 16.0, refused=(0x01, 0x21, 0x31, 0x41, 0x61, 0x91, 0xB1, 0xF1)))
    cs.append(Head("box-5x5-c40", 3, 5, 5, 7, 41, 32.0, Cin=40, refused=(0x11, 0x12, 0x13, 0x30, 0x00)))
    cs.append(Head("box-8x16-c64-al8", 3, 8, 16, 8, 144, 8.0, refused=(0x03, 0xD2)))
    cs.append(Head("box-3x5-c64", 3, 3, 5, 3, 23, 32.0, refused=(0x63,)))
    # tails: 17 x 21 is ragged in both directions for 8 x 16 and 6 x 20 tiles; 20 x 20 is where the heuristic prefers 6 x 20; 3 x 5 is
    # smaller than any tile (the plan emits the tail at every map size)
    cs.append(Head("tail-17x21", 3, 17, 21, 5, 369, 32.0, tail=True, refused=(0xA1, 0xC1, 0x11, 0x15, 0x91, 0xF1)))
    cs.append(Head("tail-20x20", 3, 20, 20, 16, 424, 16.0, tail=True, refused=(0xA1, 0x13)))
    cs.append(Head("tail-3x5", 3, 3, 5, 3, 23, 8.0, tail=True, refused=(0xC1, 0x10)))
    return cs


HEADS = _heads()
HEAD_IDS = [hc.name for hc in HEADS]
# (dtype of y and of the raw map, raw map: "bound", "null" = a null slot, "missing" = no such slot)
VARIANTS = ((F16, "null"), (F16, "bound"), (F32, "bound"), (F32, "missing"))


def family(hc, odt, raw, cfg):
    """The family a run is reported under in docs/experiments.md."""
    if hc.tail:
        return "tail 8x16" if cfg_row(cfg).fam == "patch" and (cfg >> 4) == 0xB else "tail 6x20"
    if hc.mode == 3:
        return "DFL on 0x1x"
    return "class LDS" if odt == F16 and raw != "bound" else "class direct"


# ------------------------------------------------------------------------------------------------------------
# payloads, the fp64 decode and the bound
# ------------------------------------------------------------------------------------------------------------
def _conv64(x, w, b):
    """fp64 conv of x (B, h, w, C) with w (Cout, C, k, k), stride 1, same padding -> (B, h, w, Cout)."""
    return nhwc(F.conv2d(nchw(x.to(F64)), w.to(F64), b.to(F64), 1, w.shape[-1] // 2))


def _logits(x, w, b):
    """-> (l, S): the fp64 logits of a 1x1 conv and S = |b| + sum |x| |w|."""
    return _conv64(x, w, b) + 0.0, _conv64(x.abs(), w.abs(), b.abs())


def _dyadic(v, step, lim):
    return bool((v / step == (v / step).round()).all()) and float(v.abs().max()) < lim


@lru_cache(maxsize=None)
def _exact(pl):
    """Dyadic operands of a payload (f32 tensors) and their fp64 logits.  Inputs: multiples of 1/8 in [-3/8, 3/8]; weights in
    {-1/4, 0, 1/4}; biases multiples of 1/32 -- logits with a standard deviation near 0.5, so that every DFL bin carries weight.
    Box ops: side 2 (couts 32..47) reads the first half of the input channels and the other sides the second half, and the first half
    is scaled by 8 at every odd anchor: side 2 is peaked there, soft elsewhere.  Tail: the 3x3 conv has weights in {-1, 0, 1} (8 taps
    of 576 per cout) and a bias in eighths, so that the intermediate map is a multiple of 1/8; the 1x1 has 8 weights of +-1/4 per row,
    side 2's scaled by 8.  Asserted: every product, intermediate and logit is a multiple of 2^-5, |logit| < 64 and
    sum |x||w| 2^5 < 2^24, so every logit is exact in f32 in any summation order and exact in f16."""
    mode, tail, B, h, w, Cin, Cout = pl
    g = _gen(mode, tail, B, h, w, Cin, Cout, 1)
    draw = lambda shp, lim: torch.randint(-lim, lim + 1, shp, generator=g).float()
    x = draw((B, h, w, Cin), 3) / 8
    c = SimpleNamespace(x=x, act=0, mid=None, w2=None, b2=None)
    if tail:
        keep = (torch.rand((64, Cin, 3, 3), generator=g) < 1 / 72).float()
        c.w, c.b = draw((64, Cin, 3, 3), 1) * keep, draw((64,), 4) / 8
        mid, S1 = _logits(x, c.w, c.b)
        assert _dyadic(mid, 1 / 8, 64) and float(S1.max()) * 32 < 2 ** 24
        keep2 = (torch.rand((64, 64, 1, 1), generator=g) < 1 / 8).float()
        c.w2, c.b2 = (2 * torch.randint(0, 2, (64, 64, 1, 1), generator=g).float() - 1) * keep2 / 4, draw((64,), 16) / 32
        c.w2[32:48] *= 8
        c.mid = mid.to(F32)
        c.l, S = _logits(c.mid, c.w2, c.b2)
    else:
        c.w, c.b = draw((Cout, Cin, 1, 1), 1) / 4, draw((Cout,), 16) / 32
        if mode == 3:
            half = Cin // 2
            c.w[32:48, half:] = 0
            c.w[:32, :half] = 0
            c.w[48:, :half] = 0
            xa = x.reshape(B, h * w, Cin)
            xa[:, 1::2, :half] *= 8
        c.l, S = _logits(x, c.w, c.b)
    assert _dyadic(c.l, 1 / 32, 64) and float(S.max()) * 32 < 2 ** 24, pl
    return c


@lru_cache(maxsize=None)
def _rand(pl):
    """Random operands (f32 tensors of f16-representable values; the biases: any f32), as test_fp16_conv_ops._inputs draws them:
    randn inputs with every third channel scaled by 1e-3, weights randn * sqrt(2 / K), bias randn / 2.  Tail: SiLU after the 3x3."""
    mode, tail, B, h, w, Cin, Cout = pl
    g = _gen(mode, tail, B, h, w, Cin, Cout, 0)
    hf = lambda t: t.to(F16).to(F32)
    x = torch.randn((B, h, w, Cin), generator=g)
    x[..., ::3] *= 1e-3
    c = SimpleNamespace(x=hf(x), act=int(tail), w2=None, b2=None)
    k = 3 if tail else 1
    c.w = hf(torch.randn((64 if tail else Cout, Cin, k, k), generator=g) * (2.0 / (k * k * Cin)) ** 0.5)
    c.b = torch.randn(64 if tail else Cout, generator=g) * 0.5
    if tail:
        c.w2, c.b2 = hf(torch.randn((64, 64, 1, 1), generator=g) * (2.0 / 64) ** 0.5), torch.randn(64, generator=g) * 0.5
    return c


def _dfl(l):
    """l (B, h, w, 64) fp64 -> (p (B, h w, 4, 16), d (B, h w, 4)): the DFL softmax and its expectation (test_glue_ops._decode_ref)."""
    B = l.shape[0]
    p = torch.softmax(l.reshape(B, -1, 4, 16), -1)
    return p, (p * torch.arange(16, dtype=F64)).sum(-1)


def _decode(hc, l):
    """The rows of y the op owns, in fp64 (test_glue_ops._decode_ref's formula): class (B, nc, h w) = sigmoid; box (B, 4, h w) =
    dist2bbox (xywh) * stride."""
    if hc.mode == 2:
        return torch.sigmoid(l).reshape(hc.B, hc.hw, hc.nc).transpose(1, 2).contiguous()
    _, d = _dfl(l)
    a = torch.arange(hc.hw)
    ax, ay = (a % hc.w).double() + 0.5, (a // hc.w).double() + 0.5
    x1, y1, x2, y2 = ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]
    return torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), 1) * hc.stride


def _decode_part(ref, odt):
    """The project's decode bound (test_glue_ops._decode_check): 2e-4 + 1e-5 |ref|, plus one f16 ulp of ref for f16 output."""
    return 2e-4 + 1e-5 * ref.abs() + (_u16(ref) if odt == F16 else 0.0)


def _bounds(hc, l, S, K, odt):
    """Allowed |got - fp64| of a decoding 1x1 op with K input channels -> ((y arithmetic, y rest), (raw arithmetic, raw rest)).

    A logit's arithmetic error is at most E = 1.1 (K + 1) 2^-24 S, S = |b| + sum |x||w|: the order-independent bound of a length-K fp32
    sum that starts at the bias (the arithmetic part of test_fp16_conv_ops._bound without SiLU).  What the decoder adds on top -- expf,
    the divisions, the output rounding -- is the `rest`: the project's decode bound.

      class score: sigmoid's slope is at most 1/4, so by the mean value theorem the score moves by at most E / 4.
      box side:    d(l) = sum_j j p_j, p = softmax(l) over the side's 16 bins.  dd/dl_j = p_j (j - d), so to first order the side moves
                   by sum_j p_j |j - d| E_j.  Second order: H_jk = d2d / dl_j dl_k = p_j (delta_jk - p_k)(j - d) - p_j p_k (k - d), hence
                   sum_jk |H_jk| <= sum_j p_j |j - d| (1 + sum_k p_k) + sum_k p_k |k - d| sum_j p_j = 3 sum_j p_j |j - d| <= 45 at ANY
                   point of the segment (|j - d| <= 15), and the Lagrange remainder e^T H e / 2 is at most 22.5 max_j E_j^2.  E is of the
                   order 1e-5 here (K <= 64, S of the order 10): a remainder of the order 1e-9 grid units, negligible beside the
                   first-order term (~1e-5) but carried along.
      box xywh:    x = stride (ax + (d2 - d0) / 2), w = stride (d0 + d2): with side bounds D the centre moves by stride (D0 + D2) / 2,
                   the width by stride (D0 + D2); likewise y and the height from sides 1 and 3.
      raw map:     E, plus half an f16 ulp of the logit (f16) or 2^-24 |l| (f32)."""
    E = 1.1 * (K + 1) * U * S
    raw = (nchw(E), nchw(0.5 * _u16(l) if odt == F16 else U * l.abs()))
    ref = _decode(hc, l)
    if hc.mode == 2:
        ar = (E / 4).reshape(hc.B, hc.hw, hc.nc).transpose(1, 2).contiguous()
    else:
        p, d = _dfl(l)
        E4 = E.reshape(hc.B, hc.hw, 4, 16)
        D = (p * (torch.arange(16, dtype=F64) - d[..., None]).abs() * E4).sum(-1) + 22.5 * E4.amax(-1) ** 2
        dx, dy = D[..., 0] + D[..., 2], D[..., 1] + D[..., 3]
        ar = torch.stack((dx / 2, dy / 2, dx, dy), 1) * hc.stride
    return (ar, _decode_part(ref, odt)), raw


def _worst(got, ref, arith, rest):
    """-> (worst |got - ref| / (arith + rest), worst share of the arithmetic part used past the rest); inf when got is not finite (a
    NaN from outside a view or between the weight records reached it)."""
    got = got.to(F64)
    if not bool(torch.isfinite(got).all()):
        return math.inf, math.inf
    err = (got - ref).abs()
    return float((err / (arith + rest)).max()), float(((err - rest) / arith).clamp(min=0).max())


# ------------------------------------------------------------------------------------------------------------
# one decoding op as a plan on poisoned buffers
# ------------------------------------------------------------------------------------------------------------
C0, LD_EXTRA = 8, 24  # the source view: channels [8, 8 + Cin) of rows of Cin + 24 elements


def _own(hc):
    """(row range of y, channel range of the raw map) the op owns."""
    return ((4, 4 + hc.nc), (64, 64 + hc.nc)) if hc.mode == 2 else ((0, 4), (0, 64))


def _assert_rest_is_poison(t, sl, poison, what):
    b = bits(t).clone()
    want = bits(torch.full((1,), poison, dtype=t.dtype)).item()
    b[sl] = want
    assert bool((b == want).all()), "a store left what the op owns in %s" % what


def _setup(hc, c, odt, raw, x=None, convs=None):
    """Buffers, weight blob and the op.  External slots: 0 the source, 1 y, 2 the raw map, 3 a shortcut (refusals only).  x / convs: other
    operands than the payload's (the 1x1 op on an intermediate map)."""
    x = c.x if x is None else x
    Cin = x.shape[-1]
    convs = ([(c.w, c.b)] + ([(c.w2, c.b2)] if hc.tail else [])) if convs is None else convs
    t = SimpleNamespace(odt=odt, poison=POISON16 if odt == F16 else POISON32)
    t.src = poisoned((hc.B, hc.h, hc.w, Cin + LD_EXTRA), C0, Cin, x.to(F16), NAN)
    t.y = torch.full((hc.B, hc.nrows, hc.A), t.poison, dtype=odt).to("cuda:0")
    t.raw = torch.full((hc.B, hc.rawC, hc.h, hc.w), t.poison, dtype=odt).to("cuda:0")
    t.pristine = (t.y.clone(), t.raw.clone())
    t.blob, recs = conv16_records(convs)  # the tail's four records are separate
    t.op = head16_op(hc.B, hc.h, hc.w, hc.k, view(0, Cin + LD_EXTRA, C0, Cin), view(1, 0, 0, hc.nrows), recs[0][0], recs[0][1], hc.mode,
                     64 if hc.mode == 3 else hc.nc, hc.A, hc.a0, hc.stride, L.dtype_code(odt), raw=view(2, 0, 0, hc.rawC), act=c.act,
                     tail=recs[1] if hc.tail else None)
    t.ext = [t.src, t.y] + ([t.raw] if raw == "bound" else [None] if raw == "null" else [])
    return t


def _collect(hc, t, raw):
    """After a run: everything outside what the op owns is poison, bit for bit -> (the owned rows of y (B, rows, h w), the owned
    channels of the raw map (B, C, h, w) or None), on the host."""
    (r0, r1), (c0, c1) = _own(hc)
    y, rw = t.y.cpu(), t.raw.cpu()
    _assert_rest_is_poison(y, (slice(None), slice(r0, r1), slice(hc.a0, hc.a0 + hc.hw)), t.poison, "y")
    _assert_rest_is_poison(rw, (slice(None), slice(c0, c1)) if raw == "bound" else (slice(0, 0),), t.poison, "the raw map")
    return y[:, r0:r1, hc.a0:hc.a0 + hc.hw].contiguous(), rw[:, c0:c1].contiguous() if raw == "bound" else None


def _run(hc, c, odt, raw, ids=None, refused=None, x=None, convs=None):
    """The op under every id of `ids` (default: every id head_cfg_valid admits) -> {id: (y rows, raw channels)}."""
    t = _setup(hc, c, odt, raw, x, convs)

    def reset():
        t.y.copy_(t.pristine[0])
        t.raw.copy_(t.pristine[1])

    return run_conv_cfgs([t.op], t.ext, t.blob, valid_ids(hc) if ids is None else ids, hc.refused if refused is None else refused, reset,
                         lambda: _collect(hc, t, raw))


def _run_two_launches(hc, c, odt, raw, pid):
    """What the tail replaces: the plain 3x3 CONV op (64 couts, the payload's activation) under patch id `pid` into channels
    [8, 72) of an f16 map of 88-element rows filled with 777 (slot 3), then the 1x1 decoding op on that view under 0x11.
    -> (y rows, raw channels, the map's view on the host)."""
    t = _setup(replace(hc, tail=False), c, odt, raw, convs=[(c.w, c.b), (c.w2, c.b2)])
    mid = poisoned((hc.B, hc.h, hc.w, 64 + LD_EXTRA), C0, 64, None, POISON16, dtype=F16)
    t.blob, recs = conv16_records([(c.w, c.b), (c.w2, c.b2)])
    op3 = conv16_op(hc.B, hc.h, hc.w, 3, 1, 1, view(0, hc.Cin + LD_EXTRA, C0, hc.Cin), view(3, 64 + LD_EXTRA, C0, 64), recs[0][0], recs[0][1],
                    act=c.act)
    op1 = head16_op(hc.B, hc.h, hc.w, 1, view(3, 64 + LD_EXTRA, C0, 64), view(1, 0, 0, hc.nrows), recs[1][0], recs[1][1], 3, 64, hc.A, hc.a0,
                    hc.stride, L.dtype_code(odt), raw=view(2, 0, 0, hc.rawC))
    ext = t.ext + [None] * (3 - len(t.ext)) + [mid]

    def collect():
        m = mid.cpu()
        _assert_rest_is_poison(m, (Ellipsis, slice(C0, C0 + 64)), POISON16, "the intermediate map")
        return _collect(hc, t, raw) + (m[..., C0:C0 + 64].contiguous(),)

    return run_conv_cfgs([op3, op1], ext, t.blob, [(pid, 0x11)], (), lambda: None, collect)[(pid, 0x11)]


# ------------------------------------------------------------------------------------------------------------
# the case table and the bound, anywhere
# ------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_fused_decoder_configuration():
    """All six tail ids run in at least one case, 0x10 .. 0x13 run with epi 3 and every implicit-GEMM tile family 0x0x .. 0x7x runs
    with epi 2 (the 256-cout tiles on nc = 256).  Every refused id is invalid by the mirror, and the refused lists name an aligned id on
    40 channels, persistent, weights-resident and plain patch ids under epi 2 and 3, an implicit-GEMM tile other than 256 x 64 under
    epi 3, a 256-cout tile on nc = 80, and for the tail the 128-cout patch ids and implicit-GEMM ids.  The geometry is the one the
    module's docstring promises; every dyadic payload is exact (the assertions of _exact)."""
    assert len(TAIL_IDS) == 6 and set(TAIL_IDS) == {0xB1, 0xB2, 0xB3, 0xD1, 0xD2, 0xD3}
    tails = {i for hc in HEADS if hc.tail for i in valid_ids(hc)}
    assert tails == set(TAIL_IDS)
    dfl = {i for hc in HEADS if hc.mode == 3 and not hc.tail for i in valid_ids(hc)}
    assert dfl == {0x10, 0x11, 0x12, 0x13}
    cls = {i for hc in HEADS if hc.mode == 2 for i in valid_ids(hc)}
    assert {i >> 4 for i in cls} == set(range(8)) and all(cfg_row(i).fam == "gemm" for i in cls)
    assert cls == {i for i in TABLE if i < 0x80}, "every implicit-GEMM id runs with epi 2"
    assert len(set(HEAD_IDS)) == len(HEADS)
    fams = {2: set(), 3: set(), "tail": set()}
    for hc in HEADS:
        ids = valid_ids(hc)
        assert ids and not set(ids) & set(hc.refused), hc.name
        assert not any(head_cfg_valid(hc, i) for i in hc.refused), (hc.name, [hex(i) for i in hc.refused if head_cfg_valid(hc, i)])
        assert hc.refused, hc.name
        fams["tail" if hc.tail else hc.mode] |= {(cfg_row(i).fam, cfg_row(i).tn) for i in hc.refused}
        assert hc.B == 3 and hc.h <= 24 and hc.w <= 24 and hc.a0 > 0 and hc.a0 + hc.hw < hc.A  # anchors on both sides
        if hc.Cin & 31:
            assert all(not cfg_row(i).aligned for i in ids) and any(cfg_row(i).aligned for i in hc.refused)
        if hc.tail:
            assert hc.Cin == 64 and hc.mode == 3
        _exact(hc.payload)
    assert {"persist", "wres", "patch"} <= {f for f, _ in fams[2]} and {"persist", "wres", "patch"} <= {f for f, _ in fams[3]}
    assert ("gemm", 128) in fams[3] and ("gemm", 32) in fams[3] and ("gemm", 256) in fams[2]
    assert ("patch", 128) in fams["tail"] and "gemm" in {f for f, _ in fams["tail"]}
    cl = [hc for hc in HEADS if hc.mode == 2]
    # alignment: h w not a multiple of 8 with a0 and A odd; one case where h w, a0 and A are multiples of 8
    assert {hc.hw for hc in cl if hc.hw % 8 and hc.a0 % 2 and hc.A % 2} >= {25, 117}
    assert any(not (hc.hw % 8 or hc.a0 % 8 or hc.A % 8) for hc in cl) and any(not (hc.hw % 8 or hc.a0 % 8 or hc.A % 8) for hc in HEADS if hc.mode == 3)
    # tiles: more than 256 pixels with a ragged last tile; a map smaller than any tile
    assert any(hc.M > 256 and hc.M % 256 and hc.M % 64 for hc in cl) and any(hc.M < 64 for hc in cl)
    assert {hc.nc for hc in cl} == {1, 5, 80, 256} and {hc.Cin for hc in cl} == {64, 40}
    assert {hc.Cin for hc in HEADS if hc.mode == 3 and not hc.tail} == {64, 40}
    assert {(hc.h, hc.w) for hc in HEADS if hc.tail} == {(17, 21), (20, 20), (3, 5)}
    runs, ref = sum(len(valid_ids(hc)) for hc in HEADS) * len(VARIANTS), sum(len(hc.refused) for hc in HEADS) * len(VARIANTS)
    print("head16: %d cases, %d (case, variant, id) runs and %d refused presets per payload kind" % (len(HEADS), runs, ref))


def _rand_stage(hc):
    """The operands of the decoding 1x1 stage of a random payload on the CPU: the payload's own for a 1x1 op; for a tail the f16 map
    of a float32 evaluation of its 3x3 conv + SiLU and the 1x1 record (on the GPU the map is the one read back from the device)."""
    c = _rand(hc.payload)
    if not hc.tail:
        return c.x, c.w, c.b
    mid = F.silu(nhwc(F.conv2d(nchw(c.x), c.w, c.b, 1, 1))).to(F16).to(F32)
    return mid, c.w2, c.b2


def test_cpu_float32_within_half_the_bound():
    """A float32 evaluation of every random payload's logits by torch on the CPU (another summation order than any kernel's), decoded
    in fp64 so that only the conv's arithmetic differs: the logits use at most half of E, the class scores at most half of E / 4 and
    the boxes at most half of the carried side bounds -- half of the arithmetic part of each bound of _bounds."""
    worst, n = {"raw": 0.0, "class": 0.0, "box": 0.0}, 0
    for hc in {hc.payload: hc for hc in HEADS}.values():
        x, w, b = _rand_stage(hc)
        l32 = nhwc(F.conv2d(nchw(x), w, b))
        assert l32.dtype == F32
        l, S = _logits(x, w, b)
        (y_ar, _), (raw_ar, _) = _bounds(hc, l, S, x.shape[-1], F32)
        zero = torch.zeros((), dtype=F64)
        r_raw = _worst(nchw(l32), nchw(l), raw_ar, zero)[0]
        r_y = _worst(_decode(hc, l32.to(F64)), _decode(hc, l), y_ar, zero)[0]
        assert r_raw <= 0.5 and r_y <= 0.5, (hc.name, r_raw, r_y)
        worst["raw"] = max(worst["raw"], r_raw)
        kind = "class" if hc.mode == 2 else "box"
        worst[kind] = max(worst[kind], r_y)
        n += 1
    print("CPU float32: worst error / arithmetic part over %d payloads: logits %.3f, class scores %.3f, boxes %.3f"
          % (n, worst["raw"], worst["class"], worst["box"]))


# ------------------------------------------------------------------------------------------------------------
# 1. dyadic payloads: the raw map bit for bit, y within the decode bound, one answer under every id
# ------------------------------------------------------------------------------------------------------------
def _decode_check(y, ref, odt, tag):
    r = _worst(y, ref, torch.zeros((), dtype=F64), _decode_part(ref, odt))[0]
    assert r <= 1.0, "%s: %.3f of the decode bound" % (tag, r)
    return r


@gpu
@pytest.mark.parametrize("hc", HEADS, ids=HEAD_IDS)
def test_head_exact(hc):
    """Under every id, in f16 and f32, with and without a raw map: the raw map holds the fp64 logits bit for bit (a wrong channel,
    pixel, lane half or image shows as another dyadic number, a read outside a view as NaN), y lies within the decode bound of the fp64
    decode, and all ids return the same bits of y -- for f16 class scores also both epilogues (conv_epilogue_cls_lds without a raw
    map, conv_epilogue_head with one).  The tail returns the bits of the 1x1 decoding op run on the exact intermediate map."""
    c = _exact(hc.payload)
    ref = _decode(hc, c.l)
    ids, first = valid_ids(hc), {}
    for odt, raw in VARIANTS:
        outs = _run(hc, c, odt, raw)
        assert set(outs) == set(ids)
        want_raw = bits(nchw(c.l).to(odt))
        worst = {}
        for cfg, (y, rw) in outs.items():
            tag = "%s %s raw %s under 0x%02x" % (hc.name, odt, raw, cfg)
            if raw == "bound":
                assert torch.equal(bits(rw), want_raw), tag + ": the raw map is not the logits"
            fam = family(hc, odt, raw, cfg)
            worst[fam] = max(worst.get(fam, 0.0), _decode_check(y, ref, odt, tag))
            assert torch.equal(bits(y), bits(outs[ids[0]][0])), "%s: 0x%02x and 0x%02x differ" % (hc.name, cfg, ids[0])
        for fam, r in worst.items():
            print("head16 exact %s %s raw %s [%s] %d ids: worst error / decode bound = %.3f" % (hc.name, str(odt)[6:], raw, fam, len(ids), r))
        y0 = outs[ids[0]][0]
        assert torch.equal(bits(y0), bits(first.setdefault(odt, y0))), "%s %s: y with and without a raw map differs" % (hc.name, odt)
        if hc.tail:
            one = replace(hc, tail=False)
            y1, rw1 = _run(one, c, odt, raw, ids=(0x11,), refused=(), x=c.mid, convs=[(c.w2, c.b2)])[0x11]
            assert torch.equal(bits(y1), bits(y0)), "%s %s: the tail and the 1x1 op on the exact map differ" % (hc.name, odt)
            assert raw != "bound" or torch.equal(bits(rw1), want_raw)


# ------------------------------------------------------------------------------------------------------------
# 2. random payloads: fp64 under the derived bound; the tail against the two launches it replaces
# ------------------------------------------------------------------------------------------------------------
def _held(hc, tag, fam, n, odt, raw, y, rw, l, S, K):
    """y and the raw map of one run against the fp64 decode of l under _bounds; prints the figures, then asserts."""
    (y_ar, y_rest), (raw_ar, raw_rest) = _bounds(hc, l, S, K, odt)
    r, share = _worst(y, _decode(hc, l), y_ar, y_rest)
    rr, rshare = _worst(rw, nchw(l), raw_ar, raw_rest) if raw == "bound" else (0.0, 0.0)
    print("head16 %s %s raw %s [%s] %d ids: y worst error / bound = %.3f, share of the arithmetic part %.3f; raw map %.3f, %.3f"
          % (tag, str(odt)[6:], raw, fam, n, r, share, rr, rshare))
    assert r <= 1.0 and rr <= 1.0, "%s: y %.3f, raw map %.3f of the bound" % (tag, r, rr)


@gpu
@pytest.mark.parametrize("hc", [hc for hc in HEADS if not hc.tail], ids=[hc.name for hc in HEADS if not hc.tail])
def test_head_random_within_derived_bound(hc):
    """|got - fp64| <= _bounds for y and the raw map under every id, all ids return identical bits, and y has the same bits with and
    without a raw map (f16 class scores: the two epilogues)."""
    c = _rand(hc.payload)
    l, S = _logits(c.x, c.w, c.b)
    ids, first = valid_ids(hc), {}
    for odt, raw in VARIANTS:
        outs = _run(hc, c, odt, raw)
        assert set(outs) == set(ids)
        y0, rw0 = outs[ids[0]]
        for cfg, (y, rw) in outs.items():
            assert torch.equal(bits(y), bits(y0)) and (rw is None or torch.equal(bits(rw), bits(rw0))), "%s: 0x%02x and 0x%02x differ" % (hc.name, cfg, ids[0])
        _held(hc, hc.name, family(hc, odt, raw, ids[0]), len(ids), odt, raw, y0, rw0, l, S, hc.Cin)
        assert torch.equal(bits(y0), bits(first.setdefault(odt, y0))), "%s %s: y with and without a raw map differs" % (hc.name, odt)


@gpu
@pytest.mark.parametrize("hc", [hc for hc in HEADS if hc.tail], ids=[hc.name for hc in HEADS if hc.tail])
def test_tail_random_equals_two_launches(hc):
    """The tail's y and raw map equal, bit for bit and under all six tail ids, what the plain 3x3 CONV op (SiLU, 64 couts, the same
    patch id, held to fp64 by test_fp16_conv_ops) into an f16 map followed by the 1x1 decoding op on that map returns -- the claim
    "same bits" of csrc/conv_patch.hip -- and the two launches lie within _bounds of the fp64 evaluation whose input is that map,
    read back."""
    c = _rand(hc.payload)
    for odt, raw in VARIANTS:
        outs = _run(hc, c, odt, raw)
        assert set(outs) == set(TAIL_IDS)
        held = None
        for pid in TAIL_IDS:
            y2, rw2, mid = _run_two_launches(hc, c, odt, raw, pid)
            y, rw = outs[pid]
            assert torch.equal(bits(y), bits(y2)), "%s %s under 0x%02x: y of the tail and of the two launches differ" % (hc.name, odt, pid)
            assert rw is None or torch.equal(bits(rw), bits(rw2)), "%s %s under 0x%02x: the raw maps differ" % (hc.name, odt, pid)
            if held is None or not torch.equal(bits(mid), bits(held)):  # (the patch ids return one map: one reference)
                held = mid
                l, S = _logits(mid.to(F32), c.w2, c.b2)
                _held(replace(hc, tail=False), "%s from 0x%02x on" % (hc.name, pid), family(hc, odt, raw, pid), 1, odt, raw, y2, rw2, l, S, 64)


# ------------------------------------------------------------------------------------------------------------
# 3. refusals through the plan interface
# ------------------------------------------------------------------------------------------------------------
def _refusal(what):
    """-> (case, a function that spoils the op of a set-up case)."""
    cl, bx, tl = Head("", 2, 5, 5, 7, 41, nc=5), Head("", 3, 5, 5, 7, 41), Head("", 3, 5, 5, 7, 41, tail=True)

    def shortcut(t):
        t.op.res = view(3, 16, 0, 8)
        t.ext = t.ext + [torch.zeros((cl.B, cl.h, cl.w, 16), dtype=F16, device="cuda:0")]

    def ksize1(t):
        t.op.ksize, t.op.pad = 1, 0

    return {
        "a0 + h w > A": (cl, lambda t: setattr(t.op, "A", cl.a0 + cl.hw - 1)),
        "nrows < 4 + nc": (cl, lambda t: setattr(t.op, "dst", view(1, 0, 0, 4 + cl.nc - 1))),
        "epi 3 with nl 32": (bx, lambda t: setattr(t.op, "nl", 32)),
        "rawC of 64 + nc - 1": (cl, lambda t: t.op.box.__setitem__(0, view(2, 0, 0, 64 + cl.nc - 1))),
        "a shortcut view": (cl, shortcut),
        "a tail with ksize 1": (tl, ksize1),
    }[what]


REFUSALS = ("a0 + h w > A", "nrows < 4 + nc", "epi 3 with nl 32", "rawC of 64 + nc - 1", "a shortcut view", "a tail with ksize 1")


@gpu
@pytest.mark.parametrize("what", REFUSALS)
def test_head_refusals(what):
    """launch_conv refuses the op with a BsyError before anything is launched: y and the raw map still hold their poison."""
    hc, spoil = _refusal(what)
    t = _setup(hc, _exact(hc.payload), F16, "bound")
    spoil(t)
    with pytest.raises(L.BsyError):
        run_op(t.op, t.ext, t.blob)
    torch.cuda.synchronize()
    _assert_rest_is_poison(t.y.cpu(), (slice(0, 0),), t.poison, "y")
    _assert_rest_is_poison(t.raw.cpu(), (slice(0, 0),), t.poison, "the raw map")
