"""The fp16 CONV op ALONE, across its kernel families: BSY_OP_CONV with prec 0 as one-op plans (op_plan_helpers.run_conv_cfgs) on channel
views of poisoned buffers -- f16 NaN around every source and between the weight records, 777 (7.77e7 for out_f32) around every
destination, -777 around every shortcut, NaN in the split-K slabs -- as tests/test_fp32_matrix_ops.py does for the fp32-storage
modes.  This reaches what ops.conv2d_nhwc cannot pass: two sources with row strides of their own, nearest x2 on either, the dst_scale = 2 phases of a
ConvTranspose2d, out_f32 on an offset view, split-K, a shortcut that is an offset view, and destinations the coalesced LDS epilogue
refuses -- each under EVERY kernel configuration id of csrc/conv_select.hip that the layer admits, preset through
bsy_plan_set_tuning and confirmed by bsy_plan_check_tuning (a preset that is not valid would silently run the heuristic id).

Two kinds of comparison.  Integer payloads (every result an integer of magnitude <= 2048, exact in f16) have ONE right answer whatever
the summation order and the epilogue, and are compared bit for bit with an fp64 evaluation.  Random payloads are compared with fp64
under a bound derived per output element from the operands (see _bound), never from the output range;
test_cpu_float32_within_half_the_bound shows on the CPU that a correct float32 evaluation uses less than half of its arithmetic part.

cfg_valid below mirrors conv_cfg_valid (csrc/conv_select.hip); it is written from the C++, the table test holds the case list to it
and the GPU tests hold the library to the case list.  The GPU tests are marked ``gpu`` one by one: the two tests about the case
table and the bound run anywhere.

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

from op_plan_helpers import (NAN, PHASES, POISON16, POISON32, _bound, _u16, _worst, assert_poison_intact, bits, conv16_blob, conv16_op,  # noqa: F401
                             nchw, nhwc, poisoned, run_conv_cfgs, run_op, view)

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from bs_yolo_amd import lib as L  # noqa: F401  (fails loudly when the .so is missing)

F32, F16, F64 = torch.float32, torch.float16, torch.float64


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# ------------------------------------------------------------------------------------------------------------
# the configuration table, read from the C++ source, and conv_cfg_valid mirrored
# ------------------------------------------------------------------------------------------------------------
def _table_ids():
    """The ids of kConvCfgs (without the chunk-major bit), from the text of csrc/conv_select.hip."""
    src = (Path(__file__).resolve().parents[1] / "bs_yolo_amd" / "csrc" / "conv_select.hip").read_text()
    body = src[src.index("kConvCfgs[] = {"):]
    body = body[:body.index("};")]
    return sorted({int(m, 16) for m in re.findall(r"_row<[^>]*>\((0x[0-9A-Fa-f]+)\)", body)})


TABLE = _table_ids()
GEMM_TN = {0: 32, 1: 64, 2: 128, 3: 64, 4: 128, 5: 128, 6: 64, 7: 256}  # cout tile of the implicit-GEMM tiles 0x0x .. 0x7x


def cfg_row(cfg):
    """What a row of kConvCfgs says about an id: family, cout tile, K-step, DMA ring depth, aligned operands."""
    t, v = (cfg & ~4) >> 4, (cfg & ~4) & 15
    if t <= 7:
        return SimpleNamespace(fam="gemm", tn=GEMM_TN[t], bk=64 if v == 3 else 32, stages=3 if v < 2 else 2, aligned=v != 0, nfr=0)
    if t <= 9:
        return SimpleNamespace(fam="persist", tn=128 if t == 8 else 64, bk=64 if v == 3 else 32, stages=3 if v < 2 else 2, aligned=True, nfr=0)
    if t <= 0xD:
        return SimpleNamespace(fam="patch", tn=128 if t in (0xA, 0xC) else 64, bk=32, stages=0, aligned=True, nfr=0)
    return SimpleNamespace(fam="wres", tn=128 if t == 0xE else 64, bk=32, stages=4 if v == 1 else 3, aligned=True, nfr=24 if t == 0xE else 32)


def family(ly, cfg):
    """The family a (layer, id) pair is reported under in docs/experiments.md."""
    r, t, v = cfg_row(cfg), (cfg & ~4) >> 4, (cfg & ~4) & 15
    if ly.nsl > 1:
        return "split-K"
    if ly.deconv:
        return "deconv"
    if ly.out_f32:
        return "out_f32"
    if r.fam != "gemm":
        return {"persist": "persistent", "wres": "weights-resident", "patch": "patch"}[r.fam]
    return "generic" if v == 0 else ("8-wave tiles" if t in (4, 7) else ("BK 64" if v == 3 else "aligned BK 32"))


# ------------------------------------------------------------------------------------------------------------
# the layer list
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
    B: int = 2
    H: int = 12           # the conv's input map (a deconv: the 6 x 5 map the four phases read)
    W: int = 14
    res: bool = False     # a shortcut: an offset view with a row stride of its own
    deconv: bool = False  # the four dst_scale = 2 phases of a ConvTranspose2d(C0, Cout, 2, 2)
    out_f32: bool = False
    split: tuple = (1, 1)  # (nsl_c, nsl_t)
    place: str = "a"      # "a": destination and shortcut on 16-byte boundaries; "m4": channel offsets % 8 == 4; "ld4": row strides % 8 == 4
    ids: tuple = ()       # configuration ids that must run ...
    refused: tuple = ()   # ... and ids bsy_plan_check_tuning must answer 0 for

    @property
    def Cin(self):
        return self.C0 + self.C1

    @property
    def K(self):
        return self.k * self.k * self.Cin

    @property
    def nsl(self):
        return self.split[0] * self.split[1]

    @property
    def payload(self):
        """The layer without what only places, splits or routes it: layers with equal payloads share inputs and reference."""
        return replace(self, name="", split=(1, 1), place="a", ids=(), refused=())

    @property
    def out_hw(self):
        """The op's OH x OW (the destination of a deconv holds twice that)."""
        p = self.k // 2
        return (self.H + 2 * p - self.k) // self.s + 1, (self.W + 2 * p - self.k) // self.s + 1

    @property
    def korder(self):
        """conv_korder (csrc/conv_select.hip)."""
        if self.k != 3 or self.Cin & 31 or self.C0 & 31:
            return 0
        return 2 if self.s == 2 and not self.Cin & 63 and not self.C0 & 63 else 1


def _gemm(tiles, variants, km=0):
    return tuple(t << 4 | v | km for t in tiles for v in variants)


GEN = _gemm((0, 1, 2, 3, 5, 6), (0,))
PERSIST, WRES = (0x81, 0x82, 0x83, 0x91, 0x92, 0x93), (0xE1, 0xE2, 0xF1, 0xF2)
PATCH = (0xA1, 0xB1, 0xB2, 0xB3, 0xC1, 0xD1, 0xD2, 0xD3)


def _layers():
    ls = []
    # 1. generic, two sources, 1x1 (M = 336: a ragged second 256-pixel tile)
    ls.append(Layer("gen1x1-8+16-24", C0=8, C1=16, Cout=24, ids=GEN, refused=(0x01, 0x91, 0xF1)))
    ls.append(Layer("gen1x1-40up+8-68", C0=40, C1=8, up0=1, Cout=68, ids=GEN, refused=(0x21, 0x92)))  # Cout % 8: the direct epilogue
    # 2. generic 3x3: K = 216 ends inside a 32-step
    for s in (1, 2):
        ls.append(Layer("gen3x3-24-s%d" % s, 3, s, 24, Cout=40, B=2 if s == 1 else 3, H=13, W=11, ids=GEN, refused=(0x04, 0x01)))
    # 3. aligned 1x1, two sources, nearest x2 on either
    bk32 = _gemm(range(7), (1, 2))
    ls.append(Layer("cat1x1-64up+32-48", C0=64, C1=32, up0=1, Cout=48, ids=bk32 + (0x81, 0x82, 0x91, 0x92, 0xF1, 0xF2),
                    refused=(0x03, 0x83, 0x93, 0xE1, 0xE2, 0x71)))
    ls.append(Layer("cat1x1-64up+32-136", C0=64, C1=32, up0=1, Cout=136, ids=bk32 + (0x20, 0x81, 0x82, 0x91, 0x92) + WRES,
                    refused=(0x13, 0x83, 0x72)))
    ls.append(Layer("cat1x1-64+128up-256", C0=64, C1=128, up1=1, Cout=256, H=12, W=12, ids=_gemm(range(8), (1, 2, 3)) + (0x00, 0x60) + PERSIST + WRES,
                    refused=(0x05, 0xB1, 0x40)))
    # 4. 3x3 stride 1, K walk 1 (M = 357)
    for cin in (64, 96):
        for res in (False, True):
            ls.append(Layer("k3s1-%d-72%s" % (cin, "-res" if res else ""), 3, 1, cin, Cout=72, B=1, H=17, W=21, res=res,
                            ids=(0x15, 0x16, 0x25, 0x26, 0x35, 0x36, 0x55, 0x65, 0x05, 0x46) + PATCH, refused=(0x17, 0x11, 0x91)))
    # 5. 3x3 stride 2: K walk 2 on two sources, K walk 1
    ls.append(Layer("k3s2-64+64-256", 3, 2, 64, 64, Cout=256, B=3, H=18, W=14, ids=_gemm(range(8), (5, 6, 7)), refused=(0x13, 0xB1)))
    ls.append(Layer("k3s2-96-48", 3, 2, 96, Cout=48, B=3, H=18, W=14, ids=_gemm((0, 1, 2, 3, 5, 6), (5, 6)), refused=(0x17, 0xB2)))
    # 6. ConvTranspose2d phases: 6 x 5 -> one view of 12 x 10
    ls.append(Layer("deconv-64-64", C0=64, Cout=64, B=3, H=6, W=5, deconv=True, ids=(0x10, 0x11, 0x12, 0x13, 0x21, 0x31, 0x33, 0x61, 0x62, 0x63),
                    refused=(0x91, 0xF1, 0xB1)))
    ls.append(Layer("deconv-40-136", C0=40, Cout=136, B=3, H=6, W=5, deconv=True, ids=GEN, refused=(0x21,)))
    # 7. out_f32 on an f32 view at channel offset 4
    ls.append(Layer("f32-64-80", C0=64, Cout=80, out_f32=True, ids=(0x11, 0x20, 0x21, 0x22, 0x23, 0x31, 0x51, 0x61, 0x63), refused=(0x91, 0xF1, 0xE1)))
    ls.append(Layer("f32-16-5", C0=16, Cout=5, out_f32=True, ids=GEN, refused=(0x01,)))
    # 8. split-K, each with a shortcut view
    for sp in ((1, 3), (2, 3), (4, 1), (1, 9)):  # (2, 3) and (4, 1): channel slices of 64 and 32 against C0 = 32
        ls.append(Layer("split%dx%d-k3s1-32+96-64" % sp, 3, 1, 32, 96, Cout=64, B=2, H=10, W=10, res=True, split=sp,
                        ids=(0x15, 0x16, 0x25, 0x35, 0x36, 0x65, 0x66), refused=(0x17, 0x14, 0xB1)))
    for sp in ((8, 1), (4, 1)):  # Cout 72: slab rows of ldw = 96
        ls.append(Layer("split%dx%d-1x1-512-72" % sp, C0=512, Cout=72, res=True, split=sp,
                        ids=(0x11, 0x12, 0x13, 0x21, 0x23, 0x31, 0x33, 0x61, 0x63), refused=(0x10, 0x91)))
    ls.append(Layer("split2x3-k3s2-256-64", 3, 2, 256, Cout=64, B=3, H=14, W=10, res=True, split=(2, 3),
                    ids=(0x15, 0x16, 0x17, 0x27, 0x35, 0x37, 0x65, 0x67), refused=(0xB1, 0x11)))
    # 9. misaligned twins: the implicit-GEMM ids run (direct epilogue), every other family is refused
    by = {ly.name: ly for ly in ls}
    ls.append(replace(by["cat1x1-64up+32-48"], name="m4-cat1x1-64up+32-48", place="m4", ids=bk32, refused=PERSIST + WRES))
    ls.append(replace(by["k3s1-64-72-res"], name="ld4-k3s1-64-72-res", place="ld4", ids=(0x15, 0x16, 0x25, 0x26, 0x35, 0x36, 0x55, 0x65),
                      refused=PATCH))
    return ls


LAYERS = _layers()
LAYER_IDS = [ly.name for ly in LAYERS]


def _r8(n):
    return (n + 7) // 8 * 8


def _geom(ly):
    """Row strides and channel offsets of the operands, in elements.  Every buffer is wider than its view, ld0 != ld1 and ldd != ldr.
    At least 8 elements of the row follow every destination and shortcut view, so that a store or load one 16-byte piece past the
    view stays inside its own row."""
    g = SimpleNamespace(c0=8, ld0=_r8(ly.C0) + 16, c1=16, ld1=_r8(ly.C1) + 24, cd=8, ldd=_r8(ly.Cout) + 24, cr=16, ldr=_r8(ly.Cout) + 32)
    if ly.out_f32:
        g.cd = 4
    if ly.place == "m4":
        g.cd, g.cr = 4, 12
    if ly.place == "ld4":
        g.ldd, g.ldr = g.ldd + 4, g.ldr + 4
    return g


def lds_form(ly):
    """conv_mfma_kernel's choice of conv_epilogue_lds over conv_epilogue (csrc/conv_gemm.hip); a split layer takes neither."""
    g = _geom(ly)
    ok = not ly.out_f32 and not ly.Cout & 7 and not g.ldd & 7 and not g.cd & 7 and not ly.deconv
    return ok and (not ly.res or (not g.ldr & 7 and not g.cr & 7)) and ly.nsl == 1


def cfg_valid(ly, cfg):
    """conv_cfg_valid (csrc/conv_select.hip) for a layer placed by _geom (buffers start on 256-byte boundaries)."""
    if (cfg & ~4) not in TABLE:
        return False
    r, g, ko, Cin = cfg_row(cfg), _geom(ly), ly.korder, ly.Cin
    aligned, aligned64 = not (Cin & 31 or ly.C0 & 31), not (Cin & 63 or ly.C0 & 63)
    if (r.aligned and not aligned) or (r.bk == 64 and not aligned64):
        return False
    if r.fam == "gemm":
        if bool(cfg & 4) != bool(ko):
            return False
        if ko and (not r.aligned or (ko == 1 and r.bk == 64)):
            return False
        if ly.nsl > 1 and (not r.aligned or (Cin // ly.split[0]) % r.bk):
            return False
        return r.tn != 256 or not ly.Cout & 255
    if cfg & 4 or ly.nsl > 1:
        return False
    if ly.out_f32 or ly.Cout & 7 or g.ldd & 7 or g.cd & 7 or ly.deconv:
        return False
    if r.fam in ("persist", "wres"):
        if ly.k != 1 or ly.s != 1 or ly.res:
            return False
        if r.fam == "persist":
            return ly.Cout <= 1024
        return (r.tn // 64) * (Cin // 16) <= r.nfr and Cin // 32 >= r.stages - 1 and (r.tn != 128 or ly.Cout > 64)
    return (ko == 1 and ly.k == 3 and ly.s == 1 and not ly.C1 and not ly.up0 and (not ly.res or (not g.ldr & 7 and not g.cr & 7))
            and (r.tn != 128 or ly.Cout > 64))


# ------------------------------------------------------------------------------------------------------------
# payloads, fp64 references and the bound
# ------------------------------------------------------------------------------------------------------------
def _lin(ly):
    def lin(xs, w, b):
        if ly.deconv:
            return nhwc(F.conv_transpose2d(nchw(xs[0]), w, b, stride=2))
        maps = [F.interpolate(nchw(x), scale_factor=2.0, mode="nearest") if up else nchw(x)
                for x, up in zip(xs, (ly.up0, ly.up1)) if x is not None]
        return nhwc(F.conv2d(torch.cat(maps, 1), w, b, ly.s, ly.k // 2))
    return lin


@lru_cache(maxsize=None)
def _inputs(pl, kind):
    """Operands of a layer payload, drawn once, as float32 tensors of f16-representable values (the bias: any f32).  "int": inputs in
    [-3, 3], weights in {-1, 0, 1}, integer bias and shortcut in [-8, 8].  "rand": randn inputs with every third channel scaled by 1e-3,
    weights randn * sqrt(2 / K), bias randn / 2, shortcut randn."""
    g = _gen(pl.k, pl.s, pl.C0, pl.C1, pl.up0, pl.up1, pl.Cout, pl.B, pl.H, pl.W, pl.res, pl.deconv, pl.out_f32, kind == "int")
    oh, ow = pl.out_hw
    shapes = [(pl.B, pl.H >> pl.up0, pl.W >> pl.up0, pl.C0), (pl.B, pl.H >> pl.up1, pl.W >> pl.up1, pl.C1) if pl.C1 else None]
    wshape = (pl.C0, pl.Cout, 2, 2) if pl.deconv else (pl.Cout, pl.Cin, pl.k, pl.k)
    rshape = (pl.B, oh, ow, pl.Cout) if pl.res else None
    h = lambda t: t.to(F16).to(F32)
    if kind == "int":
        draw = lambda shp, lim: torch.randint(-lim, lim + 1, shp, generator=g).float()
        xs = tuple(None if s is None else draw(s, 3) for s in shapes)
        w, b = draw(wshape, 1), draw((pl.Cout,), 8)
        res = draw(rshape, 8) if rshape else None
    else:
        xs = []
        for s in shapes:
            x = None if s is None else torch.randn(s, generator=g)
            if x is not None:
                x[..., ::3] *= 1e-3
                x = h(x)
            xs.append(x)
        xs = tuple(xs)
        w, b = h(torch.randn(wshape, generator=g) * (2.0 / pl.K) ** 0.5), torch.randn(pl.Cout, generator=g) * 0.5
        res = h(torch.randn(rshape, generator=g)) if rshape else None
    return SimpleNamespace(xs=xs, w=w, b=b, res=res, act=kind != "int")


@lru_cache(maxsize=None)
def _case(pl, kind):
    """_inputs plus the fp64 evaluation: v (pre-activation), a = act(v), ref = y = a + r, S = |b| + sum |x_i| |w_i| over the taps inside
    the map.  An integer payload must be exact in every format on the way: v and y integers of magnitude <= 2048, S < 2^24."""
    c = _inputs(pl, kind)
    d = lambda t: None if t is None else t.to(F64)
    lin = _lin(pl)
    xs64, w64, b64 = tuple(d(x) for x in c.xs), d(c.w), d(c.b)
    v = lin(xs64, w64, b64)
    a = F.silu(v) if c.act else v
    y = a + d(c.res) if c.res is not None else a
    S = lin(tuple(None if x is None else x.abs() for x in xs64), w64.abs(), b64.abs())
    if kind == "int":
        assert bool((v == v.round()).all()) and bool((y == y.round()).all())
        assert float(v.abs().max()) <= 2048 and float(y.abs().max()) <= 2048 and float(S.max()) < 2 ** 24
        y = y + 0.0  # no kernel returns -0 here: the chains start at a +0 or non-zero bias
    return SimpleNamespace(xs=c.xs, w=c.w, b=c.b, res=c.res, act=c.act, lin=lin, v=v, a=a, ref=y, S=S)


# ------------------------------------------------------------------------------------------------------------
# one layer as a plan on poisoned views
# ------------------------------------------------------------------------------------------------------------
def _setup(ly, c, phases=PHASES):
    """Buffers, weight blob and ops of a layer (a deconv: one op per phase in `phases`, each with its own weight record).  External
    slots: 0 / 1 the sources, 2 the destination, 3 the shortcut, 4 the split-K slabs."""
    g = _geom(ly)
    oh, ow = ly.out_hw
    sc = 2 if ly.deconv else 1
    M, ldw = ly.B * oh * ow, (ly.Cout + 31) // 32 * 32
    t = SimpleNamespace(g=g, odt=F32 if ly.out_f32 else F16, poison=POISON32 if ly.out_f32 else POISON16)
    t.s0 = poisoned((ly.B, ly.H >> ly.up0, ly.W >> ly.up0, g.ld0), g.c0, ly.C0, c.xs[0].to(F16), NAN)
    t.s1 = poisoned((ly.B, ly.H >> ly.up1, ly.W >> ly.up1, g.ld1), g.c1, ly.C1, c.xs[1].to(F16), NAN) if ly.C1 else None
    t.dst = poisoned((ly.B, oh * sc, ow * sc, g.ldd), g.cd, ly.Cout, None, t.poison, dtype=t.odt)
    # the shortcut's poison is -777: with the destination's own 777 a 16-byte piece stored past the view of a shortcut layer would hold
    # 0 (the padded couts) + 777 and go unseen
    t.rbuf = poisoned((ly.B, oh, ow, g.ldr), g.cr, ly.Cout, c.res.to(F16), -POISON16) if ly.res else None
    t.slab = None
    if ly.nsl > 1:  # nsl slabs of NaN (a slab element nobody wrote reaches the output) + one more slab's worth of poison
        t.used = ly.nsl * M * ldw
        t.slab = torch.full((t.used + M * ldw,), NAN, dtype=F32)
        t.slab[t.used:] = POISON32
        t.slab = t.slab.to("cuda:0")
    t.pristine = [None if b is None else b.clone() for b in (t.dst, t.rbuf, t.slab)]
    t.blob, recs = conv16_blob(c.w, c.b, ly.deconv, phases)
    t.ops = [conv16_op(ly.B, ly.H, ly.W, ly.k, ly.s, ly.k // 2, view(0, g.ld0, g.c0, ly.C0), view(2, g.ldd, g.cd, ly.Cout), w_off, b_off,
                       src1=view(1, g.ld1, g.c1, ly.C1) if ly.C1 else None, up0=ly.up0, up1=ly.up1,
                       res=view(3, g.ldr, g.cr, ly.Cout) if ly.res else None, act=int(c.act), out_f32=int(ly.out_f32), dst_scale=sc,
                       dst_dy=dy, dst_dx=dx, nsl_c=ly.split[0], nsl_t=ly.split[1], slab=view(4, ldw, 0, ldw))
             for w_off, b_off, dy, dx in recs]
    t.ext = [t.s0, t.s1, t.dst, t.rbuf, t.slab]
    return t


def _run(ly, c, ids=None, refused=None, phases=PHASES):
    """The layer under every id of `ids` (default: the layer's own lists) -> {id: the destination view on the host}.  After every run:
    the destination outside its view, the whole shortcut buffer and the poison behind the slabs are intact bit for bit."""
    t = _setup(ly, c, phases)

    def reset():
        t.dst.copy_(t.pristine[0])
        if t.slab is not None:
            t.slab.copy_(t.pristine[2])

    def collect():
        assert_poison_intact(t.dst, t.g.cd, ly.Cout, t.poison)
        if t.rbuf is not None:
            assert torch.equal(bits(t.rbuf), bits(t.pristine[1])), "a store reached the shortcut buffer"
        if t.slab is not None:
            assert torch.equal(bits(t.slab[t.used:]), bits(t.pristine[2][t.used:])), "a store left the split-K slabs"
        return t.dst[..., t.g.cd:t.g.cd + ly.Cout].cpu()

    return run_conv_cfgs(t.ops, t.ext, t.blob, ly.ids if ids is None else ids, ly.refused if refused is None else refused, reset, collect)


# ------------------------------------------------------------------------------------------------------------
# the case table and the bound, anywhere
# ------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_configuration():
    """Every id of kConvCfgs runs in at least one case; every family runs on two sources at least once (the patch kernel takes one
    source by its rule): the implicit GEMM generic and aligned, BK 32 with 3 and 2 stages and BK 64, the persistent and the
    weights-resident kernel.  The ids a case lists are valid for it by cfg_valid and the refused ones are not; the geometry is the one
    the module's docstring promises; every integer payload is exact (the assertions of _case)."""
    ran = {i & ~4 for ly in LAYERS for i in ly.ids}
    assert len(TABLE) == 48 and set(TABLE) <= ran, [hex(i) for i in sorted(set(TABLE) - ran)]
    two = set()
    for ly in LAYERS:
        for i in ly.ids if ly.C1 else ():
            r = cfg_row(i)
            two.add((r.fam, r.aligned, r.bk, r.stages) if r.fam == "gemm" else r.fam)
    want = {("gemm", False, 32, 3), ("gemm", True, 32, 3), ("gemm", True, 32, 2), ("gemm", True, 64, 2), "persist", "wres"}
    assert want <= two, want - two
    for fam, lo, hi in (("gemm", 0x00, 0x7F), ("persist", 0x80, 0x9F), ("patch", 0xA0, 0xDF), ("wres", 0xE0, 0xFF)):
        assert all(cfg_row(i).fam == fam for i in TABLE if lo <= i <= hi)
    assert len(set(LAYER_IDS)) == len(LAYERS)
    for ly in LAYERS:
        g = _geom(ly)
        assert ly.ids and not set(ly.ids) & set(ly.refused), ly.name
        assert all(cfg_valid(ly, i) for i in ly.ids), (ly.name, [hex(i) for i in ly.ids if not cfg_valid(ly, i)])
        assert not any(cfg_valid(ly, i) for i in ly.refused), (ly.name, [hex(i) for i in ly.refused if cfg_valid(ly, i)])
        # sources: offsets and strides multiples of 8, wider than the view, the two strides different
        assert g.c0 % 8 == 0 and g.ld0 % 8 == 0 and g.ld0 >= g.c0 + ly.C0 and g.c1 % 8 == 0 and g.ld1 % 8 == 0 and g.ld1 >= g.c1 + ly.C1
        assert g.ld0 != g.ld1 and g.ldd != g.ldr
        assert g.ldd >= g.cd + ly.Cout + 8 and g.ldr >= g.cr + ly.Cout + 8
        if ly.place == "a":
            assert g.ldd % 8 == 0 and g.ldr % 8 == 0 and g.cr % 8 == 0 and g.cd % (4 if ly.out_f32 else 8) == 0
        else:  # what launch_conv still accepts: ld % 4, pointer % 8 bytes
            assert (g.cd % 8 == 4 and g.cr % 8 == 4) if ly.place == "m4" else (g.ldd % 8 == 4 and g.ldr % 8 == 4)
            assert not lds_form(ly) and lds_form(replace(ly, place="a")) and all(cfg_row(i).fam == "gemm" for i in ly.ids)
            assert {cfg_row(i).fam for i in ly.refused} >= ({"persist", "wres"} if ly.k == 1 else {"patch"})
        assert ly.B <= 3 and ly.H <= 24 and ly.W <= 24 and (ly.K <= 1152 or ly.nsl > 1)
        assert not (ly.up0 or ly.up1) or (ly.H % 2 == 0 and ly.W % 2 == 0 and ly.k == 1)
        oh, ow = ly.out_hw
        M = ly.B * oh * ow
        assert M > 64 and M % 64, ly.name  # two tiles of the smallest kind and a ragged last tile of every kind
        if ly.nsl > 1:
            assert ly.Cin % ly.split[0] == 0 and (ly.Cin // ly.split[0]) % 32 == 0 and (ly.k * ly.k) % ly.split[1] == 0 and ly.res
        _case(ly.payload, "int")
    assert any(ly.nsl > 1 and ly.C1 and 0 < ly.C0 % (ly.Cin // ly.split[0]) for ly in LAYERS)  # a slice straddles the two sources
    assert any(ly.nsl > 1 and ly.Cout % 32 for ly in LAYERS)                                     # slab rows wider than Cout


def test_cpu_float32_within_half_the_bound():
    """A float32 evaluation of every random payload by torch on the CPU (another summation order than any kernel's), rounded as each
    of the two forms rounds: before the rounding it uses at most half of the bound's arithmetic part, and the rounded value stays
    within that half plus the rounding part -- which a correctly rounded result can use up entirely, so it is not halved."""
    worst, n = 0.0, 0
    for pl in dict.fromkeys(ly.payload for ly in LAYERS):
        c = _case(pl, "rand")
        a32 = F.silu(c.lin(c.xs, c.w, c.b))
        assert a32.dtype == F32
        arith, _ = _bound(pl, c, False)
        worst = max(worst, _worst(a32, c.a, arith))
        for two in ((False, True) if pl.res else (False,)):
            _, rnd = _bound(pl, c, two)
            if pl.out_f32:
                y = a32
            elif two:
                y = (a32.to(F16).to(F32) + c.res).to(F16)
            else:
                y = (a32 + c.res if pl.res else a32).to(F16)
            assert _worst(y, c.ref, 0.5 * arith + rnd) <= 1.0, pl
        n += 1
    print("CPU float32: worst error / arithmetic part of the bound = %.3f over %d payloads" % (worst, n))
    assert worst <= 0.5


# ------------------------------------------------------------------------------------------------------------
# 1. integer payloads: bit for bit under every configuration
# ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ly", LAYERS, ids=LAYER_IDS)
def test_conv_integers_bit_for_bit(ly):
    """Every configuration of the layer returns the fp64 reference's bits: a wrong row stride, source, upsampling shift, tap, slice
    or phase shows as a wrong integer, a read outside a view or between the weight records as NaN.  A deconv layer runs its four
    phases into one (B, 2H, 2W) view and is compared with F.conv_transpose2d."""
    c = _case(ly.payload, "int")
    want = bits(c.ref.to(F32 if ly.out_f32 else F16))
    outs = _run(ly, c)
    assert set(outs) == set(ly.ids)
    for cfg, got in outs.items():
        assert torch.equal(bits(got), want), "%s under 0x%02x" % (ly.name, cfg)


@gpu
def test_conv_single_phase_touches_only_its_pixels():
    """dst_scale = 2 with (dy, dx) = (1, 0): only the pixels (2i + 1, 2j) of the view change, and they hold the phase's 1x1 conv."""
    ly = next(l for l in LAYERS if l.name == "deconv-64-64")
    c = _case(ly.payload, "int")
    ref = c.ref.to(F16)
    want = torch.full_like(ref, POISON16)
    want[:, 1::2, 0::2] = ref[:, 1::2, 0::2]
    for cfg, got in _run(ly, c, ids=(0x10, 0x11, 0x63), refused=(), phases=((1, 0),)).items():
        assert torch.equal(bits(got), bits(want)), hex(cfg)


# ------------------------------------------------------------------------------------------------------------
# 2. random payloads with SiLU: fp64 under the derived bound; one layer, one answer
# ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ly", LAYERS, ids=LAYER_IDS)
def test_conv_random_within_derived_bound(ly):
    """|got - fp64| <= _bound under every configuration, and all configurations of the layer return identical bits.  A misaligned twin
    without a shortcut returns the aligned placement's bits (with one it rounds once instead of twice and stays within the bound)."""
    c = _case(ly.payload, "rand")
    arith, rnd = _bound(ly, c, lds_form(ly))
    outs = _run(ly, c)
    assert set(outs) == set(ly.ids)
    for cfg, got in outs.items():
        r = _worst(got, c.ref, arith + rnd)
        over = float((((got.to(F64) - c.ref).abs() - rnd) / arith).clamp(min=0).max()) if r <= 1.0 else math.inf
        print("conv16 %s 0x%02x [%s]: worst error / bound = %.3f, past the rounding part: %.3f of the arithmetic part" % (ly.name, cfg, family(ly, cfg), r, over))
        assert r <= 1.0, "%s under 0x%02x: %.3f of the bound" % (ly.name, cfg, r)
    first = outs[ly.ids[0]]
    for cfg, got in outs.items():
        assert torch.equal(bits(got), bits(first)), "%s: 0x%02x and 0x%02x differ" % (ly.name, cfg, ly.ids[0])
    if ly.place != "a":
        twin = replace(ly, place="a")
        aligned = _run(twin, c, ids=ly.ids[:1], refused=())[ly.ids[0]]
        assert _worst(aligned, c.ref, sum(_bound(twin, c, True))) <= 1.0
        if not ly.res:
            assert torch.equal(bits(first), bits(aligned))


# ------------------------------------------------------------------------------------------------------------
# 3. refusals through the plan interface
# ------------------------------------------------------------------------------------------------------------
REFUSALS = {
    "C0 of 12": Layer("", C0=12, C1=16, Cout=24),
    "slices of 48 channels": Layer("", C0=96, Cout=64, split=(2, 1)),
    "K walk 2 with 32-channel slices": Layer("", 3, 2, 128, Cout=64, B=3, H=14, W=10, split=(4, 1)),
    "ksize 3 with an upsampled source": Layer("", 3, 1, 32, up0=1, Cout=32),
    "odd map with an upsampled source": Layer("", C0=32, up0=1, Cout=32, H=13, W=14),
}


@gpu
@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(what):
    """launch_conv refuses the op with a BsyError before anything is launched: the whole destination still holds its poison."""
    ly = REFUSALS[what]
    t = _setup(ly, _inputs(ly.payload, "int"))
    with pytest.raises(L.BsyError):
        run_op(t.ops[0], t.ext, t.blob)
    torch.cuda.synchronize()
    assert_poison_intact(t.dst, t.g.cd, 0, t.poison)
