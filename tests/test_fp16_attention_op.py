"""The fp16 attention kernel (csrc/attention.hip) and its plan op ALONE, against fp64 under a bound derived from the kernel's arithmetic
(op_plan_helpers.attn16_bound) instead of a constant tolerance, on inputs built so that single keys decide the output:

  1. every (key_dim, head_dim) instantiation in the resident and the streaming form;
  2. a one-hot sweep: the whole softmax weight on one key, at the first and last key of a tile, of a streaming chunk, and the last real key;
  3. equal, strongly negative logits: a zero-padded key of the ragged tile (logit 0) in the maximum or the row sum would take everything;
  4. the resident capacity edge, N == attn_res_rows and one more;
  5. the query split over workgroups at head_dim 128 (4-wave workgroups) against the unsplit launch, bit for bit;
  6. BSY_OP_ATTN (prec 0) as a one-op plan on channel views of poisoned buffers, with and without pe, against the stand-alone call;
  7. what launch_attention refuses, on the host, before any launch.

All payloads are f16-valued and drawn from fixed seeds; every test prints its worst error / bound (docs/experiments.md lists them).

Run on the MI355X box with ``pytest -m gpu``.
"""
import ctypes as C
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

from op_plan_helpers import (DEV, NAN, POISON16, _worst, assert_poison_intact, attn16_bound, attn16_op, attn16_pe_blob, attn_pe_ref64,
                             attn_ref64, bits, poisoned, poisoned_image, run_op, view)
from test_attention_fused import _res_rows

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bs_yolo_amd import lib as L  # noqa: F401  (fails loudly when the .so is missing)
    from bs_yolo_amd import ops as O

F16 = torch.float16
RESIDENT, STREAMING = 1, 2
FORM = {0: "auto", RESIDENT: "resident", STREAMING: "streaming"}
# N -> the map (H, W) the keys are laid out on (what pe's taps walk; without pe only H * W counts)
HW = {70: (7, 10), 161: (7, 23), 33: (3, 11), 129: (3, 43), 417: (3, 139), 320: (16, 20), 321: (3, 107), 512: (16, 32), 513: (19, 27),
      35: (5, 7), 260: (13, 20), 37: (1, 37), 342: (18, 19)}  # (the last four: the maps of the plan-op cases)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _f16(t):
    return t.half().float()


TARGETS = (0, 1, 31, 32, 63, 64, 127, 128, 159, 160)  # first / last key of a tile, of a 128-key chunk, the last real key of N = 161


KINDS = ("randn", "peaky", "onehot", "uniform")


def _payload(kind, B, N, heads, kd, hd):
    """(B, N, heads * (2 kd + hd)) f16-valued floats in the op's [q | k | v] order.
      randn   all three standard normal
      peaky   q and k 8 times as wide: logits 64 times as wide, nearly one-hot rows, the running maximum moves by tens per tile
      onehot  u a fixed +-1 pattern; every query 6u, every key -6u but the target's, which is 6u: the target's logit leads by
              72 kd scale (>= 400 at kd^-0.5), its weight is 1 and every other 0 in any precision.  Image b aims head 0 at key
              TARGETS[b] and head 1 at TARGETS[B - 1 - b].
      uniform q = +4, k = -4 in every channel: all logits equal -16 kd scale (-90.5 at 32 / 64), the output is the mean of v"""
    g = _gen(KINDS.index(kind), B, N, heads, kd, hd)
    q, k, v = (torch.randn(B, N, heads, c, generator=g) for c in (kd, kd, hd))
    if kind == "peaky":
        q, k = q * 8, k * 8
    elif kind == "onehot":
        assert B == len(TARGETS) and heads == 2 and N > max(TARGETS)
        u = torch.tensor([1.0 if c % 3 else -1.0 for c in range(kd)])
        q, k = (6 * u).expand(B, N, heads, kd).clone(), (-6 * u).expand(B, N, heads, kd).clone()
        for b in range(B):
            k[b, TARGETS[b], 0], k[b, TARGETS[B - 1 - b], 1] = 6 * u, 6 * u
    elif kind == "uniform":
        q, k = torch.full_like(q, 4.0), torch.full_like(k, -4.0)
    return _f16(torch.cat((q.reshape(B, N, -1), k.reshape(B, N, -1), v.reshape(B, N, -1)), -1))


@lru_cache(maxsize=None)
def _case(kind, B, N, heads, kd, hd, scale=None):
    """Payload and fp64 reference, computed once per case and left unchanged."""
    scale = kd ** -0.5 if scale is None else scale
    qkv = _payload(kind, B, N, heads, kd, hd)
    return SimpleNamespace(qkv=qkv, heads=heads, kd=kd, hd=hd, scale=scale, ref=attn_ref64(qkv, heads, kd, hd, scale))


@lru_cache(maxsize=None)
def _pe(Cc):
    """Attention.pe's folded depthwise conv for Cc channels: f16-valued (w (Cc, 1, 3, 3), b (Cc))."""
    g = _gen(9, Cc)
    return _f16(torch.randn(Cc, 1, 3, 3, generator=g) * 0.3), _f16(torch.randn(Cc, generator=g))


@lru_cache(maxsize=None)
def _pe_ref(kind, B, N, heads, kd, hd):
    c = _case(kind, B, N, heads, kd, hd)
    return attn_pe_ref64(c.ref, *_pe(heads * hd), *HW[N])


def _launch(c, impl, pe=False, qkv=None):
    """ops.attention_pe_nhwc on the case's payload (or on `qkv`, a device tensor) -> the device output (B, H, W, heads * hd)."""
    if qkv is None:
        B, N, Cq = c.qkv.shape
        qkv = c.qkv.half().view(B, *HW[N], Cq).to(DEV)
    kw = dict(zip(("pe_w", "pe_b"), _pe(c.heads * c.hd))) if pe else {}
    out = O.attention_pe_nhwc(qkv, c.heads, c.kd, c.hd, c.scale, impl=impl, **kw)
    torch.cuda.synchronize()
    return out


def _ratio(got, c, what, pe=None):
    """worst |got - fp64| / bound over the case (inf: a non-finite output), printed."""
    want = c.ref.out if pe is None else pe.y
    r = _worst(got.detach().cpu().reshape(want.shape), want, attn16_bound(c.ref, pe))
    print("attn16 %s: worst error / bound = %.3f" % (what, r))
    return r


# ------------------------------------------------------------------------------------------------------------
# 1. every instantiation, both forms
# ------------------------------------------------------------------------------------------------------------
PAIRS = [(kd, hd) for kd in (16, 32, 48, 64) for hd in (32, 64, 96, 128)]
# N = 70: three key tiles, the last ragged, one streaming chunk.  N = 161: two chunks, a ragged sixth tile, and 6 query blocks for two
# 4-wave workgroups: the last two waves have no queries but must keep staging and the barriers.
FORMS = [(RESIDENT, 70), (STREAMING, 70), (STREAMING, 161)]


@pytest.mark.parametrize("impl,N", FORMS, ids=["%s-%d" % (FORM[i], n) for i, n in FORMS])
@pytest.mark.parametrize("kd,hd", PAIRS, ids=["%d/%d" % p for p in PAIRS])
def test_every_instantiation_matches_fp64(kd, hd, impl, N):
    assert N <= _res_rows(kd, hd)
    c = _case("randn", 2, N, 2, kd, hd)
    assert _ratio(_launch(c, impl), c, "1 %d/%d %s N %d randn" % (kd, hd, FORM[impl], N)) <= 1.0


@pytest.mark.parametrize("impl,N", [(RESIDENT, 70), (STREAMING, 161)], ids=["resident-70", "streaming-161"])
def test_peaky_logits_match_fp64(impl, N):
    c = _case("peaky", 2, N, 2, 32, 64)
    assert _ratio(_launch(c, impl), c, "1 32/64 %s N %d peaky" % (FORM[impl], N)) <= 1.0


@pytest.mark.parametrize("impl,N", [(RESIDENT, 70), (STREAMING, 161)], ids=["resident-70", "streaming-161"])
def test_scale_is_the_ops_field_not_rsqrt_key_dim(impl, N):
    """scale = 0.3 where key_dim^-0.5 is 0.177: a kernel that derived the scale from key_dim would be off by far more than the bound."""
    c = _case("randn", 2, N, 2, 32, 64, 0.3)
    assert _ratio(_launch(c, impl), c, "1 32/64 %s N %d scale 0.3" % (FORM[impl], N)) <= 1.0


# ------------------------------------------------------------------------------------------------------------
# 2. every key position counts
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kd,hd,impl", [(32, 64, RESIDENT), (32, 64, STREAMING), (64, 128, STREAMING)],
                         ids=["32/64-resident", "32/64-streaming", "64/128-streaming"])
def test_one_hot_sweep_returns_the_target_keys_v(kd, hd, impl):
    """One launch of ten images, each with the whole weight on another key: the output is that key's v row to within the bound (the
    P V term of which is 2^-11 |v_t|).  A key dropped, counted twice or paired with another key's V row -- a slip in the permuted
    accumulator-as-operand order, the transposing read or its swizzle -- returns another row of v, or 0, or twice the row."""
    c = _case("onehot", len(TARGETS), 161, 2, kd, hd)
    v = c.ref.v.view(len(TARGETS), 161, 2, hd)
    for b, t in enumerate(TARGETS):  # the reference itself is one-hot: out == v_t to fp64 resolution
        assert float((c.ref.out.view(len(TARGETS), 161, 2, hd)[b, :, 0] - v[b, t, 0]).abs().max()) < 1e-12
    assert _ratio(_launch(c, impl), c, "2 %d/%d %s one-hot" % (kd, hd, FORM[impl])) <= 1.0


# ------------------------------------------------------------------------------------------------------------
# 3. padded keys never count
# ------------------------------------------------------------------------------------------------------------
UNIFORM = [(32, 64, RESIDENT, 33), (32, 64, STREAMING, 33), (32, 64, RESIDENT, 129), (32, 64, STREAMING, 129), (32, 64, RESIDENT, 417),
           (32, 64, STREAMING, 417), (64, 128, 0, 321)]


@pytest.mark.parametrize("kd,hd,impl,N", UNIFORM, ids=["%d/%d-%s-%d" % (a, b, FORM[i], n) for a, b, i, n in UNIFORM])
def test_padded_keys_never_count(kd, hd, impl, N):
    """Every real logit is -16 kd scale (-90.5 / -128) and equal: the output is the plain mean of v.  The rows N .. 32 ceil(N / 32) - 1
    of the ragged tile are zeros, logit 0: one of them in the running maximum or in the row sum outweighs all real keys by e^90 and
    the output collapses to 0 -- far outside the bound, whose terms are all of the order of 2^-11 mean |v|."""
    if impl == 0:
        assert N > _res_rows(kd, hd)  # impl 0 streams here
    c = _case("uniform", 2, N, 2, kd, hd)
    assert float((c.ref.out - c.ref.v.mean(1, keepdim=True)).abs().max()) < 1e-12
    assert _ratio(_launch(c, impl), c, "3 %d/%d %s N %d uniform" % (kd, hd, FORM[impl], N)) <= 1.0


# ------------------------------------------------------------------------------------------------------------
# 4. resident capacity edge
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pe", [False, True], ids=["plain", "pe"])
@pytest.mark.parametrize("kd,hd,rows", [(32, 64, 512), (64, 128, 320)], ids=["32/64", "64/128"])
def test_resident_capacity_edge(kd, hd, rows, pe):
    """N == attn_res_rows: the LDS image is full to its last row, impl 0 and impl 1 are the same launch.  N == rows + 1: the resident
    form refuses, impl 0 streams.  With pe the resident epilogue reads v of the map's last row from the image's last rows."""
    assert _res_rows(kd, hd) == rows
    heads = 2 if hd == 64 else 1
    full, over = _case("randn", 1, rows, heads, kd, hd), _case("randn", 1, rows + 1, heads, kd, hd)
    p_full, p_over = (_pe_ref("randn", 1, n, heads, kd, hd) if pe else None for n in (rows, rows + 1))
    got0, got1 = _launch(full, 0, pe), _launch(full, RESIDENT, pe)
    assert torch.equal(bits(got0), bits(got1))
    assert _ratio(got1, full, "4 %d/%d N %d resident%s" % (kd, hd, rows, " + pe" * pe), p_full) <= 1.0
    with pytest.raises(RuntimeError):
        _launch(over, RESIDENT, pe)
    assert _ratio(_launch(over, 0, pe), over, "4 %d/%d N %d auto (streams)%s" % (kd, hd, rows + 1, " + pe" * pe), p_over) <= 1.0


# ------------------------------------------------------------------------------------------------------------
# 5. query split at head_dim 128
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pe", [False, True], ids=["plain", "pe"])
def test_query_split_at_head_dim_128_returns_the_unsplit_bits(pe):
    """64 / 128, N = 320: ten query blocks on 4-wave workgroups.  One image of one head alone is dealt to nsplit = min(256, ceil(10 / 4))
    = 3 workgroups, each staging the head again; as the first and the last of 256 images it has one workgroup (nsplit = 1)."""
    c = _case("randn", 1, 320, 1, 64, 128)
    x = c.qkv.half().view(1, 16, 20, -1).to(DEV)
    alone = _launch(c, RESIDENT, pe)
    many = _launch(c, RESIDENT, pe, qkv=x.expand(256, -1, -1, -1).contiguous())
    assert torch.equal(bits(many[:1]), bits(alone)) and torch.equal(bits(many[255:]), bits(alone))
    assert _ratio(alone, c, "5 64/128 N 320 split%s" % (" + pe" * pe), _pe_ref("randn", 1, 320, 1, 64, 128) if pe else None) <= 1.0


# ------------------------------------------------------------------------------------------------------------
# 6. the plan op alone on poisoned views
# ------------------------------------------------------------------------------------------------------------
# (kd, hd, heads, B, H, W, NaN channels beside the payload in a source row)
PLAN_CASES = [(32, 64, 2, 2, 5, 7, 24), (32, 64, 2, 2, 13, 20, 40), (16, 32, 1, 2, 1, 37, 32), (64, 128, 1, 2, 18, 19, 24)]
PLAN_VIEWS = [(8, 4), (16, 8)]  # (source channel offset, destination channel offset)


def _plan_setup(kd, hd, heads, B, H, W, extra, cs, cd, pe):
    """The ATTN op over views: the [q | k | v] payload in channels [cs, cs + C) of rows of C + extra f16, NaN in the other channels
    and -- poisoned_image -- in front of the first and behind the last row; the destination POISON16 outside [cd, cd + heads * hd) of
    rows of heads * hd + 12 + cd; the pe record in a blob with NaN behind its matrix and its bias.
    -> (op, external tensors [source, destination], blob, what keeps the source allocation alive)."""
    Cq, Co = heads * (2 * kd + hd), heads * hd
    ld, ldo = Cq + extra, Co + 12 + cd
    rows = torch.full((B, H, W, ld), NAN)
    rows[..., cs:cs + Cq] = _payload("randn", B, H * W, heads, kd, hd).view(B, H, W, Cq)
    flat, src = poisoned_image(rows, F16)
    dst = poisoned((B, H, W, ldo), cd, Co, None, POISON16, dtype=F16)
    blob, offs = attn16_pe_blob(*_pe(Co)) if pe else (b"", None)
    op = attn16_op(B, H, W, view(0, ld, cs, Cq), view(1, ldo, cd, Co), heads, kd, hd, kd ** -0.5, offs)
    return op, [src, dst], blob, flat


@pytest.mark.parametrize("pe", [False, True], ids=["act0", "act1-pe"])
@pytest.mark.parametrize("cs,cd", PLAN_VIEWS, ids=["src8-dst4", "src16-dst8"])
@pytest.mark.parametrize("kd,hd,heads,B,H,W,extra", PLAN_CASES, ids=["32/64-5x7", "32/64-13x20", "16/32-1x37", "64/128-18x19"])
def test_plan_op_on_poisoned_views(kd, hd, heads, B, H, W, extra, cs, cd, pe):
    """BSY_OP_ATTN alone through bsy_plan_run: build_attn resolves both views with their channel offsets and takes pe from blob
    offsets.  A read beside the payload, before the first or behind the last row, or behind a pe record is a NaN in the output; a
    store outside the destination view breaks the poison.  18 x 19 = 342 keys of 64 / 128 do not fit: the plan's impl 0 streams."""
    if (H, W) == (18, 19):
        assert H * W > _res_rows(kd, hd)
    N, Cq, Co = H * W, heads * (2 * kd + hd), heads * hd
    assert HW[N] == (H, W)
    c = _case("randn", B, N, heads, kd, hd)
    op, (src, dst), blob, keep = _plan_setup(kd, hd, heads, B, H, W, extra, cs, cd, pe)
    assert torch.equal(bits(src[..., cs:cs + Cq]), bits(c.qkv.half().view(B, H, W, Cq)))
    run_op(op, [src, dst], blob)
    assert_poison_intact(dst, cd, Co, POISON16)
    got = dst[..., cd:cd + Co]
    assert torch.equal(bits(got), bits(_launch(c, 0, pe, qkv=src[..., cs:cs + Cq].contiguous()))), "plan op != stand-alone call"
    what = "6 %d/%d heads %d map %dx%d views %d/%d%s" % (kd, hd, heads, H, W, cs, cd, " + pe" * pe)
    assert _ratio(got, c, what, _pe_ref("randn", B, N, heads, kd, hd) if pe else None) <= 1.0


# ------------------------------------------------------------------------------------------------------------
# 7. refusals (host-side, before any launch)
# ------------------------------------------------------------------------------------------------------------
def _src_off4(op): op.src0.coff = 4          # 8 bytes past a 16-byte boundary: the kernel's 16-byte loads
def _dst_off2(op): op.dst.coff = 2           # 4 bytes past an 8-byte boundary: its 8-byte stores
def _ld_odd(op): op.src0.ld -= 4             # 276: still >= the 256-channel row, no multiple of 8
def _ldo_odd(op): op.dst.ld -= 2             # 142: still >= 128, no multiple of 4
def _ld_small(op): op.src0.ld = 248          # a multiple of 8 below heads * (2 kd + hd) = 256
def _ldo_small(op): op.dst.ld = 124          # a multiple of 4 below heads * hd = 128
def _kd24(op): op.key_dim = 24
def _hd48(op): op.head_dim = 48


REFUSED_OPS = [_src_off4, _dst_off2, _ld_odd, _ldo_odd, _ld_small, _ldo_small, _kd24, _hd48]


@pytest.mark.parametrize("pe", [False, True], ids=["act0", "act1-pe"])
@pytest.mark.parametrize("spoil", REFUSED_OPS, ids=[f.__name__[1:] for f in REFUSED_OPS])
def test_plan_op_refusals(spoil, pe):
    """One field of a good op (the 5 x 7 case of group 6) made wrong; the tensors keep their sizes, and every spoiled stride or width
    is smaller than the true one.  launch_attention refuses on the host: RuntimeError, the whole destination still poison."""
    op, ext, blob, keep = _plan_setup(32, 64, 2, 2, 5, 7, 24, 8, 4, pe)
    spoil(op)
    with pytest.raises(RuntimeError):
        run_op(op, ext, blob)
    assert_poison_intact(ext[1], 4, 0, POISON16)


def _c_entry(qkv, H, W, wp, bp, out, impl=0, w_ptr=None):
    """bsy_attention_pe itself on 32 / 64, two heads: the tensors' own strides, H and W as given, the pe matrix at `w_ptr`."""
    B, ld, ldo = qkv.shape[0], qkv.shape[-1], out.shape[-1]
    w_ptr = wp.data_ptr() if w_ptr is None else w_ptr
    L.check(L.lib.bsy_attention_pe(C.c_void_p(qkv.data_ptr()), ld, B, H, W, 2, 32, 64, 32 ** -0.5, C.c_void_p(w_ptr), C.c_void_p(bp.data_ptr()),
                                   C.c_void_p(out.data_ptr()), ldo, impl, L.stream_ptr(qkv.device)))
    torch.cuda.synchronize()


def _c_entry_setup():
    c = _case("randn", 2, 70, 2, 32, 64)
    qkv = c.qkv.half().view(2, 7, 10, -1).to(DEV)
    wp, bp = O.pack_dw_weight(*_pe(128), DEV)
    out = torch.full((2, 7, 10, 128), POISON16, dtype=F16, device=DEV)
    return qkv, wp, bp, out


def test_impl_3_is_refused():
    qkv, wp, bp, out = _c_entry_setup()
    for pe in ({}, dict(pe_w=O.Packed(wp, bp, (128, 1, 3, 3)))):
        with pytest.raises(RuntimeError):
            O.attention_pe_nhwc(qkv, 2, 32, 64, 32 ** -0.5, impl=3, out=out, **pe)
    torch.cuda.synchronize()
    assert_poison_intact(out, 0, 0, POISON16)


@pytest.mark.parametrize("H,W", [(70, 0), (0, 70), (7, -10), (65536, 65536)])
def test_pe_on_a_map_that_is_not_n_keys_is_refused(H, W):
    """launch_attention refuses pe unless H * W == N.  Both callers -- bsy_attention_pe and build_attn -- derive N from H and W, so
    through the C entry the mismatch can only be a map that has no N at all: an empty or negative side, or a product past an int.
    bsy_attention_pe answers those itself ("bad map size") before launch_attention sees them; the tensors hold 7 x 10 keys."""
    qkv, wp, bp, out = _c_entry_setup()
    with pytest.raises(RuntimeError):
        _c_entry(qkv, H, W, wp, bp, out)
    assert_poison_intact(out, 0, 0, POISON16)


def test_pe_weights_off_a_16_byte_boundary_are_refused():
    """The pe matrix 4 bytes into its allocation (the kernel reads it with 16-byte loads); the same call with the pointer where it
    belongs runs -- the refusal is about the pointer."""
    qkv, wp, bp, out = _c_entry_setup()
    wide = torch.cat((wp.reshape(-1), wp.new_zeros(4)))  # the shifted matrix still lies inside an allocation of ours
    with pytest.raises(RuntimeError):
        _c_entry(qkv, 7, 10, wide, bp, out, w_ptr=wide.data_ptr() + 4)
    with pytest.raises(RuntimeError):
        _c_entry(qkv, 7, 10, wp, torch.cat((bp, bp.new_zeros(4)))[1:], out)
    assert_poison_intact(out, 0, 0, POISON16)
    _c_entry(qkv, 7, 10, wp, bp, out)
    assert bool(torch.isfinite(out).all()) and not bool((out == POISON16).all())
