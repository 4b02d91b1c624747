"""Shared pieces of the one-op plan tests (test_glue_ops.py, test_bsyolo_ops.py, test_fp32_matrix_ops.py, test_fp16_conv_ops.py, test_fp16_head_ops.py,
test_fp16_block_ops.py, test_fp16_attention_op.py): a single bsy_op run through bsy_plan_create / bsy_plan_run with every tensor bound as an external slot, poisoned
views and a weight-blob builder.  Not a test module."""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

DEV = "cuda:0"
NAN = float("nan")
POISON16, POISON32 = 777.0, 7.77e7  # destination poison: exact in f16 / f32, far outside every payload the tests draw


def view(slot, ld, coff, C_):
    """Channels [coff, coff + C_) of external slot `slot`, rows of `ld` elements."""
    from bs_yolo_amd import lib as L
    return L.View(L.BSY_EXT_BASE + slot, ld, coff, C_)


def no_view():
    from bs_yolo_amd import lib as L
    return L.View(*L.NO_VIEW)


def new_op(kind, prec, B, H, W):
    """A bsy_op of `kind` with every view absent; OH / OW default to H / W."""
    from bs_yolo_amd import lib as L
    op = L.Op()
    op.kind, op.prec = kind, prec
    op.B, op.H, op.W, op.OH, op.OW = B, H, W, H, W
    op.src0, op.src1, op.dst, op.res = no_view(), no_view(), no_view(), no_view()
    for i in range(L.BSY_MAX_LEVELS):
        op.box[i], op.cls[i], op.msk[i] = no_view(), no_view(), no_view()
    return op


def run_op(op, ext_tensors, blob=b""):
    """One-op plan: engine + weights (`blob`, padded to 256 bytes: bsy_plan_create refuses an engine without weights), plan, run on
    the current stream, synchronise; plan and engine are destroyed whatever happens.  None in ext_tensors = a null slot."""
    run_ops([op], ext_tensors, blob)


def run_ops(ops, ext_tensors, blob=b""):
    """run_op for a chain of ops in ONE plan, launched in their order on the current stream."""
    from bs_yolo_amd import lib as L
    blob = bytes(blob) + b"\0" * max(0, 256 - len(blob))
    eng, plan = C.c_void_p(), C.c_void_p()
    L.check(L.lib.bsy_engine_create(0, C.byref(eng)))
    try:
        L.check(L.lib.bsy_engine_load_weights(eng, (C.c_char * len(blob)).from_buffer_copy(blob), len(blob)))
        L.check(L.lib.bsy_plan_create(eng, (L.Op * len(ops))(*ops), len(ops), None, 0, C.byref(plan)))
        n = len(ext_tensors)
        ext = (C.c_void_p * max(n, 1))(*[None if t is None else t.data_ptr() for t in ext_tensors])
        L.check(L.lib.bsy_plan_run(plan, ext, n, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    finally:
        if plan:
            L.lib.bsy_plan_destroy(plan)
        L.lib.bsy_engine_destroy(eng)


def poisoned(shape_with_ld, coff, C_, payload, poison, dtype=None):
    """Device tensor of `shape_with_ld` (last axis = the row stride ld) and payload's dtype: `payload` (shape[:-1] + (C_,); None = a
    destination, `dtype` says which) in channels [coff, coff + C_), `poison` everywhere else -- under a None payload too."""
    dtype = payload.dtype if payload is not None else dtype
    t = torch.full(tuple(shape_with_ld), poison, dtype=dtype)
    if payload is not None:
        assert tuple(payload.shape) == tuple(shape_with_ld[:-1]) + (C_,) and coff + C_ <= shape_with_ld[-1]
        t[..., coff:coff + C_] = payload
    return t.to(DEV)


def bits(t):
    """The tensor's bit pattern (NaN-safe, sign-of-zero-exact comparisons)."""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def assert_poison_intact(t, coff, C_, poison):
    """Everything of the device tensor `t` outside channels [coff, coff + C_) still holds `poison`, bit for bit."""
    h = t.detach().cpu()
    want = bits(torch.full((1,), poison, dtype=h.dtype)).item()
    b = bits(h)
    assert bool((b[..., :coff] == want).all()) and bool((b[..., coff + C_:] == want).all()), "a store left the destination view"


def weights_blob(arrays):
    """Arrays laid out at 256-byte offsets -> (bytes, [offset of each])."""
    blob, offs = b"", []
    for a in arrays:
        blob += b"\0" * (-len(blob) % 256)
        offs.append(len(blob))
        blob += np.ascontiguousarray(a).tobytes()
    return blob, offs


_NAN_PAD = np.full(128, np.nan, np.float32).tobytes()  # 512 bytes; an f32 NaN read as two f16 is (0, NaN)


def poisoned_blob(arrays):
    """weights_blob with NaN instead of zeros between the records: every record is followed by 256 to 511 bytes of NaN, so a read
    past a record's end -- or in front of the next one -- reaches the output.  -> (bytes, [offset of each])."""
    blob, offs = b"", []
    for a in arrays:
        offs.append(len(blob))
        blob += np.ascontiguousarray(a).tobytes()
        blob += _NAN_PAD[:4 * ((-len(blob) % 256) // 4 + 64)]
        assert len(blob) % 256 == 0, "records are whole 4-byte words"
    return blob, offs


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def dw_ref(x, w9, bias, act, res, kh=3, kw=3, stride=1, act_c=None):
    """fp64 depthwise conv of x (B, H, W, C); w9 (kh * kw, C) tap-major as the kernels read it; SiLU on the first act_c channels."""
    Cc = x.shape[-1]
    w = w9.double().t().reshape(Cc, 1, kh, kw)
    y = F.conv2d(nchw(x.double()), w, bias.double(), stride, (kh // 2, kw // 2), 1, Cc)
    n = Cc if act_c is None else act_c
    if act and n:
        y = torch.cat((F.silu(y[:, :n]), y[:, n:]), 1)
    y = nhwc(y)
    return y + res.double() if res is not None else y


def dwg_record(wk, bias, wld, koff):
    """A DWCONV_G weight record whose rows are longer than the launch: wk (taps, C) in columns [koff, koff + C) of a NaN (taps, wld)
    matrix, bias (C,) behind koff NaNs.  -> (matrix, bias vector) as float32 arrays for a blob."""
    taps, Cc = wk.shape
    assert koff + Cc <= wld
    w, b = torch.full((taps, wld), NAN), torch.full((koff + Cc,), NAN)
    w[:, koff:koff + Cc], b[koff:] = wk, bias
    return w.numpy(), b.numpy()


def dwg_op(prec, B, H, W, kh, kw, stride, src, dst, w_off, b_off, wld, koff, act_c, mid_c=0):
    """A DWCONV_G op, fields as run_op reads them: ksize = kh, pad = kw, heads = weight row length, key_dim = channel offset into the
    rows and the bias, act = leading SiLU channels, mid_c = first channel of an identity-kernel half (0 = none)."""
    from bs_yolo_amd import lib as L
    op = new_op(L.OP_DWCONV_G, prec, B, H, W)
    op.OH, op.OW = (H + 2 * (kh // 2) - kh) // stride + 1, (W + 2 * (kw // 2) - kw) // stride + 1
    op.ksize, op.pad, op.stride, op.heads, op.key_dim, op.act, op.mid_c = kh, kw, stride, wld, koff, int(act_c), int(mid_c)
    op.src0, op.dst, op.w_off, op.b_off = src, dst, w_off, b_off
    return op


def conv1x1_op(B, H, W, src, dst, w_off, b_off, act=True, res=None):
    """A fp16 1x1 CONV op (weights packed by ops.pack_conv_weight) as Plan.conv emits it: one source, SiLU, an optional shortcut."""
    from bs_yolo_amd import lib as L
    op = new_op(L.OP_CONV, 0, B, H, W)
    op.ksize, op.stride, op.pad, op.act, op.dst_scale = 1, 1, 0, int(act), 1
    op.src0, op.dst, op.w_off, op.b_off = src, dst, w_off, b_off
    if res is not None:
        op.res = res
    return op


def packed_1x1(w, b):
    """Dense (cout, cin) f16-valued weights + f32 bias -> the packed [CoutPad][Kpad] f16 matrix and [CoutPad] f32 bias, as host arrays."""
    from bs_yolo_amd import ops as O
    wp, bp = O.pack_conv_weight(w[:, :, None, None], b, "cpu")
    return wp.numpy(), bp.numpy()


def conv32_record(w, b, prec):
    """One dense conv's record for the fp32-storage modes, laid out as weights.pack_record does for f32 / split: the f32
    [k*k*cin][cout] matrix of w (cout, cin, k, k) and, for prec == 2, the hi / lo f16 planes of weights.split_f16_planes at the
    256-byte offsets run_op_f32 computes behind it.  The gaps between the three parts hold f32 NaN (read as f16: 0, NaN); the planes'
    own padding up to Kpad stays zero, the kernels multiply it.  -> (weight record as a uint8 array, bias as a float32 array)."""
    from bs_yolo_amd import weights as Wt
    cout, cin, k, _ = w.shape
    K = k * k * cin
    rec = w.float().permute(2, 3, 1, 0).reshape(K, cout).contiguous().numpy().tobytes()
    if prec == 2:
        hi, lo = Wt.split_f16_planes(w.float().permute(0, 2, 3, 1).reshape(cout, K))
        assert hi.shape == (cout, (K + 31) // 32 * 32)
        for plane in (hi, lo):
            rec += _NAN_PAD[:-len(rec) % 256] + plane.numpy().tobytes()
            assert len(rec) % 4 == 0
    return np.frombuffer(rec, np.uint8), b.float().contiguous().numpy()


def conv32_op(prec, B, H, W, ksize, stride, pad, src0, dst, w_off, b_off, src1=None, up0=0, up1=0, res=None, act=0, dst_scale=1, dst_dy=0,
              dst_dx=0, in_dtype=None, first=False):
    """A CONV (first: CONV_FIRST, src0 = the BCHW image of `in_dtype`) op of the fp32-storage modes, fields as run_op_f32 reads them.
    H, W: the conv's input map (a source read through nearest x2 holds H / 2 x W / 2); the destination holds OH * dst_scale rows."""
    from bs_yolo_amd import lib as L
    op = new_op(L.OP_CONV_FIRST if first else L.OP_CONV, prec, B, H, W)
    op.OH, op.OW = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    op.ksize, op.stride, op.pad, op.act = ksize, stride, pad, int(act)
    op.src0, op.dst, op.up0, op.up1 = src0, dst, up0, up1
    if src1 is not None:
        op.src1 = src1
    if res is not None:
        op.res = res
    op.dst_scale, op.dst_dy, op.dst_dx = dst_scale, dst_dy, dst_dx
    op.in_dtype = L.BSY_F32 if in_dtype is None else in_dtype
    op.w_off, op.b_off = w_off, b_off
    return op


def attn32_op(prec, B, H, W, src, dst, heads, key_dim, head_dim, scale):
    """An ATTN op of the fp32-storage modes: src = the [q | k | v] map (heads * (2 key_dim + head_dim) channels), N = H * W."""
    from bs_yolo_amd import lib as L
    op = new_op(L.OP_ATTN, prec, B, H, W)
    op.src0, op.dst = src, dst
    op.heads, op.key_dim, op.head_dim, op.scale = heads, key_dim, head_dim, float(scale)
    return op


def attn16_op(B, H, W, src, dst, heads, kd, hd, scale, pe=None):
    """A fp16 (prec 0) ATTN op, fields as build_attn reads them (csrc/op_args.h): src = the [q | k | v] view, N = H * W;
    pe = (w_off, b_off): act = 1 and the blob offsets of Attention.pe's depthwise record (attn16_pe_blob), folded into the epilogue."""
    from bs_yolo_amd import lib as L
    op = new_op(L.OP_ATTN, 0, B, H, W)
    op.src0, op.dst = src, dst
    op.heads, op.key_dim, op.head_dim, op.scale = heads, kd, hd, float(scale)
    if pe is not None:
        op.act, op.w_off, op.b_off = 1, pe[0], pe[1]
    return op


def attn16_pe_blob(w, b):
    """Attention.pe's record for attn16_op in a poisoned blob: ops.pack_dw_weight's f32 [9][heads * hd] matrix of w (heads * hd, 1, 3, 3)
    and the f32 bias, NaN behind each.  -> (bytes, (w_off, b_off))."""
    from bs_yolo_amd import ops as O
    wp, bp = O.pack_dw_weight(w, b, "cpu")
    blob, offs = poisoned_blob([wp.numpy(), bp.numpy()])
    return blob, (offs[0], offs[1])


def attn_ref64(qkv, heads, kd, hd, scale):
    """Softmax attention in fp64 on the fp16 ATTN op's layout, with what attn16_bound needs.  qkv (B, ..., heads * (2 kd + hd)) in
    [q (all heads) | k (all heads) | v (all heads)] order, the axes between the first and the last flattened to N.  ->
      out   (B, N, heads * hd)  sum_j p_j v_jd / sum_j p_j,  p_j = exp(s_j - max s),  s_j = scale * q . k_j
      A     (B, N, heads * hd)  sum_j p_j |v_jd| / sum_j p_j
      Smax  (B, N, heads)       scale * max_j sum_c |q_c| |k_jc|
      l     (B, N, heads)       sum_j p_j  (>= 1: the maximal key has p = 1)
      vmax  (B, heads * hd)     max_j |v_jd|
      v     (B, N, heads * hd)  the v channels (for pe), and N, heads, kd, hd."""
    from types import SimpleNamespace
    B, C_ = qkv.shape[0], qkv.shape[-1]
    assert C_ == heads * (2 * kd + hd)
    x = qkv.detach().cpu().double().reshape(B, -1, C_)
    N = x.shape[1]
    q = x[..., :heads * kd].view(B, N, heads, kd).permute(0, 2, 1, 3)
    k = x[..., heads * kd:2 * heads * kd].view(B, N, heads, kd).permute(0, 2, 1, 3)
    v = x[..., 2 * heads * kd:].view(B, N, heads, hd).permute(0, 2, 1, 3)
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    l = p.sum(-1, keepdim=True)
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, -1)
    return SimpleNamespace(out=flat(p @ v / l), A=flat(p @ v.abs() / l), l=flat(l),
                           Smax=flat((q.abs() @ k.abs().transpose(-1, -2)).max(-1, keepdim=True).values * scale),
                           vmax=x[..., 2 * heads * kd:].abs().max(1).values, v=x[..., 2 * heads * kd:].contiguous(),
                           N=N, heads=heads, kd=kd, hd=hd)


def attn_pe_ref64(r, w, b, H, W):
    """Attention.pe on top of attn_ref64's `r`: w (heads * hd, 1, 3, 3), b (heads * hd), the N keys an H x W map.  ->
      y    (B, N, heads * hd)  r.out + depthwise3x3(v) + bias, in fp64
      mag  (B, N, heads * hd)  |bias| + sum_taps |w| |v|, the magnitude the depthwise arithmetic's error scales with."""
    from types import SimpleNamespace
    B, Cc = r.v.shape[0], r.v.shape[-1]
    assert H * W == r.N and tuple(w.shape) == (Cc, 1, 3, 3)
    w9 = w.double().reshape(Cc, 9).t()
    v = r.v.view(B, H, W, Cc)
    dw = dw_ref(v, w9, b, False, None).reshape(B, r.N, Cc)
    mag = dw_ref(v.abs(), w9.abs(), b.abs(), False, None).reshape(B, r.N, Cc)
    return SimpleNamespace(y=r.out + dw, mag=mag)


def attn16_bound(r, pe=None):
    """Allowed |got - fp64| per output element of the fp16 attention kernel (csrc/attention.hip), from attn_ref64's `r`: derived from
    the kernel's arithmetic -- 32-key tiles, f32 online softmax, P rounded to f16 for the PV product, the row sum of the unrounded
    P -- not fitted to its output.  u = 2^-24, nt = ceil(N / 32); the sum of
      2^-11 A                                          P rounded to f16 for the PV product while the row sum keeps the f32 P
      N 2^-25 vmax / max(l, 1)                         the f16 subnormal floor of P (subnormals are not flushed in the default mode)
      2 ((kd + 8) u Smax 1.4427 * 1.45 + 4u) A         the f32 error of the exponent's argument and of v_exp_f32, in the numerator
                                                       and in the denominator
      1.1 (N + 2 nt + 8) u A                           the f32 sums of O and l, and the alpha rescales
      0.5 ulp16(out) + 2u |out|                        o * inv rounded to f32, then to f16
    and, with pe = attn_pe_ref64(...) (the value compared is then pe.y = out + dw):
      0.5 ulp16(out)                                   the attention output rounded to f16 before the depthwise sum is added
      12u (|bias| + sum_taps |w| |v|)                  the depthwise arithmetic: a bias and nine f32 fmas
      0.5 ulp16(y) + u |y|                             the final f32 sum and its rounding to f16"""
    nt = (r.N + 31) // 32
    A, out = r.A, r.out
    Smax = r.Smax.repeat_interleave(r.hd, -1)
    l = r.l.repeat_interleave(r.hd, -1)
    b = 2.0 ** -11 * A
    b = b + r.N * 2.0 ** -25 * r.vmax[:, None, :] / l.clamp(min=1.0)
    b = b + 2 * ((r.kd + 8) * U * Smax * 1.4427 * 1.45 + 4 * U) * A
    b = b + 1.1 * (r.N + 2 * nt + 8) * U * A
    b = b + 0.5 * _u16(out) + 2 * U * out.abs()
    if pe is not None:
        b = b + 0.5 * _u16(out) + 12 * U * pe.mag + 0.5 * _u16(pe.y) + U * pe.y.abs()
    return b


def assert_outside_views_intact(t, before, views):
    """Everything of the device tensor `t` outside the channel ranges `views` = [(coff, C), ...] has the bits of `before` (its host
    copy from before the run)."""
    keep = torch.ones(t.shape[-1], dtype=torch.bool)
    for coff, C_ in views:
        keep[coff:coff + C_] = False
    assert torch.equal(bits(t)[..., keep], bits(before)[..., keep]), "a store left the destination view"


def ulp(v, mant, floor_exp):
    """Unit in the last place of |v| (float64 array) in a format of `mant` stored mantissa bits, floored at 2^floor_exp (the subnormal spacing)."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(a)
    return np.where(a == 0, 2.0 ** floor_exp, np.maximum(np.ldexp(1.0, e - 1 - mant), 2.0 ** floor_exp))


def ulp16(v):
    return ulp(v, 10, -24)


def ulp32(v):
    return ulp(v, 23, -149)


# ---- the fp16 CONV op (tests/test_fp16_conv_ops.py) ----
def conv16_op(B, H, W, ksize, stride, pad, src0, dst, w_off, b_off, src1=None, up0=0, up1=0, res=None, act=0, out_f32=0, dst_scale=1,
              dst_dy=0, dst_dx=0, nsl_c=0, nsl_t=0, slab=None):
    """A fp16 CONV op, fields as build_conv reads them (csrc/op_args.h).  H, W: the conv's input map (a source read
    through nearest x2 holds H / 2 x W / 2); the destination holds OH * dst_scale rows.  Split-K: ksplit = nsl_c | nsl_t << 8 and
    box[0] = `slab`, the view of the f32 slab buffer."""
    from bs_yolo_amd import lib as L
    op = new_op(L.OP_CONV, 0, B, H, W)
    op.OH, op.OW = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    op.ksize, op.stride, op.pad, op.act, op.out_f32 = ksize, stride, pad, int(act), int(out_f32)
    op.src0, op.dst, op.up0, op.up1 = src0, dst, up0, up1
    if src1 is not None:
        op.src1 = src1
    if res is not None:
        op.res = res
    op.dst_scale, op.dst_dy, op.dst_dx = dst_scale, dst_dy, dst_dx
    if nsl_c * nsl_t > 1:
        op.ksplit = nsl_c | nsl_t << 8
        op.box[0] = slab
    op.w_off, op.b_off = w_off, b_off
    return op


PHASES = ((0, 0), (0, 1), (1, 0), (1, 1))


def conv16_blob(w, b, deconv=False, phases=PHASES):
    """The packed records of one fp16 conv (k = 1 or 3) in a poisoned blob: ops.pack_conv_weight's [CoutPad][Kpad] f16 matrix and
    [CoutPad] f32 bias, NaN between the records.  deconv: w is a ConvTranspose2d(cin, cout, 2, 2) weight (cin, cout, 2, 2) and every
    phase (dy, dx) of `phases` gets a 1x1 record of its own, W[:, :, dy, dx]^T, as plan.py's WRec kind "deconv" and
    weights.pack_record cut it.  -> (bytes, [(w_off, b_off, dy, dx), ...])."""
    from bs_yolo_amd import ops as O
    assert w.shape[-1] in ((2,) if deconv else (1, 3))
    parts = [(dy, dx, w[:, :, dy, dx].t().contiguous()[:, :, None, None]) for dy, dx in phases] if deconv else [(0, 0, w)]
    arrays = []
    for _, _, wk in parts:
        wp, bp = O.pack_conv_weight(wk, b, "cpu")
        arrays += [wp.numpy(), bp.numpy()]
    blob, offs = poisoned_blob(arrays)
    return blob, [(offs[2 * i], offs[2 * i + 1], dy, dx) for i, (dy, dx, _) in enumerate(parts)]


def run_conv_cfgs(ops, ext_tensors, blob, cfgs, refused, reset, collect):
    """ONE plan of `ops` (all CONV) kept alive over a list of kernel configuration ids.  For every id: reset() (re-poison the
    destination), bsy_plan_set_tuning with the id on every op, bsy_plan_check_tuning -- which must answer 1 on every op for an id of
    `cfgs` and 0 for an id of `refused`: a preset that is not valid is ignored at launch, and the case would test the heuristic
    configuration under another name -- then, for an id of `cfgs`, run on the current stream, synchronise and keep collect()'s value.
    An entry of `cfgs` may be a tuple with one id per op instead (ops of different kernel families in one plan).
    -> {entry: collect()}.  The plan and the engine are destroyed whatever happens."""
    from bs_yolo_amd import lib as L
    blob = bytes(blob) + b"\0" * max(0, 256 - len(blob))
    n, out = len(ops), {}
    eng, plan = C.c_void_p(), C.c_void_p()
    L.check(L.lib.bsy_engine_create(0, C.byref(eng)))
    try:
        L.check(L.lib.bsy_engine_load_weights(eng, (C.c_char * len(blob)).from_buffer_copy(blob), len(blob)))
        L.check(L.lib.bsy_plan_create(eng, (L.Op * n)(*ops), n, None, 0, C.byref(plan)))
        n_ext = len(ext_tensors)
        ext = (C.c_void_p * max(n_ext, 1))(*[None if t is None else t.data_ptr() for t in ext_tensors])
        for cfg, want in [(c, 1) for c in cfgs] + [(c, 0) for c in refused]:
            reset()
            per_op = list(cfg) if isinstance(cfg, tuple) else [cfg] * n
            assert len(per_op) == n
            L.check(L.lib.bsy_plan_set_tuning(plan, (C.c_int32 * n)(*per_op), n))
            valid = (C.c_int32 * n)()
            L.check(L.lib.bsy_plan_check_tuning(plan, ext, n_ext, valid, n))
            assert list(valid) == [want] * n, "configuration %s: bsy_plan_check_tuning says %s, the case expects %d" % (
                "/".join("0x%02x" % c for c in dict.fromkeys(per_op)), list(valid), want)
            if want:
                L.check(L.lib.bsy_plan_run(plan, ext, n_ext, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                torch.cuda.synchronize()
                out[cfg] = collect()
    finally:
        if plan:
            L.lib.bsy_plan_destroy(plan)
        L.lib.bsy_engine_destroy(eng)
    return out


# ---- the fused Detect head ops (tests/test_fp16_head_ops.py) ----
def conv16_records(convs):
    """The packed records of several fp16 convs [(w, b), ...] in ONE poisoned blob, every matrix and every bias vector a record of its
    own with NaN behind it.  -> (bytes, [(w_off, b_off), ...])."""
    from bs_yolo_amd import ops as O
    arrays = []
    for w, b in convs:
        wp, bp = O.pack_conv_weight(w, b, "cpu")
        arrays += [wp.numpy(), bp.numpy()]
    blob, offs = poisoned_blob(arrays)
    return blob, [(offs[2 * i], offs[2 * i + 1]) for i in range(len(convs))]


def head16_op(B, H, W, ksize, src0, y, w_off, b_off, mode, cout, A, a0, stride, out_dtype, raw=None, act=0, tail=None, res=None):
    """A fp16 CONV op with the Detect decoder in its epilogue, fields as Plan._decoding_conv emits them and run_op's BSY_OP_CONV case
    reads them: out_f32 = `mode` (2: class scores, 3: DFL boxes), dst = `y`, the (B, y.C, A) prediction tensor of `out_dtype` whose
    anchors [a0, a0 + H * W) belong to this level, nl = the conv's couts, lvl_stride[0] = the level's stride, box[0] = `raw`, the level's
    (B, raw.C, H, W) raw map of the same dtype (None: no raw map).  tail = (w2_off, b2_off): the box-branch tail -- this op is the 3x3
    conv (64 couts, `act`) and the record named is the branch's 64 -> 64 1x1 conv."""
    op = conv16_op(B, H, W, ksize, 1, ksize // 2, src0, y, w_off, b_off, res=res, act=act, out_f32=mode)
    op.nl, op.A, op.out_dtype = cout, A, out_dtype
    op.lvl_h[0], op.lvl_h[1], op.lvl_w[0], op.lvl_stride[0] = H, a0, W, float(stride)
    if raw is not None:
        op.box[0] = raw
    if tail is not None:
        op.mid_c, op.w2_off, op.b2_off = 64, tail[0], tail[1]
    return op


# ---- the derived bound of the fp16 conv ops (tests/test_fp16_conv_ops.py, tests/test_fp16_block_ops.py) ----
U = 2.0 ** -24  # unit roundoff of f32


def _u16(t):
    return torch.from_numpy(ulp16(t.numpy()))


def _bound(ly, c, two_roundings):
    """Allowed |got - fp64| per output element -> (arithmetic part, rounding part):

      arithmetic:  1.1 (K + nsl) 2^-24 S  +  8 * 2^-24 |a|  (SiLU)
                   the order-independent bound of a length-K fp32 sum that starts at the bias, one more add per split-K slice
                   (gamma_n <= 1.1 n u here), carried through SiLU, whose slope lies in (-0.1, 1.1); x / (1 + expf(-x)).
      rounding:    half an f16 ulp of y (subnormal floor included; out_f32: 2^-24 |y|), plus half an f16 ulp of a where the form rounds
                   before it adds the shortcut -- half(half(act(v)) + r): conv_epilogue_lds and the patch kernel; conv_epilogue and
                   splitk_reduce_kernel add in f32 and round once."""
    arith = 1.1 * (ly.K + ly.nsl) * U * c.S
    if c.act:
        arith = arith + 8 * U * c.a.abs()
    rnd = U * c.ref.abs() if ly.out_f32 else 0.5 * _u16(c.ref)
    if two_roundings and c.res is not None:
        rnd = rnd + 0.5 * _u16(c.a)
    return arith, rnd


def _worst(got, ref, bound):
    """worst |got - ref| / bound; inf when got is not finite (a NaN from outside a view or between the weight records reached it)."""
    got = got.to(torch.float64)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - ref).abs() / bound).max())


# ---- the image and fused block ops (tests/test_fp16_block_ops.py) ----
def poisoned_image(x, dtype, mis=0):
    """The BCHW image `x` as a whole tensor of `dtype` inside a larger NaN-filled device allocation: at least one image row (and 64
    elements) of NaN in front of it and behind it, its first element `mis` elements past a 128-byte boundary.  A read outside the
    image reaches the output as NaN.  -> (the allocation, the image: a view into it)."""
    n, pad = x.numel(), (x.shape[-1] + 63) // 64 * 64 + 64
    flat = torch.full((2 * pad + n + 8,), NAN, dtype=dtype)
    flat[pad + mis:pad + mis + n] = x.to(dtype).reshape(-1)
    flat = flat.to(DEV)
    img = flat[pad + mis:pad + mis + n].view(x.shape)
    assert img.is_contiguous() and img.data_ptr() % 128 == (mis * img.element_size()) % 128
    return flat, img


def image_view(slot):
    """The image as Plan.conv_first names it: the whole BCHW tensor of an external slot (ld and coff 0, C 3)."""
    return view(slot, 0, 0, 3)


def conv_first16_op(B, H, W, dst, w_off, b_off, in_dtype, act=1, img=None, ksize=3, stride=2, pad=1):
    """A fp16 CONV_FIRST op, fields as Plan.conv_first emits them and build_conv_first reads them: src0 = the image (slot 0 unless
    `img`), H / W its size, dst the NHWC f16 view, (w_off, b_off) the record packed with a zero 4th input channel."""
    from bs_yolo_amd import lib as L
    op = new_op(L.OP_CONV_FIRST, 0, B, H, W)
    op.OH, op.OW = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    op.ksize, op.stride, op.pad, op.act, op.dst_scale, op.in_dtype = ksize, stride, pad, int(act), 1, in_dtype
    op.src0, op.dst, op.w_off, op.b_off = image_view(0) if img is None else img, dst, w_off, b_off
    return op


def stem_op(B, H, W, dst, mid_c, rec0, rec1, in_dtype, act=1, img=None):
    """A STEM op, fields as Plan._fuse_stem emits them and build_stem reads them: H / W = the image, OH / OW = the layer-1 map,
    mid_c = C0, dst.C = C1, (w_off, b_off) = rec0 of layer 0, (w2_off, b2_off) = rec1 of layer 1."""
    from bs_yolo_amd import lib as L
    op = new_op(L.OP_STEM, 0, B, H, W)
    oh0, ow0 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    op.OH, op.OW = (oh0 - 1) // 2 + 1, (ow0 - 1) // 2 + 1
    op.ksize, op.stride, op.pad, op.act, op.dst_scale, op.in_dtype, op.mid_c = 3, 2, 1, int(act), 1, in_dtype, mid_c
    op.src0, op.dst = image_view(0) if img is None else img, dst
    (op.w_off, op.b_off), (op.w2_off, op.b2_off) = rec0, rec1
    return op


def bneck_op(B, H, W, src, dst, mid_c, rec1, rec2, act=1):
    """A BNECK op, fields as Plan.bottleneck emits them and build_bneck reads them: mid_c = the hidden width, rec1 / rec2 = the
    (w, b) records of cv1 / cv2; the shortcut is the source view itself."""
    from bs_yolo_amd import lib as L
    op = new_op(L.OP_BNECK, 0, B, H, W)
    op.ksize, op.stride, op.pad, op.act, op.dst_scale, op.mid_c = 3, 1, 1, int(act), 1, mid_c
    op.src0, op.dst = src, dst
    (op.w_off, op.b_off), (op.w2_off, op.b2_off) = rec1, rec2
    return op


def c3k2_op(B, H, W, src, dst, mid_c, recs):
    """A C3K2 op, fields as Plan.c2f emits them and build_c3k2 reads them: mid_c = c, aux_off[0..7] = the (w, b) records of cv1,
    m.cv1, m.cv2, cv2."""
    from bs_yolo_amd import lib as L
    op = new_op(L.OP_C3K2, 0, B, H, W)
    op.ksize, op.stride, op.pad, op.act, op.dst_scale, op.mid_c = 3, 1, 1, 1, 1, mid_c
    op.src0, op.dst = src, dst
    assert len(recs) == 4
    for j, (w_off, b_off) in enumerate(recs):
        op.aux_off[2 * j], op.aux_off[2 * j + 1] = w_off, b_off
    return op
