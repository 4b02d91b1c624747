"""Tensor-level wrappers over the stand-alone C entry points (same kernels the engine launches).

Used by the per-module hooks (plugin.py) and by the parity tests.  Activations are NHWC fp16 torch tensors
(``x.permute(0, 2, 3, 1).contiguous()`` of the reference's BCHW tensors) or channel slices of wider ones (`_nhwc`); every call runs
on the current stream.  Weights are given raw -- the module's fp32 (w, b), packed on every call -- or as the `Packed` pair a
``pack_*`` function returned, so that a caller packs once and calls many times.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import lib as L
from .weights import dense_f16, dense_f32, depthwise


def _stream(t: torch.Tensor):
    return L.stream_ptr(t.device)


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _nhwc(t: Optional[torch.Tensor]):
    """(pointer, ld, B, H, W, C) of an NHWC tensor, or of a channel slice of a wider one: channels adjacent, pixels `ld` elements apart
    in (b, h, w) order (stride(3) == 1, stride(2) == ld, stride(1) == W * ld, stride(0) == H * W * ld; a dimension of size 1 has no
    stride to speak of).  None -> a null pointer with ld 0."""
    if t is None:
        return None, 0, 0, 0, 0, 0
    B, H, W, c = t.shape
    ld = t.stride(2) if W > 1 else t.stride(1) if H > 1 else t.stride(0) if B > 1 else c
    assert all(n == 1 or s == e for n, s, e in zip(t.shape, t.stride(), (H * W * ld, W * ld, ld, 1))), (tuple(t.shape), t.stride())
    return _p(t), ld, B, H, W, c


class Packed(tuple):
    """(w, b): a conv's weights in a device layout of weights.py, on the device.  `shape` is the raw weight's (Cout, Cin, kh, kw), so a
    wrapper reads its widths off raw and packed weights alike."""
    def __new__(cls, w, b, shape):
        self = super().__new__(cls, (w, b))
        self.shape = tuple(shape)
        return self


def pack_conv_weight(w: torch.Tensor, b: Optional[torch.Tensor], device) -> Packed:
    """(Cout, Cin, k, k) fp32 [+ bias] -> packed fp16 [CoutPad][Kpad] + fp32 [CoutPad] on `device` (weights.dense_f16)."""
    wp, bp = dense_f16(w, b)
    return Packed(wp.to(device), bp.to(device), w.shape)


def pack_conv_weight_f32(w: torch.Tensor, b: torch.Tensor, device, split: bool = False) -> Packed:
    """(Cout, Cin, k, k) + bias -> ((f32 [K][Cout] matrix,) or, split, (matrix, hi, lo)) + f32 [Cout] on `device` (weights.dense_f32)."""
    mats, bp = dense_f32(w, b, split)
    return Packed(tuple(t.to(device) for t in mats), bp.to(device), w.shape)


def pack_dw_weight(w: torch.Tensor, b: torch.Tensor, device) -> Packed:
    """(C, 1, kh, kw) + bias -> f32 [kh*kw][C] + f32 [C] on `device` (weights.depthwise)."""
    wp, bp = depthwise(w, b)
    return Packed(wp.to(device), bp.to(device), w.shape)


def _packed(pack, w, b, device, **kw) -> Packed:
    return w if isinstance(w, Packed) else pack(w, b, device, **kw)


def _out_hw(H: int, W: int, kh: int, kw: int, s: int):
    return (H + 2 * (kh // 2) - kh) // s + 1, (W + 2 * (kw // 2) - kw) // s + 1


def conv2d_nhwc(x: torch.Tensor, wp: torch.Tensor, bp: torch.Tensor, cout: int, k: int, s: int = 1, act: bool = True,
                res: Optional[torch.Tensor] = None, out_f32: bool = False, cin: Optional[int] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B,H,W,C) fp16 view (uses the first `cin` channels), (wp, bp) = pack_conv_weight(...) -> (B,OH,OW,cout), into the view `out`
    where one is given.  Conv.forward_fuse (conv.py:149-151)."""
    assert x.dtype == torch.float16
    px, ld, B, H, W, c = _nhwc(x)
    cin = c if cin is None else cin
    if out is None:
        ldy = (cout + 3) // 4 * 4 if out_f32 else (cout + 7) // 8 * 8
        out = torch.zeros((B, *_out_hw(H, W, k, k, s), ldy), dtype=torch.float32 if out_f32 else torch.float16, device=x.device)
    L.check(L.lib.bsy_conv2d(px, ld, B, H, W, cin, _p(wp), _p(bp), *_nhwc(out)[:2], cout, k, s, int(act), *_nhwc(res)[:2], int(out_f32),
                             _stream(x)))
    return out


def _conv2d_f32(x, w, b, k, s, cin, split):
    """What both fp32-storage convs do before their call: the packed weights, the input view and a new zeroed output."""
    assert x.dtype == torch.float32
    px, ld, B, H, W, c = _nhwc(x)
    cin = c if cin is None else cin
    cout = w.shape[0]
    assert tuple(w.shape) == (cout, cin, k, k)
    mats, bk = _packed(pack_conv_weight_f32, w, b, x.device, split=split)
    ldy = (cout + 3) // 4 * 4
    out = torch.zeros((B, *_out_hw(H, W, k, k, s), ldy), dtype=torch.float32, device=x.device)
    return mats, bk, (px, ld, B, H, W, cin), out, ldy, cout


def conv2d_nhwc_f32(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, k: int, s: int = 1, act: bool = True,
                    res: Optional[torch.Tensor] = None, cin: Optional[int] = None, impl: int = 0) -> torch.Tensor:
    """fp32 engine mode's conv: x (B,H,W,C) f32 view (first `cin` channels), w (Cout,Cin,k,k) f32, b (Cout) -- or w =
    pack_conv_weight_f32(w, b, device) -- -> (B,OH,OW,Cout) f32.
    impl 0 = the engine's routing, 1 = scalar kernel, 2 = fp32 MFMA kernel (bsy_conv2d_f32)."""
    mats, bk, xa, out, ldy, cout = _conv2d_f32(x, w, b, k, s, cin, False)
    L.check(L.lib.bsy_conv2d_f32(*xa, _p(mats[0]), _p(bk), _p(out), ldy, cout, k, s, int(act), *_nhwc(res)[:2], impl, _stream(x)))
    return out


def conv2d_nhwc_f32x(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, k: int, s: int = 1, act: bool = True,
                     res: Optional[torch.Tensor] = None, cin: Optional[int] = None) -> torch.Tensor:
    """fp32x engine mode's conv (bsy_conv2d_f32x): fp32 NHWC in / out, operands split into f16 pairs, three f16 MFMAs per product.
    x (B,H,W,C) f32 view (first `cin` channels), w (Cout,Cin,k,k) f32, b (Cout) -- or w = pack_conv_weight_f32(w, b, device,
    split=True) -- -> (B,OH,OW,Cout up 4) f32."""
    (_, hi, lo), bk, xa, out, ldy, cout = _conv2d_f32(x, w, b, k, s, cin, True)
    L.check(L.lib.bsy_conv2d_f32x(*xa, _p(hi), _p(lo), hi.shape[1], _p(bk), _p(out), ldy, cout, k, s, int(act), *_nhwc(res)[:2],
                                  _stream(x)))
    return out


def conv_first(img: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None, k: int = 3, s: int = 2, act: bool = True,
               out: Optional[torch.Tensor] = None):
    """img BCHW fp16/fp32; w (Cout,3,3,3) fp32, b (Cout) -- or w = pack_conv_weight(w, b, device); -> NHWC fp16."""
    assert img.is_contiguous() and img.shape[1] == 3
    B, _, H, W = img.shape
    cout = w.shape[0]
    wp, bp = _packed(pack_conv_weight, w, b, img.device)
    if out is None:
        out = torch.empty((B, *_out_hw(H, W, k, k, s), cout), dtype=torch.float16, device=img.device)
    L.check(L.lib.bsy_conv_first(_p(img), L.dtype_code(img.dtype), B, H, W, _p(wp), _p(bp), *_nhwc(out)[:2], cout, k, s, int(act),
                                 _stream(img)))
    return out


def stem_fused(img: torch.Tensor, w0: torch.Tensor, b0: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
               act: bool = True) -> torch.Tensor:
    """Layers 0 + 1 in one launch: img BCHW fp16/fp32; w0 (C0,3,3,3), w1 (C1,C0,3,3) fp32 -> NHWC fp16 (B,H/4,W/4,C1)."""
    assert img.is_contiguous() and img.shape[1] == 3
    B, _, H, W = img.shape
    c0, c1 = w0.shape[0], w1.shape[0]
    w0p, b0p = _packed(pack_conv_weight, w0, b0, img.device)
    w1p, b1p = _packed(pack_conv_weight, w1, b1, img.device)
    oh0, ow0 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((B, (oh0 - 1) // 2 + 1, (ow0 - 1) // 2 + 1, c1), dtype=torch.float16, device=img.device)
    L.check(L.lib.bsy_stem_fused(_p(img), L.dtype_code(img.dtype), B, H, W, _p(w0p), _p(b0p), c0, _p(w1p), _p(b1p), c1,
                                 _p(out), c1, int(act), _stream(img)))
    return out


def bottleneck_fused(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x + cv2(cv1(x)) in one launch.  x, out: (B,H,W,C) fp16 NHWC, possibly channel slices of wider buffers
    (stride(2) = leading dimension); w1 (CH,C,3,3), w2 (C,CH,3,3) fp32 (BN already folded) with their biases, or pack_conv_weight's
    pairs in the place of w1 / w2."""
    px, ld, B, H, W, c = _nhwc(x)
    ch = w1.shape[0]
    w1p, b1p = _packed(pack_conv_weight, w1, b1, x.device)
    w2p, b2p = _packed(pack_conv_weight, w2, b2, x.device)
    if out is None:
        out = torch.empty((B, H, W, c), dtype=torch.float16, device=x.device)
    assert out.shape == x.shape
    L.check(L.lib.bsy_bottleneck_fused(px, ld, B, H, W, c, ch, _p(w1p), _p(b1p), _p(w2p), _p(b2p), *_nhwc(out)[:2], 1, _stream(x)))
    return out


def c3k2_fused(x: torch.Tensor, w1, b1, wa, ba, wb, bb, w4, b4, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Whole C3k2 block (c3k = False, one Bottleneck; block.py:3796-3804) in one launch: x (B,H,W,Cin) fp16 NHWC view ->
    (B,H,W,C2).  w1 (2c,Cin,1,1), wa (c/2,c,3,3), wb (c,c/2,3,3), w4 (C2,3c,1,1) fp32 with BN folded, biases fp32; or
    pack_conv_weight's pairs in the place of the weights."""
    px, ld, B, H, W, cin = _nhwc(x)
    c, c2 = wb.shape[0], w4.shape[0]
    packs = [_packed(pack_conv_weight, w, b, x.device) for w, b in ((w1, b1), (wa, ba), (wb, bb), (w4, b4))]  # (alive until the launch)
    if out is None:
        out = torch.empty((B, H, W, c2), dtype=torch.float16, device=x.device)
    assert out.shape == (B, H, W, c2)
    L.check(L.lib.bsy_c3k2_fused(px, ld, B, H, W, cin, c, c2, *[_p(t) for pk in packs for t in pk], *_nhwc(out)[:2], _stream(x)))
    return out


def dwpw_fused(x: torch.Tensor, wd: torch.Tensor, bd: torch.Tensor, w: torch.Tensor, b: torch.Tensor, act: bool = True) -> torch.Tensor:
    """DWConv 3x3 + SiLU -> Conv 1x1 (+act) in one launch.  x (B,H,W,C) fp16 view; wd (C,1,3,3), bd (C) or pack_dw_weight's pair;
    w (C2,C,1,1), b (C2) or pack_conv_weight's pair."""
    px, ld, B, H, W, Cc = _nhwc(x)
    c2 = w.shape[0]
    wdp, bdp = _packed(pack_dw_weight, wd, bd, x.device)
    wp, bp = _packed(pack_conv_weight, w, b, x.device)
    out = torch.empty((B, H, W, c2), dtype=torch.float16, device=x.device)
    L.check(L.lib.bsy_dwpw_fused(px, ld, B, H, W, Cc, _p(wdp), _p(bdp), _p(wp), _p(bp), _p(out), c2, c2, int(act), _stream(x)))
    return out


def dwconv_nhwc(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None, stride: int = 1, act: bool = False,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Depthwise kh x kw conv, padding k/2 (csrc/bsyolo_ops.hip).  x (B,H,W,C) fp16 view; w (C,1,kh,kw) fp32, b (C) -- or w =
    pack_dw_weight(w, b, device)."""
    px, ld, B, H, W, Cc = _nhwc(x)
    kh, kw = int(w.shape[2]), int(w.shape[3])
    wp, bp = _packed(pack_dw_weight, w, b, x.device)
    if out is None:
        out = torch.empty((B, *_out_hw(H, W, kh, kw, stride), Cc), dtype=torch.float16, device=x.device)
    L.check(L.lib.bsy_dwconv(px, ld, B, H, W, Cc, kh, kw, stride, _p(wp), Cc, _p(bp), *_nhwc(out)[:2], int(act), _stream(x)))
    return out


def ela_nhwc(x: torch.Tensor, wsp: torch.Tensor, wch: torch.Tensor, gnw: torch.Tensor, gnb: torch.Tensor, coef) -> torch.Tensor:
    """ELA.forward (nn/Addmodules/ELA.py:77-101).  x (B,H,W,C) fp16; wsp / wch (C,1,k) Conv1d weights; coef = the three
    sigmoids (ch, sp, res)."""
    B, H, W, Cc = x.shape
    k = int(wsp.shape[-1])
    dev = x.device
    f = lambda t: t.detach().float().reshape(-1).contiguous().to(dev)  # noqa: E731
    a, b_, c, d = f(wsp), f(wch), f(gnw), f(gnb)
    scratch = torch.empty(int(L.lib.bsy_ela_scratch_bytes(B, H, W, Cc)) // 4, dtype=torch.float32, device=dev)
    out = torch.empty_like(x)
    cf = (C.c_float * 3)(*[float(v) for v in coef])
    L.check(L.lib.bsy_ela(_p(x), Cc, B, H, W, Cc, k, _p(a), _p(b_), _p(c), _p(d), cf, _p(scratch), _p(out), Cc, _stream(x)))
    return out


def dwconv3x3_nhwc(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None, act: bool = True,
                   res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B,H,W,C) fp16 view, res likewise; w (C,1,3,3) fp32, b (C) -- or w = pack_dw_weight(w, b, device).  DWConv (conv.py:224-229)."""
    px, ld, B, H, W, Cc = _nhwc(x)
    wp, bp = _packed(pack_dw_weight, w, b, x.device)
    out = torch.empty((B, H, W, Cc), dtype=x.dtype, device=x.device)
    L.check(L.lib.bsy_dwconv3x3(px, ld, B, H, W, Cc, _p(wp), _p(bp), _p(out), Cc, int(act), *_nhwc(res)[:2], _stream(x)))
    return out


def sppf_pool_nhwc(x1: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x1 (B,H,W,C) -> (B,H,W,4C) = cat[x1, m(x1), m(m(x1)), m(m(m(x1)))], m = MaxPool2d(5,1,2) (block.py:3145-3149).  `out`: the
    (B,H,W,4C) concat buffer (a view) whose first C channels are x1 itself; the pools fill the rest in place."""
    B, H, W, Cc = x1.shape
    if out is None:
        out = torch.zeros((B, H, W, 4 * Cc), dtype=torch.float16, device=x1.device)
        out[..., :Cc] = x1
    else:
        assert out.shape == (B, H, W, 4 * Cc) and out.data_ptr() == x1.data_ptr()
    L.check(L.lib.bsy_sppf_pool(*_nhwc(out)[:2], B, H, W, Cc, _stream(x1)))
    return out


def pool_down_nhwc(x: torch.Tensor, mode: int, C: Optional[int] = None, coff: int = 0, out: Optional[torch.Tensor] = None,
                   out_coff: int = 0) -> torch.Tensor:
    """The pooling front end of AConv / ADown (block.py:3692-3723) on channels [coff, coff + C) of x (B,H,W,ld), fp16 or fp32, H and W
    even.  mode 0: avg_pool2d(x, 2, 1) on an (B,H,W) map whose last row and column are zero; mode 1: max_pool2d(avg_pool2d(x, 2, 1),
    3, 2, 1) on (B,H/2,W/2).  Written into channels [out_coff, out_coff + C) of `out` (a new C-channel tensor when None)."""
    assert x.is_contiguous() and x.dim() == 4
    B, H, W, ld = x.shape
    C = ld - coff if C is None else C
    if out is None:
        out = torch.empty((B, H // 2, W // 2, C) if mode else (B, H, W, C), dtype=x.dtype, device=x.device)
    assert out.is_contiguous() and out.dtype == x.dtype
    L.check(L.lib.bsy_pool_down(_p(x), ld, coff, _p(out), out.shape[-1], out_coff, B, H, W, C, int(mode), L.dtype_code(x.dtype),
                                _stream(x)))
    return out


def attention_nhwc(qkv: torch.Tensor, heads: int, key_dim: int, head_dim: int, scale: float) -> torch.Tensor:
    """qkv (B,N,heads*(2kd+hd)) fp16 in [q|k|v] (all-heads-contiguous) order -> (B,N,heads*hd) (block.py:4279-4286)."""
    B, N, ld = qkv.shape
    out = torch.empty((B, N, heads * head_dim), dtype=torch.float16, device=qkv.device)
    L.check(L.lib.bsy_attention(_p(qkv), ld, B, N, heads, key_dim, head_dim, float(scale), _p(out), heads * head_dim,
                                _stream(qkv)))
    return out


def attention_pe_nhwc(qkv: torch.Tensor, heads: int, key_dim: int, head_dim: int, scale: float,
                      pe_w: Optional[torch.Tensor] = None, pe_b: Optional[torch.Tensor] = None, impl: int = 0,
                      out: Optional[torch.Tensor] = None, out_coff: int = 0) -> torch.Tensor:
    """qkv (B,H,W,heads*(2kd+hd)) fp16 in [q|k|v] order -> attention + pe(v) (B,H,W,heads*hd) in one launch (block.py:4279-4286).
    pe_w (heads*hd,1,3,3) / pe_b (heads*hd): Attention.pe's folded depthwise conv; None runs the attention alone.  impl 0 auto /
    1 resident / 2 streaming kernel form.  `out` (B,H,W,>= out_coff + heads*hd), a view: written at channel out_coff, the rest untouched.
    pe_w may be pack_dw_weight's pair."""
    assert qkv.dim() == 4
    pq, ld, B, H, W, _ = _nhwc(qkv)
    Cc = heads * head_dim
    if out is None:
        out = torch.empty((B, H, W, Cc), dtype=torch.float16, device=qkv.device)
    assert out.dtype == torch.float16 and out.shape[:3] == qkv.shape[:3] and out.shape[3] >= out_coff + Cc
    wp, bp = _packed(pack_dw_weight, pe_w, pe_b, qkv.device) if pe_w is not None else (None, None)
    L.check(L.lib.bsy_attention_pe(pq, ld, B, H, W, heads, key_dim, head_dim, float(scale), _p(wp), _p(bp), *_nhwc(out[..., out_coff:])[:2],
                                   int(impl), _stream(qkv)))
    return out


def detect_decode(box: Sequence[torch.Tensor], cls: Sequence[torch.Tensor], hw: Sequence[tuple],
                  strides: Sequence[float], nc: int, out_dtype=torch.float32,
                  msk: Optional[Sequence[torch.Tensor]] = None, xyxy: bool = False) -> torch.Tensor:
    """box[l], cls[l] [, msk[l]] f32: (B*h*w, 64 / >= nc / nm) matrices, or (B, h, w, .) maps -- also channel slices of one (B, h, w, no)
    tensor per level, rows a multiple of 4 floats apart -> (B, 4+nc+nm, A) (head.py:100-131).  xyxy: the boxes as corners, the form an
    end2end head decodes (head.py:148; bsy_detect_decode_fmt); False is bsy_detect_decode as it always was."""
    nl = len(box)
    B = box[0].numel() // (box[0].shape[-1] * hw[0][0] * hw[0][1])
    nm = msk[0].shape[-1] if msk else 0
    A = sum(h * w for h, w in hw)
    y = torch.empty((B, 4 + nc + nm, A), dtype=out_dtype, device=box[0].device)
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float

    def rows(ts):  # (pointers, leading dimensions) of one tensor per level
        if not ts:
            return None, None
        return (vp * nl)(*[t.data_ptr() for t in ts]), (i32 * nl)(*[_nhwc(t)[1] if t.dim() == 4 else t.stride(0) for t in ts])

    hh = (i32 * nl)(*[h for h, _ in hw])
    ww = (i32 * nl)(*[w for _, w in hw])
    st = (f32 * nl)(*[float(s) for s in strides])
    if xyxy:
        L.check(L.lib.bsy_detect_decode_fmt(*rows(box), *rows(cls), *rows(msk), hh, ww, st, nl, B, nc, nm, 1, _p(y), L.dtype_code(out_dtype),
                                            _stream(y)))
        return y
    L.check(L.lib.bsy_detect_decode(*rows(box), *rows(cls), *rows(msk), hh, ww, st, nl, B, nc, nm, _p(y), L.dtype_code(out_dtype),
                                    _stream(y)))
    return y


def kpts_decode(kpt: torch.Tensor, hw: Sequence[tuple], strides: Sequence[float], kpt_shape, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pose.kpts_decode, the non-export branch (head.py:273-279), in one launch: kpt (B, nkpt * ndim, A) fp16 / fp32, contiguous and
    left as it is -> (B, nkpt * ndim, A) of the same dtype.  hw: the levels' (h, w), strides: theirs.  `out`: where to write instead
    of a new tensor -- a (B, nk, A) tensor or view whose images are contiguous (nk, A) blocks, e.g. ``pred[:, 4 + nc:]`` of a
    preallocated (B, 4 + nc + nk, A) prediction, which saves Pose.forward's final torch.cat.  No allocation with `out`, no sync."""
    nkpt, ndim = int(kpt_shape[0]), int(kpt_shape[1])
    nl, nk = len(hw), nkpt * ndim
    if not (kpt.is_cuda and kpt.dim() == 3 and kpt.is_contiguous() and kpt.shape[1] == nk):
        raise ValueError("kpts_decode: kpt must be a contiguous (B, nkpt * ndim, A) device tensor")
    B, _, A = kpt.shape
    if out is None:
        out = torch.empty_like(kpt)
    if (out.dtype != kpt.dtype or out.device != kpt.device or tuple(out.shape) != (B, nk, A) or out.stride(2) != 1 or out.stride(1) != A
            or (B > 1 and out.stride(0) < nk * A)):
        raise ValueError("kpts_decode: out must be (B, nkpt * ndim, A) of kpt's dtype with contiguous (nk, A) images")
    i32, f32 = C.c_int, C.c_float
    hh = (i32 * nl)(*[int(h) for h, _ in hw])
    ww = (i32 * nl)(*[int(w) for _, w in hw])
    st = (f32 * nl)(*[float(s) for s in strides])
    L.check(L.lib.bsy_kpts_decode(_p(kpt), L.dtype_code(kpt.dtype), B, nkpt, ndim, A, hh, ww, st, nl, _p(out),
                                  out.stride(0) if B > 1 else nk * A, _stream(kpt)))
    return out


def scale_img(x: torch.Tensor, ratio: float, flip: Optional[int] = None, gs: int = 32,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scale_img(x.flip(flip) if flip else x, ratio, gs=gs) (utils/torch_utils.py:430-442) in one launch (bsy_scale_img): x (B,C,H,W)
    fp16 / fp32 -> (B,C,PH,PW) of the same dtype.  Unlike the reference, ratio 1.0 with a flip still writes a new tensor."""
    from .tta import scaled_size
    assert x.is_contiguous() and x.dim() == 4 and x.dtype in (torch.float16, torch.float32)
    B, Cc, H, W = x.shape
    (oh, ow), (ph, pw) = scaled_size(H, W, ratio, gs)
    if out is None:
        out = torch.empty((B, Cc, ph, pw), dtype=x.dtype, device=x.device)
    assert out.is_contiguous() and tuple(out.shape) == (B, Cc, ph, pw) and out.dtype == x.dtype
    L.check(L.lib.bsy_scale_img(_p(x), L.dtype_code(x.dtype), B, Cc, H, W, oh, ow, ph, pw, int(flip or 0), _p(out), _stream(x)))
    return out


def tta_merge(ys: Sequence[torch.Tensor], windows: Sequence[tuple], scales: Sequence[float], flips: Sequence[Optional[int]],
              img_hw: tuple, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """_descale_pred + _clip_augmented + torch.cat(y, -1) (nn/tasks.py:366-391) in one launch (bsy_tta_merge): ys[p] (B,no,A_p) of one
    dtype, windows[p] = the kept anchors [begin, end) -> (B, no, sum of the window lengths)."""
    n = len(ys)
    y0 = ys[0]
    B, no = y0.shape[:2]
    for y in ys:
        assert y.is_contiguous() and y.dim() == 3 and tuple(y.shape[:2]) == (B, no) and y.dtype == y0.dtype and y.device == y0.device
    total = sum(e - b for b, e in windows)
    if out is None:
        out = torch.empty((B, no, total), dtype=y0.dtype, device=y0.device)
    assert out.is_contiguous() and tuple(out.shape) == (B, no, total) and out.dtype == y0.dtype
    i32 = C.c_int32
    L.check(L.lib.bsy_tta_merge((C.c_void_p * n)(*[y.data_ptr() for y in ys]), (i32 * n)(*[y.shape[2] for y in ys]),
                                (i32 * n)(*[b for b, _ in windows]), (i32 * n)(*[e for _, e in windows]),
                                (C.c_float * n)(*[float(s) for s in scales]), (i32 * n)(*[int(f or 0) for f in flips]), n, B, no,
                                int(img_hw[0]), int(img_hw[1]), L.dtype_code(y0.dtype), _p(out), _stream(out)))
    return out


def end2end_topk(pred: torch.Tensor, max_det: int = 300, out: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """v10Detect.postprocess(pred.permute(0, 2, 1), max_det, nc) (nn/modules/head.py:151-172) in two launches (bsy_end2end_topk):
    pred (B, 4+nc, A) fp16 / fp32 on the device -> (B, min(max_det, A), 6) fp32 rows [box, score, class].  Ties go to the lower
    anchor, then the lower class (include/bsyolo.h).  No host synchronisation; `out` / `workspace` may be preallocated (graph capture)."""
    if not pred.is_cuda:
        raise RuntimeError("bs_yolo_amd.ops.end2end_topk needs a GPU tensor (no CPU fallback)")
    if pred.dim() != 3 or pred.shape[1] < 5:
        raise ValueError("pred must be (B, 4+nc, A)")
    pred = pred.contiguous()
    B, Cc, A = pred.shape
    nc = Cc - 4
    K = min(int(max_det), A)
    nbytes = L.lib.bsy_end2end_topk_workspace_bytes(B, A, nc, int(max_det))
    if workspace is None:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=pred.device)
    if out is None:
        out = torch.empty((B, K, 6), dtype=torch.float32, device=pred.device)
    assert out.is_contiguous() and tuple(out.shape) == (B, K, 6) and out.dtype == torch.float32
    L.check(L.lib.bsy_end2end_topk(_p(pred), L.dtype_code(pred.dtype), B, nc, A, int(max_det), _p(out), _p(workspace),
                                   workspace.numel() * workspace.element_size(), _stream(pred)))
    return out


def classify_tail(logits: torch.Tensor, nc: int, k: int = 0, out_dtype: torch.dtype = torch.float32):
    """Classify's tail (nn/modules/head.py:300-304) in one launch (bsy_classify_tail): logits (B, ld) fp32 on the device, ld a multiple
    of 4 and >= nc, rows 16-byte aligned -> (y, x, idx, val): y = softmax(logits[:, :nc]) and x = logits[:, :nc], (B, nc) each in
    out_dtype; idx (int32) / val (fp32), (B, k): the k most probable classes by the STORED y, descending, ties to the lower class
    (a stable descending sort of y) -- None, None with k = 0.  Columns past nc are never read.  No host synchronisation."""
    if not logits.is_cuda:
        raise RuntimeError("bs_yolo_amd.ops.classify_tail needs a GPU tensor (no CPU fallback)")
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("logits must be a contiguous (B, ld) fp32 tensor")
    B, ld = logits.shape
    y = torch.empty((B, nc), dtype=out_dtype, device=logits.device)
    x = torch.empty((B, nc), dtype=out_dtype, device=logits.device)
    idx = torch.empty((B, k), dtype=torch.int32, device=logits.device) if k else None
    val = torch.empty((B, k), dtype=torch.float32, device=logits.device) if k else None
    L.check(L.lib.bsy_classify_tail(_p(logits), ld, B, int(nc), _p(y), _p(x), L.dtype_code(out_dtype), int(k),
                                    _p(idx) if k else None, _p(val) if k else None, _stream(logits)))
    return y, x, idx, val


def maxsig_attn(embed: torch.Tensor, proj: torch.Tensor, G: torch.Tensor, bias: torch.Tensor, scale, nh: int,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MaxSigmoidAttnBlock's gate (nn/modules/block.py:3483-3515) in one launch (bsy_maxsig_attn): embed, proj (B,H,W,C) NHWC fp16 or fp32
    on the device (or channel slices of wider tensors), C = nh * hc; G (nc, C) the guide rows with the block's 1 / sqrt(hc) folded in,
    bias (nh), scale (nh) or a float.  For pixel p and head m: out[p, m hc + j] = proj[p, m hc + j] * scale[m] * sigmoid(max_n
    <embed[p, head m], G[n, head m]> + bias[m]).  out: proj itself (in place) or another tensor of its shape; None = a new one.  It must
    not overlap embed.  fp16: hc a multiple of 16 from 16 to 128 (the guide is rounded to f16, its rows padded by weights.guide)."""
    from .weights import guide
    if not embed.is_cuda:
        raise RuntimeError("bs_yolo_amd.ops.maxsig_attn needs GPU tensors (no CPU fallback)")
    pe, lde, B, H, W, Cc = _nhwc(embed)
    pp, ldp, *shape_p = _nhwc(proj)
    if out is None:
        out = torch.empty((B, H, W, Cc), dtype=embed.dtype, device=embed.device)
    po, ldo, *shape_o = _nhwc(out)
    assert tuple(shape_p) == tuple(shape_o) == (B, H, W, Cc) and proj.dtype == out.dtype == embed.dtype and Cc % int(nh) == 0
    G = torch.as_tensor(G).detach().cpu()
    nc = G.shape[0] if G.dim() == 2 else 0
    assert G.dim() == 2 and G.shape[1] == Cc
    f32 = embed.dtype == torch.float32
    gp = guide(G.double(), f32).to(embed.device) if nc else torch.zeros(32, Cc, dtype=embed.dtype, device=embed.device)
    sc = torch.as_tensor(scale, dtype=torch.float32).reshape(-1).cpu()
    bs = torch.cat([torch.as_tensor(bias, dtype=torch.float32).reshape(-1).cpu(), sc.expand(int(nh)) if sc.numel() == 1 else sc]).to(embed.device)
    assert bs.numel() == 2 * int(nh)
    L.check(L.lib.bsy_maxsig_attn(pe, lde, pp, ldp, po, ldo, B, H, W, int(nh), Cc // int(nh), _p(gp), int(nc), _p(bs), L.dtype_code(embed.dtype),
                                  _stream(embed)))
    return out


def cbfuse(taps: Sequence[torch.Tensor], shifts: Sequence[int], last: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CBFuse (nn/modules/block.py:3760-3772) in one launch (bsy_cbfuse): last (B,H,W,C) NHWC fp16 or fp32 on the device (or a channel
    slice of a wider tensor); taps: 1 to 5 NHWC tensors or channel slices, tap i of (B, H >> shifts[i], W >> shifts[i], >= C), of which the
    first C channels are read through nearest upsampling by 2^shifts[i] (0 .. 4).  out = tap 0 + ... + tap n-1 + last, summed in f32 in
    that order and rounded once.  out: `last` itself (in place) or another tensor of its shape; None = a new one.  It must not overlap a
    tap.  Every argument is checked before anything is launched."""
    taps, shifts = list(taps), [int(k) for k in shifts]
    if not last.is_cuda or not all(t.is_cuda for t in taps):
        raise RuntimeError("bs_yolo_amd.ops.cbfuse needs GPU tensors (no CPU fallback)")
    if not 1 <= len(taps) <= L.BSY_CBFUSE_MAX_TAPS or len(shifts) != len(taps):
        raise ValueError(f"cbfuse: {len(taps)} taps with {len(shifts)} shifts (1 to {L.BSY_CBFUSE_MAX_TAPS} taps, a shift each)")
    pl, ldl, B, H, W, Cc = _nhwc(last)
    if out is None:
        out = torch.empty((B, H, W, Cc), dtype=last.dtype, device=last.device)
    po, ldo, *shape_o = _nhwc(out)
    if tuple(shape_o) != (B, H, W, Cc):
        raise ValueError(f"cbfuse: out is {tuple(out.shape)}, last {tuple(last.shape)}")
    if last.dtype not in (torch.float16, torch.float32) or any(t.dtype != last.dtype for t in taps + [out]):
        raise ValueError(f"cbfuse: mixed storage types {[str(t.dtype) for t in taps + [last, out]]} (all fp16 or all fp32)")
    ptrs, lds = [], []
    for i, (t, k) in enumerate(zip(taps, shifts)):
        if not 0 <= k <= 4:
            raise ValueError(f"cbfuse: tap {i} has shift {k} (0 to 4)")
        if H % (1 << k) or W % (1 << k):
            raise ValueError(f"cbfuse: tap {i}: {H} x {W} is not divisible by {1 << k}")
        pt, ldt, Bt, Ht, Wt, Ct = _nhwc(t)
        if (Bt, Ht, Wt) != (B, H >> k, W >> k):
            raise ValueError(f"cbfuse: tap {i} is {tuple(t.shape)}, the target {tuple(last.shape)} over 2^{k}")
        if Ct < Cc:
            raise ValueError(f"cbfuse: tap {i} is narrower ({Ct} channels) than the target ({Cc})")
        ptrs.append(pt.value)
        lds.append(ldt)
    n = len(taps)
    L.check(L.lib.bsy_cbfuse((C.c_void_p * n)(*ptrs), (C.c_int * n)(*lds), (C.c_int * n)(*shifts), n, pl, ldl, po, ldo, B, H, W, Cc,
                             L.dtype_code(last.dtype), _stream(last)))
    return out
