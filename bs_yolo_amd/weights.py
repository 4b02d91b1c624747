"""Weight preparation: BN folding + packing into the engine's device blob.

  * fold_conv_bn  -- the arithmetic of utils/torch_utils.py:242-269 fuse_conv_and_bn (called per Conv by
                     BaseModel.fuse, nn/tasks.py:209-215): W' = diag(g / sqrt(var + eps)) W,  b' = beta - g mu / sqrt(var + eps).
                     Accepts either an un-fused state_dict (conv.weight + bn.*) or an already fused one
                     (conv.weight + conv.bias), which is what a reference model holds after AutoBackend's fuse().
  * pack_record   -- three steps, each stated once: the record's SOURCE reads the module's fp32 (w, b) from the state dict (SOURCES:
                     key names, the module's own shapes and synth_state_dict's draws side by side), op_channels re-lays them out
                     to the op's channels, and a LAYOUT function writes the device form:
                     dense_f16  : fp16 [CoutPad][Kpad], K order (kh, kw, cin), bias fp32 [CoutPad]  (conv_gemm.hip, conv_first.hip)
                     dense_f32  : f32 [K][Cout] (+ the split-f16 planes of the fp32x mode), bias f32 [Cout]  (ref32.hip, conv32x_mfma.hip)
                     depthwise  : f32 [kh*kw][C], bias f32 [C]  (elementwise.hip, bsyolo_ops.hip)
                     guide      : a C2fAttn block's text rows behind its Linear, [rows][C] f16 (rows padded to 32 with copies of row 0) or
                                  f32, and f32 [bias | scale]  (maxsig.hip; record kind "maxsig")
  * YOLO-World   -- the text features travel in the state dict under the reserved key "txt_feats", (nc, E) or (1, nc, E).  Two record kinds
                     fold them in, in float64, rounded once to the storage type: "maxsig" (above) and "world_cls", WorldDetect's BatchNorm
                     contrastive head folded into the class branch's last 1x1 conv.
                     The stand-alone operators (ops.py) and the per-module hooks (plugin.py) pack with the same three functions.
"""
from __future__ import annotations

import ctypes
import math
import re
from typing import Dict, List, Mapping, Tuple

import numpy as np
import torch

from . import lib as L
from .plan import Plan, WRec

BN_EPS = 1e-3  # utils/torch_utils.py:424


def _f32(t) -> torch.Tensor:
    return torch.as_tensor(t).detach().to("cpu", torch.float32)


def _f64(t) -> torch.Tensor:
    return torch.as_tensor(t).detach().to("cpu", torch.float64)


def _real(t) -> torch.Tensor:
    """A record's values on the CPU: float64 stays (the YOLO-World folds, rounded once by the layout), everything else becomes fp32."""
    t = torch.as_tensor(t).detach().to("cpu")
    return t if t.dtype == torch.float64 else t.to(torch.float32)


def _to_f16(t: torch.Tensor) -> torch.Tensor:
    """Round to f16 ONCE: torch converts float64 through float32 (two roundings), numpy does not."""
    return torch.from_numpy(t.contiguous().numpy().astype(np.float16)) if t.dtype == torch.float64 else t.to(torch.float16)


def fold_conv_bn(sd: Mapping[str, torch.Tensor], prefix: str, eps: float = BN_EPS):
    """(weight, bias) fp32 of `prefix` (a reference Conv module) with BatchNorm folded in."""
    w = _f32(sd[prefix + ".conv.weight"])
    if prefix + ".bn.weight" in sd:
        g, beta = _f32(sd[prefix + ".bn.weight"]), _f32(sd[prefix + ".bn.bias"])
        mu, var = _f32(sd[prefix + ".bn.running_mean"]), _f32(sd[prefix + ".bn.running_var"])
        scale = g / torch.sqrt(var + eps)
        w = w * scale.view(-1, 1, 1, 1)
        b = beta - g * mu / torch.sqrt(var + eps)
        if prefix + ".conv.bias" in sd:
            b = b + scale * _f32(sd[prefix + ".conv.bias"])
    else:
        b = _f32(sd[prefix + ".conv.bias"])
    return w, b


def fold_refconv(sd: Mapping[str, torch.Tensor], prefix: str):
    """(weight, bias) fp32 of the fork's RepConv (block.py:793-816), the form every yaml-built RepBottleneck.cv1 has: a bare conv whose
    kernel is weight + convmap(weight), convmap a 3x3 conv over the co * ci two-dimensional kernels with one group each and no bias
    (:813-815).  No BatchNorm, no bias, no activation: the bias is zero."""
    w = _f32(sd[prefix + ".weight"])
    co, ci, kh, kw = w.shape
    cm = _f32(sd[prefix + ".convmap.weight"])
    assert tuple(cm.shape[:2]) == (co * ci, 1), (prefix, tuple(cm.shape))
    k = w + torch.nn.functional.conv2d(w.view(1, co * ci, kh, kw), cm, None, 1, cm.shape[-1] // 2, 1, co * ci).view_as(w)
    return k, torch.zeros(co)


def fold_repvgg(sd: Mapping[str, torch.Tensor], prefix: str, eps: float = BN_EPS):
    """(weight, bias) fp32 of upstream's RepConv (conv.py:296-397; what an upstream-pickled YOLOv9 checkpoint holds): SiLU(conv1(x) +
    conv2(x)), a 3x3 and a 1x1 Conv with BatchNorm each, folded as get_equivalent_kernel_bias does (:328-369) -- every branch folded
    with its BN, the 1x1 kernel padded to the centre tap, kernels and biases added.  A model that went through fuse() holds the
    result as conv.weight / conv.bias and is taken as it is.  (The optional identity-BN branch, bn=True, is not built by RepBottleneck.)"""
    if prefix + ".conv1.conv.weight" not in sd:
        return _f32(sd[prefix + ".conv.weight"]), _f32(sd[prefix + ".conv.bias"])
    if prefix + ".bn.weight" in sd:
        raise NotImplementedError(f"{prefix}: RepConv with an identity BatchNorm branch (bn=True) is not folded")
    w3, b3 = fold_conv_bn(sd, prefix + ".conv1", eps)
    w1, b1 = fold_conv_bn(sd, prefix + ".conv2", eps)
    assert w3.shape[-1] == 3 and w1.shape[-1] == 1, (prefix, tuple(w3.shape), tuple(w1.shape))
    return w3 + torch.nn.functional.pad(w1, [1, 1, 1, 1]), b3 + b1


def fold_repvggdw(sd: Mapping[str, torch.Tensor], prefix: str, eps: float = BN_EPS):
    """(weight (C, 1, 7, 7), bias) fp32 of RepVGGDW (block.py:3818-3877; CIB's third stage with lk=True): SiLU(conv(x) + conv1(x)), a depthwise
    7x7 and a depthwise 3x3 Conv with BatchNorm each, folded as its fuse() does (:3853-3877) -- each branch folded with its BN, the 3x3
    kernel zero-padded to 7x7, kernels and biases added.  A model that went through fuse() holds the result as conv.weight / conv.bias
    (`conv1` is gone) and is taken as it is; the keys tell the two forms apart, as for fold_repvgg."""
    if prefix + ".conv1.conv.weight" not in sd:
        return _f32(sd[prefix + ".conv.weight"]), _f32(sd[prefix + ".conv.bias"])
    w7, b7 = fold_conv_bn(sd, prefix + ".conv", eps)
    w3, b3 = fold_conv_bn(sd, prefix + ".conv1", eps)
    assert w7.shape[-1] == 7 and w3.shape[-1] == 3 and w7.shape[1] == w3.shape[1] == 1, (prefix, tuple(w7.shape), tuple(w3.shape))
    return w7 + torch.nn.functional.pad(w3, [2, 2, 2, 2]), b7 + b3


_REPVGG_KEY = re.compile(r"\.cv[23]\.0\.m\.\d+\.cv1\.(conv1\.conv|conv)\.weight$")


def repconv_form(sd: Mapping[str, torch.Tensor]) -> str:
    """Which RepConv a model's RepBottlenecks (RepNCSPELAN4.cv2.0 / cv3.0, a RepCSP each) hold, from its state-dict keys: a
    `convmap.weight` -> "refconv" (the fork's own, every yaml-built model); `cv1.conv1.conv.weight`, or after fuse() `cv1.conv.weight`
    under a RepBottleneck -> "repvgg" (upstream's, an upstream-pickled checkpoint).  A model without RepBottlenecks: "refconv", unused."""
    if any(k.endswith(".convmap.weight") for k in sd):
        return "refconv"
    return "repvgg" if any(_REPVGG_KEY.search(k) for k in sd) else "refconv"


# ---- layouts: an op's final fp32 (w, b) -> the tensors the kernels read (on the CPU; callers move or serialise them) ----
def _align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


def _bytes(*parts: torch.Tensor) -> bytes:
    """The tensors' bytes one after the other, each but the last padded to 256 bytes (a record's f32 matrix and its split planes:
    csrc/op_args.h build_conv32 computes the same offsets)."""
    raw = [t.numpy().tobytes() for t in parts]
    return b"".join(x.ljust(_align(len(x)), b"\0") for x in raw[:-1]) + raw[-1]


def packed_dims(cout: int, cin: int, k: int) -> Tuple[int, int]:
    """(CoutPad, Kpad) of the fp16 dense layout, as the library says them (csrc/conv_select.hip bsy_conv_packed_dims)."""
    cp, kp = ctypes.c_int(), ctypes.c_int()
    L.check(L.lib.bsy_conv_packed_dims(cout, cin, k, ctypes.byref(cp), ctypes.byref(kp)))
    return cp.value, kp.value


def dense_f16(w, b=None, once: bool = False):
    """(Cout, Cin, k, k) [+ bias (Cout)] -> fp16 [CoutPad][Kpad], K order (kh, kw, cin), and bias f32 [CoutPad], zero in the padding
    (csrc/conv_gemm.hip).  An image conv (Cin = 3) is packed with a zero 4th input channel, K = (kh, kw, c4) (csrc/image_conv.h).
    The weights go through fp32 whatever they come as; once (the float64 fold of a "world_cls" record alone): float64 is rounded to f16 ONCE."""
    w = _real(w) if once else _f32(w)
    cout, cin, k, _ = w.shape
    cp, kp = packed_dims(cout, cin, k)
    if cin == 3:
        w = torch.cat([w, torch.zeros(cout, 1, k, k, dtype=w.dtype)], 1)
    K = k * k * w.shape[1]
    wp = torch.zeros(cp, kp, dtype=torch.float16)
    wp[:cout, :K] = _to_f16(w.permute(0, 2, 3, 1).reshape(cout, K))
    bp = torch.zeros(cp, dtype=torch.float32)
    if b is not None:
        bp[:cout] = _f32(b)
    return wp, bp


def split_f16_planes(w2d: torch.Tensor):
    """(Cout, K) f32 -> (hi, lo) f16 planes [Cout][K rounded up to 32] with w ~= hi + lo (csrc/conv32x_mfma.hip): hi = f16(w),
    lo = f16(w - hi); the subtraction is exact in f32, so the pair carries w to ~22 bits (less where lo falls into f16's
    subnormal range: |w| < 2^-3 keeps an absolute 2^-25).  Values beyond the f16 range saturate at +-65504 like the kernel's
    pixel split (never an infinity)."""
    cout, K = w2d.shape
    kp = (K + 31) // 32 * 32
    w = torch.zeros(cout, kp, dtype=torch.float32)
    w[:, :K] = w2d
    hi = w.clamp(-65504.0, 65504.0).to(torch.float16)
    lo = (w - hi.float()).clamp(-65504.0, 65504.0).to(torch.float16)
    return hi, lo


def dense_f32(w, b, split: bool = False):
    """(Cout, Cin, k, k) + bias -> ((matrix,) or (matrix, hi, lo), bias): the fp32 correctness mode's f32 [k*k*cin][cout] matrix (K order
    (kh, kw, cin) as in the fp16 layout, cout fastest) and bias f32 [cout], no padding (csrc/ref32.hip); split (fp32x mode) adds the two
    f16 planes of split_f16_planes, which a record carries behind the matrix (_bytes)."""
    w = _f32(w)  # (a float64 fold is rounded here, once)
    cout = w.shape[0]
    mats = (w.permute(2, 3, 1, 0).reshape(-1, cout).contiguous(),)
    if split:
        mats += split_f16_planes(w.permute(0, 2, 3, 1).reshape(cout, -1))
    return mats, _f32(b).contiguous()


def depthwise(w, b):
    """(C, 1, kh, kw) + bias -> f32 [kh*kw][C] and bias f32 [C], in every precision (csrc/elementwise.hip, csrc/bsyolo_ops.hip)."""
    w = _f32(w)
    return w.reshape(w.shape[0], -1).t().contiguous(), _f32(b).contiguous()


# ---- sources: where a record's (w, b) come from in the state dict.  Per source the parameters it reads -- (key, the module's own
# shape, synth_state_dict's draw), in the order they are drawn -- and the reader (sd, r, eps) -> fp32 (w, b) of the module ----
DW_KINDS = ("dw", "dwg", "dwg_plain", "dwg_ext", "repvggdw")


def _he(fan: int):  # He-normal
    return lambda g, shape: torch.randn(*shape, generator=g) * (2.0 / fan) ** 0.5


def _uni(scale: float, shift: float):
    return lambda g, shape: torch.rand(*shape, generator=g) * scale + shift


def _module_dims(r: WRec):
    """The module's own (cout, cin, kh, kw): the record's, or real_cout / real_cin where the op runs wider than the module.  (A "world_cls"
    record's module is the FOLDED conv: text rows x c3.)"""
    co = r.real_cout or (r.cout // 2 if r.kind == "dwg_ext" else r.cout)
    return co, 1 if r.kind in DW_KINDS else (r.real_cin or r.cin), r.k, r.kw or r.k


def _conv_bn_params(prefix: str, co: int, ci: int, kh: int, kw: int):
    """A reference Conv module (conv.py:133-151), un-fused: what fold_conv_bn reads.  Randomised BN statistics."""
    return [(prefix + ".conv.weight", (co, ci, kh, kw), _he(ci * kh * kw)),
            (prefix + ".bn.weight", (co,), _uni(0.6, 0.7)), (prefix + ".bn.bias", (co,), _uni(0.6, -0.3)),
            (prefix + ".bn.running_mean", (co,), _uni(0.6, -0.3)), (prefix + ".bn.running_var", (co,), _uni(1.0, 0.5))]


def _conv2(r):  # two Conv modules on the same input, half the width each, stacked along cout (plan.py conv(name2=...))
    co, ci, kh, kw = _module_dims(r)
    return _conv_bn_params(r.name, co // 2, ci, kh, kw) + _conv_bn_params(r.post, co // 2, ci, kh, kw)


def _read_conv2(sd, r, eps):
    (w, b), (w2, b2) = fold_conv_bn(sd, r.name, eps), fold_conv_bn(sd, r.post, eps)
    return torch.cat([w, w2]), torch.cat([b, b2])


def _bare(r):  # a bare nn.Conv2d / nn.Linear with bias; `post`: a depthwise 1x1 conv after it (MSCAAttention.dilconv, MSCA.py:31)
    co, ci, kh, kw = _module_dims(r)
    post = [(r.post + ".weight", (co, 1, 1, 1), _uni(1.0, 0.5)), (r.post + ".bias", (co,), _uni(0.4, -0.2))] if r.post else []
    return [(r.name + ".weight", (co, ci, kh, kw), _he(ci * kh * kw)), (r.name + ".bias", (co,), _uni(0.4, -0.2))] + post


def _read_bare(sd, r, eps):
    w, b = _f32(sd[r.name + ".weight"]), _f32(sd[r.name + ".bias"])
    if w.dim() == 2:  # nn.Linear (Classify.linear, head.py:294): a 1x1 conv on the (B, 1, 1, cin) map
        w = w[:, :, None, None]
    if r.post:  # y -> a*y + d, folded in
        a, d = _f32(sd[r.post + ".weight"]).view(-1), _f32(sd[r.post + ".bias"])
        w, b = w * a.view(-1, 1, 1, 1), a * b + d
    return w, b


def _deconv(r):  # nn.ConvTranspose2d(c, c, 2, 2, 0) (block.py:91), weight layout (cin, cout, 2, 2); one record per output phase
    return [(r.name + ".weight", (r.cin, r.cout, 2, 2), _he(r.cin)), (r.name + ".bias", (r.cout,), _uni(0.4, -0.2))]


def _read_deconv(sd, r, eps):
    dy, dx = r.tap  # out[2i+dy, 2j+dx] = W[:, :, dy, dx]^T x[i, j] + b, i.e. one 1x1 conv per output phase
    return _f32(sd[r.name + ".weight"])[:, :, dy, dx].permute(1, 0).reshape(r.cout, r.cin, 1, 1), _f32(sd[r.name + ".bias"])


def _refconv(r):  # block.py:793-816: a buffer `weight` and the per-kernel 3x3 map over it
    co, ci, kh, kw = _module_dims(r)
    return [(r.name + ".weight", (co, ci, kh, kw), _he(ci * kh * kw)),
            (r.name + ".convmap.weight", (co * ci, 1, 3, 3), lambda g, shape: torch.randn(*shape, generator=g) * (2.0 / 9) ** 0.5 * 0.25)]


def _repvgg(r):  # conv.py:296-397, un-fused: a 3x3 and a 1x1 Conv + BN
    co, ci, _, _ = _module_dims(r)
    return _conv_bn_params(r.name + ".conv1", co, ci, 3, 3) + _conv_bn_params(r.name + ".conv2", co, ci, 1, 1)


def _repvggdw(r):  # block.py:3818-3877, un-fused: a depthwise 7x7 and a depthwise 3x3 Conv + BN
    co = _module_dims(r)[0]
    return _conv_bn_params(r.name + ".conv", co, 1, 7, 7) + _conv_bn_params(r.name + ".conv1", co, 1, 3, 3)


def _ela(r):  # ELA (nn/Addmodules/ELA.py:36-72): three scalar mixing weights, two Conv1d over k taps, one GroupNorm
    c, k = r.cout, r.k
    return ([(f"{r.name}.{s}", (1,), lambda g, shape: torch.randn(*shape, generator=g)) for s in ("ch_weight", "sp_weight", "res_weight")]
            + [(r.name + ".spatial_conv.weight", (c, 1, k), _he(k)), (r.name + ".ch_att.2.weight", (c, 1, k), _he(k)),
               (r.name + ".gn.weight", (c,), _uni(0.6, 0.7)), (r.name + ".gn.bias", (c,), _uni(0.6, -0.3))])


def _read_ela(sd, r, eps):
    """-> ([spatial_conv (C,k)][ch_att.2 (C,k)][gn.weight][gn.bias] as one vector, no bias); the three scalar mixing weights enter
    the op record as their sigmoids (r.coef)."""
    p = [_f32(sd[key]) for key, _, _ in _ela(r)]
    r.coef = tuple(float(torch.sigmoid(t.view(-1)[0])) for t in p[:3])
    return torch.cat([t.reshape(-1) for t in p[3:]]).contiguous(), None


# ---- YOLO-World: the text features and the two records that fold them in ----
TXT_KEY = "txt_feats"  # reserved state-dict key: WorldModel.txt_feats (nn/tasks.py:611), (nc, E) or (1, nc, E)


def _unit_rows(g, shape):
    return torch.nn.functional.normalize(torch.randn(*shape, generator=g), dim=-1)


def text_rows(sd, r: WRec) -> torch.Tensor:
    """The text features of `sd` as float64 (rows, E) for record `r`: E must be the record's, the rows the plan's text_nc."""
    if TXT_KEY not in sd:
        raise KeyError(f"{r.name}: the state dict has no {TXT_KEY!r} (a YOLO-World graph reads its text features there: (nc, E) or (1, nc, E))")
    t = _f64(sd[TXT_KEY])
    if t.dim() == 3:
        if t.shape[0] != 1:
            raise NotImplementedError(f"{TXT_KEY} of shape {tuple(t.shape)}: per-image text features are not accelerated (one set per call)")
        t = t[0]
    if t.dim() != 2 or t.shape[1] != r.embed:
        raise ValueError(f"{r.name}: {TXT_KEY} of shape {tuple(t.shape)}, the layer takes rows of E = {r.embed}")
    if t.shape[0] != r.cout:
        raise ValueError(f"{r.name}: {TXT_KEY} has {t.shape[0]} rows, the plan was built to score {r.cout} (text_nc)")
    return t


def _maxsig(r):  # MaxSigmoidAttnBlock (block.py:3483-3515) of a C2fAttn: gl = nn.Linear(E, c), bias (nh); cout = text rows, cin = c, k = nh
    return [(r.name + ".gl.weight", (r.cin, r.embed), _he(r.embed)), (r.name + ".gl.bias", (r.cin,), _uni(0.4, -0.2)),
            (r.name + ".bias", (r.k,), _uni(2.0, -1.0)), (TXT_KEY, (r.cout, r.embed), _unit_rows)]


def _read_maxsig(sd, r, eps):
    """-> (G float64 (rows, c), [bias | scale] float64 (2 nh)): G[n] = (gl.weight @ t_n + gl.bias) / sqrt(hc) with t_n the text row AS GIVEN
    (the block does not normalise it; dividing before the maximum is dividing after it); scale = 1 where the module holds the float."""
    t = text_rows(sd, r)
    nh, hc = r.k, r.cin // r.k
    G = (t @ _f64(sd[r.name + ".gl.weight"]).t() + _f64(sd[r.name + ".gl.bias"])) / math.sqrt(hc)
    scale = _f64(sd[r.name + ".scale"]).reshape(-1) if r.name + ".scale" in sd else torch.ones(nh, dtype=torch.float64)
    bias = _f64(sd[r.name + ".bias"]).reshape(-1)
    assert tuple(G.shape) == (r.cout, r.cin) and bias.numel() == nh and scale.numel() == nh, (r.name, tuple(G.shape), bias.numel(), scale.numel())
    return G, torch.cat([bias, scale])


def guide(G: torch.Tensor, f32: bool) -> torch.Tensor:
    """The guide rows as csrc/maxsig.hip reads them: f32 [rows][c] as they are, or f16 with the rows padded to a multiple of 32 by REPEATING
    ROW 0 -- the kernel takes its maximum over whole blocks of 32 rows, and a copy of a real row can never win against the rows themselves
    (a zero row would: every real dot product may be negative)."""
    if f32:
        return _f32(G).contiguous()
    pad = -G.shape[0] % 32
    return _to_f16(torch.cat([G, G[:1].expand(pad, -1)]) if pad else G)


def _world_cls(r):  # WorldDetect's cv3.l.2 = nn.Conv2d(c3, E, 1) and cv4.l = BNContrastiveHead(E) (head.py:314-315; r.post = "<head>.cv4.<l>")
    co, ci = r.embed, r.real_cin or r.cin
    return [(r.name + ".weight", (co, ci, 1, 1), _he(ci)), (r.name + ".bias", (co,), _uni(0.4, -0.2)),
            (r.post + ".norm.weight", (co,), _uni(0.6, 0.7)), (r.post + ".norm.bias", (co,), _uni(0.6, -0.3)),
            (r.post + ".norm.running_mean", (co,), _uni(0.6, -0.3)), (r.post + ".norm.running_var", (co,), _uni(1.0, 0.5)),
            (r.post + ".bias", (1,), lambda g, shape: torch.full(shape, -4.21)), (r.post + ".logit_scale", (), lambda g, shape: torch.full(shape, -1.0)),
            (TXT_KEY, (r.cout, r.embed), _unit_rows)]


def _read_world_cls(sd, r, eps):
    """BNContrastiveHead(cv3.l.2(x), text) (block.py:3609-3631) as ONE biased 1x1 conv c3 -> rows, float64: with a = gamma / sqrt(var + eps),
    b = beta - mean a (the eval-mode BatchNorm), w^ = the unit-normalised text rows and s = exp(logit_scale):
    W' = s w^ diag(a) W3,  b' = s w^ (a o b3 + b) + bias."""
    t = text_rows(sd, r)
    W3, b3 = _f64(sd[r.name + ".weight"]).flatten(1), _f64(sd[r.name + ".bias"])
    g, beta = _f64(sd[r.post + ".norm.weight"]), _f64(sd[r.post + ".norm.bias"])
    mu, var = _f64(sd[r.post + ".norm.running_mean"]), _f64(sd[r.post + ".norm.running_var"])
    a = g / torch.sqrt(var + eps)
    b = beta - mu * a
    wn = torch.nn.functional.normalize(t, dim=-1)
    s = torch.exp(_f64(sd[r.post + ".logit_scale"]).reshape(()))
    W = s * (wn * a) @ W3
    bias = s * (wn @ (a * b3 + b)) + _f64(sd[r.post + ".bias"]).reshape(())
    return W[:, :, None, None], bias


_CONV_BN = (lambda r: _conv_bn_params(r.name, *_module_dims(r)), lambda sd, r, eps: fold_conv_bn(sd, r.name, eps))
_BARE = (_bare, _read_bare)
SOURCES = {"conv": _CONV_BN, "first": _CONV_BN, "first_s2d": _CONV_BN, "dw": _CONV_BN, "dwg": _CONV_BN, "dwg_ext": _CONV_BN,
           "conv2": (_conv2, _read_conv2), "plain": _BARE, "dwg_plain": _BARE, "deconv": (_deconv, _read_deconv),
           "refconv": (_refconv, lambda sd, r, eps: fold_refconv(sd, r.name)),
           "repvgg": (_repvgg, lambda sd, r, eps: fold_repvgg(sd, r.name, eps)),
           "repvggdw": (_repvggdw, lambda sd, r, eps: fold_repvggdw(sd, r.name, eps)), "ela": (_ela, _read_ela),
           "maxsig": (_maxsig, _read_maxsig), "world_cls": (_world_cls, _read_world_cls)}


def record_keys(r: WRec) -> List[str]:
    """The state-dict keys record `r` reads of an un-fused reference model."""
    return [key for key, _, _ in SOURCES[r.kind][0](r)]


# ---- channel step: the module's (w, b) -> the op's ----
def _take(t: torch.Tensor, idx, dim: int = 0) -> torch.Tensor:
    """t's slices idx[0], idx[1], ... along `dim`; zeros where idx[i] < 0."""
    idx = torch.as_tensor(idx, dtype=torch.long)
    assert int(idx.max()) < t.shape[dim], (tuple(t.shape), dim, int(idx.max()))
    return t.index_select(dim, idx.clamp(min=0)).index_fill_(dim, torch.nonzero(idx < 0).view(-1), 0.0)


def op_channels(r: WRec, w: torch.Tensor, b: torch.Tensor):
    """The module's fp32 (w, b) -> the op's (r.cout, r.cin | 1, kh, kw) and (r.cout): which channels are re-laid out or zero."""
    dw = r.kind in DW_KINDS
    shape = (r.cout, 1 if dw else r.cin, r.k, r.kw or r.k)
    if r.rows is not None or r.cols is not None:
        # the op's channels are a re-laid-out, zero-padded copy of the module's (plan.py _pmsfa_padded, T.cmap)
        if r.rows is not None:
            w, b = _take(w, r.rows), _take(b, r.rows)
        if r.cols is not None and not dw:
            w = _take(w, r.cols, 1)
    elif r.real_cout or r.real_cin:
        # the op runs wider than the module (plan.py detect(): widths padded to a multiple of 8): zero weights and biases in the padding
        co, ci = _module_dims(r)[:2]
        assert tuple(w.shape[:2]) == (co, ci), (r.name, tuple(w.shape), (co, ci))
        w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, shape[1] - ci, 0, r.cout - co))
        b = torch.nn.functional.pad(b, (0, r.cout - co))
    if r.kind == "first_s2d":
        # 6x6 stride-2 pad-2 image conv (YOLOv5u's stem, cfg/models/v5/yolov5.yaml:16) = 3x3 stride-1 pad-1 conv over the
        # space-to-depth image [Y][X][(dy, dx, c)] (csrc/elementwise.hip s2d_kernel): input row 2 oy - 2 + kh with kh = 2 a + dy is
        # s2d row oy - 1 + a, so w3[co][(dy, dx, c)][a][b] = w[co][c][2a + dy][2b + dx]; channels 12 .. 15 are zero padding.
        # (Only fp16 plans hold such a record: plan.py conv_first.)
        assert tuple(w.shape) == (r.cout, 3, 6, 6), (r.name, tuple(w.shape))
        shape = (r.cout, 16, 3, 3)
        w3 = torch.zeros(shape)
        for dy in (0, 1):
            for dx in (0, 1):
                w3[:, (dy * 2 + dx) * 3:(dy * 2 + dx) * 3 + 3] = w[:, :, dy::2, dx::2]
        w = w3
    if r.kind == "dwg_ext":
        # PMSFA.conv3 (block.py:3042): a depthwise 7x7 over the first half of its input, extended with an identity
        # kernel (centre tap 1, bias 0, no activation) so the second half passes through untouched
        half = r.cout // 2
        assert tuple(w.shape) == (half,) + shape[1:], (r.name, tuple(w.shape))
        ident = torch.zeros(r.cout - half, *shape[1:])
        ident[:, 0, shape[2] // 2, shape[3] // 2] = 1.0
        w, b = torch.cat([w, ident]), torch.cat([b, torch.zeros(r.cout - half)])
    assert tuple(w.shape) == shape, (r.name, tuple(w.shape), shape)
    if r.perm is not None:  # output-channel permutation (qkv)
        w, b = _take(w, r.perm), _take(b, r.perm)
    return w, b


def pack_record(sd: Mapping[str, torch.Tensor], r: WRec, eps: float = BN_EPS, f32: bool = False, split: bool = False):
    """-> (weight bytes, bias bytes) for one op: source -> channel step -> layout.  f32: dense convs in the fp32 correctness mode's
    layout (dense_f32; split, the fp32x mode: followed by the two f16 planes); depthwise / ELA records are f32 in every mode."""
    w, b = SOURCES[r.kind][1](sd, r, eps)
    if r.kind == "ela":  # one flat f32 vector as it is read, no bias
        return _bytes(w), b""
    if r.kind == "maxsig":  # the guide rows in the storage type, [bias | scale] f32
        return _bytes(guide(w, f32)), _bytes(_f32(b).contiguous())
    w, b = op_channels(r, w, b)
    if r.kind not in DW_KINDS and f32:
        mats, bp = dense_f32(w, b, split)
        return _bytes(*mats), _bytes(bp)
    wp, bp = depthwise(w, b) if r.kind in DW_KINDS else dense_f16(w, b, once=r.kind == "world_cls")
    return _bytes(wp), _bytes(bp)


def pack_plan_weights(plan: Plan, sd: Mapping[str, torch.Tensor], eps: float = BN_EPS) -> bytes:
    """Packs every record of `plan` (sets w_off / b_off on the records) -> host blob (fp32 layouts for an fp32-mode plan)."""
    chunks, off = [], 0
    for r in plan.wrecs.values():
        wb, bb = pack_record(sd, r, eps, f32=getattr(plan, "f32_mode", False), split=getattr(plan, "split_f16", False))
        r.w_off, r.b_off = off, off + _align(len(wb))
        chunks += [wb, b"\0" * (_align(len(wb)) - len(wb)), bb, b"\0" * (_align(len(bb)) - len(bb))]
        off = r.b_off + _align(len(bb))
    return b"".join(chunks)


def adopt_offsets(plan: Plan, packed: Plan) -> None:
    """Copy blob offsets from an already packed plan of the same model (other input shape)."""
    for k, r in plan.wrecs.items():
        src = packed.wrecs[k]
        assert (src.kind, src.cout, src.cin, src.k) == (r.kind, r.cout, r.cin, r.k)
        r.w_off, r.b_off, r.coef = src.w_off, src.b_off, src.coef


def synth_state_dict(plan: Plan, seed: int = 0, cls_gain: float = 0.1, cls_bias: float = -4.21) -> Dict[str, torch.Tensor]:
    """Seeded random parameters for benchmarking without a checkpoint (no weights ship with the reference:
    .MISSING_LARGE_BLOBS): every record's parameters (SOURCES) in the records' order, a module that several records read drawn
    once.  He-normal conv weights, randomised BN statistics.  The class head is damped (cls_gain) and
    shifted (cls_bias) so that a realistic share of anchors passes conf 0.25: the defaults put 1.5 % of the anchors
    of YOLO11s @640 (seed 0) above 0.25 (SURVEY 8d asks for 1-2 %), i.e. ~126 NMS candidates per image."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    for r in plan.wrecs.values():
        for key, shape, draw in SOURCES[r.kind][0](r):
            if key in sd:
                continue
            if r.kind == "plain" and "cv3." in r.name:  # Detect's class branch (v10Detect's one2one_cv3 too): damped weights, a constant bias (nothing drawn)
                sd[key] = draw(g, shape) * cls_gain if key.endswith(".weight") else torch.full(shape, float(cls_bias))
            elif r.kind == "plain" and "cv2." in r.name and key.endswith(".bias"):  # the box branch
                sd[key] = torch.rand(*shape, generator=g) + 0.5
            else:
                sd[key] = draw(g, shape)
    return sd
