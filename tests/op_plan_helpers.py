"""Shared pieces of the one-op plan tests (test_glue_ops.py): a single bsy_op run through bsy_plan_create / bsy_plan_run with every
tensor bound as an external slot, poisoned views and a weight-blob builder.  Not a test module."""
import ctypes as C

import numpy as np
import torch

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
    from bs_yolo_amd import lib as L
    blob = bytes(blob) + b"\0" * max(0, 256 - len(blob))
    eng, plan = C.c_void_p(), C.c_void_p()
    L.check(L.lib.bsy_engine_create(0, C.byref(eng)))
    try:
        L.check(L.lib.bsy_engine_load_weights(eng, (C.c_char * len(blob)).from_buffer_copy(blob), len(blob)))
        L.check(L.lib.bsy_plan_create(eng, (L.Op * 1)(op), 1, None, 0, C.byref(plan)))
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


def ulp(v, mant, floor_exp):
    """Unit in the last place of |v| (float64 array) in a format of `mant` stored mantissa bits, floored at 2^floor_exp (the subnormal spacing)."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(a)
    return np.where(a == 0, 2.0 ** floor_exp, np.maximum(np.ldexp(1.0, e - 1 - mant), 2.0 ** floor_exp))


def ulp16(v):
    return ulp(v, 10, -24)


def ulp32(v):
    return ulp(v, 23, -149)
