"""The fp16 attention kernel in its two forms (keys resident in LDS / streamed in 128-key chunks) and Attention.pe folded into its
epilogue (csrc/attention.hip): against fp32 softmax attention, fused against unfused bit for bit, and through the engine."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bs_yolo_amd import lib as L  # noqa: F401  (fails loudly when the .so is missing)
    from bs_yolo_amd import ops as O
    from bs_yolo_amd.engine import YoloEngine
    from bs_yolo_amd.graphs import stock_cfg

DEV = "cuda:0"
RESIDENT, STREAMING = 1, 2


def _res_rows(kd, hd):
    """Keys the resident form holds (mirror of attn_res_rows in csrc/attention.hip)."""
    return min(512, (128 * 1024 // ((kd + 8 + hd) * 2)) & ~31)


def _fits(N, kd, hd):
    return (N + 31) // 32 * 32 <= _res_rows(kd, hd)


@functools.lru_cache(maxsize=None)
def _case(B, heads, N, kd, hd, kind="randn"):
    """(qkv (B, 1, N, ld) fp16 on the device, fp32 reference (B, N, heads * hd)), computed once per case."""
    g = torch.Generator().manual_seed(7 + N)
    q = torch.randn(B, heads, kd, N, generator=g)
    k = torch.randn(B, heads, kd, N, generator=g)
    v = torch.randn(B, heads, hd, N, generator=g)
    if kind == "peaky":  # logits 64 times as wide: nearly one-hot rows, the running maximum moves by tens per tile
        q, k = q * 8, k * 8
    elif kind == "first":  # every query's largest logit belongs to key 3: the maximum never moves after the first tile
        q = q.abs()
        k[:, :, :, 3] = 3.0
    q, k, v = q.half().float(), k.half().float(), v.half().float()
    scale = kd ** -0.5
    attn = ((q.transpose(-2, -1) @ k) * scale).softmax(-1)      # block.py:4284-4285
    ref = (v @ attn.transpose(-2, -1)).reshape(B, heads * hd, N).transpose(1, 2).contiguous()
    qkv = torch.cat((q.reshape(B, heads * kd, N), k.reshape(B, heads * kd, N), v.reshape(B, heads * hd, N)), 1)
    return qkv.transpose(1, 2).contiguous().half().reshape(B, 1, N, -1).to(DEV), ref


def _run(qkv, heads, kd, hd, impl=0, **kw):
    out = O.attention_pe_nhwc(qkv, heads, kd, hd, kd ** -0.5, impl=impl, **kw)
    torch.cuda.synchronize()
    return out


def _check(B, heads, N, kd, hd, impl, kind="randn"):
    qkv, ref = _case(B, heads, N, kd, hd, kind)
    got = _run(qkv, heads, kd, hd, impl).float().cpu().reshape(B, N, heads * hd)
    err = (got - ref).abs().max().item()
    print(f"attention B={B} heads={heads} N={N} {kd}/{hd} impl={impl} {kind}: max abs err {err:.3e}")
    # P is rounded to fp16 before the PV product (like any fp16 attention): 2^-11 relative on the weights
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=3e-3, atol=3e-3)


SHAPES = [(2, 2, 100, 32, 64), (1, 4, 400, 32, 64), (1, 1, 9, 16, 128), (1, 2, 37, 32, 64), (2, 1, 100, 48, 96), (1, 2, 33, 48, 64)]
EDGES = [(1, 2, n, 32, 64) for n in (31, 32, 33, 127, 129, 417)]


@pytest.mark.parametrize("impl", [0, STREAMING])
@pytest.mark.parametrize("B,heads,N,kd,hd", SHAPES + EDGES)
def test_attention_matches_fp32_softmax(B, heads, N, kd, hd, impl):
    assert _fits(N, kd, hd)  # impl 0 is the resident form for every one of these
    _check(B, heads, N, kd, hd, impl)


@pytest.mark.parametrize("impl", [0, STREAMING])
def test_attention_streaming_1600_tokens(impl):
    assert not _fits(1600, 32, 64)  # a 40 x 40 map (1280 input) does not fit: impl 0 streams
    _check(1, 1, 1600, 32, 64, impl)


def test_resident_form_refuses_what_does_not_fit():
    qkv, _ = _case(1, 1, 1600, 32, 64)
    with pytest.raises(RuntimeError):
        O.attention_pe_nhwc(qkv, 1, 32, 64, 32 ** -0.5, impl=RESIDENT)


@pytest.mark.parametrize("impl", [RESIDENT, STREAMING])
@pytest.mark.parametrize("kind", ["peaky", "first"])
@pytest.mark.parametrize("N", [100, 400])
def test_attention_peaky_logits_and_rescale_skip(N, kind, impl):
    _check(1, 2, N, 32, 64, impl, kind)


@pytest.mark.parametrize("impl", [RESIDENT, STREAMING])
def test_attention_is_deterministic(impl):
    qkv, _ = _case(1, 4, 400, 32, 64)
    assert torch.equal(_run(qkv, 4, 32, 64, impl), _run(qkv, 4, 32, 64, impl))


def test_query_split_returns_the_unsplit_bits():
    """One image of four heads: its query blocks are dealt to several workgroups per head.  The same image as the first of 64:
    one workgroup per head.  Each query's arithmetic is the same."""
    qkv, _ = _case(1, 4, 400, 32, 64)
    alone = _run(qkv, 4, 32, 64, RESIDENT)
    many = _run(qkv.expand(64, -1, -1, -1).contiguous(), 4, 32, 64, RESIDENT)
    assert torch.equal(many[:1], alone)
    assert torch.equal(many[63:], alone)


# ---- pe in the epilogue: the bits of attention followed by the depthwise launch ------------------------------------------------
MAPS = [(3, 5), (1, 7), (7, 13), (20, 20), (40, 40)]


@pytest.mark.parametrize("kd,hd", [(32, 64), (16, 32), (64, 128)])
@pytest.mark.parametrize("H,W", MAPS)
def test_fused_pe_equals_attention_then_dwconv(H, W, kd, hd):
    B, N = 2, H * W
    for heads in (1, 2, 4):
        C = heads * hd
        g = torch.Generator().manual_seed(H * 100 + W + heads)
        qkv = torch.randn(B, H, W, heads * (2 * kd + hd), generator=g).half().to(DEV)
        w = torch.randn(C, 1, 3, 3, generator=g) * 0.3
        b = torch.randn(C, generator=g)
        v = qkv[..., 2 * heads * kd:].contiguous()
        forms = [STREAMING] + ([RESIDENT] if _fits(N, kd, hd) else [])
        for impl in forms + [0]:
            att = _run(qkv, heads, kd, hd, impl)
            want = O.dwconv3x3_nhwc(v, w, b, act=False, res=att)
            # into a buffer wider than heads * hd: the other columns keep their poison
            wide = torch.full((B, H, W, C + 24), 777.0, dtype=torch.float16, device=DEV)
            got = _run(qkv, heads, kd, hd, impl, pe_w=w, pe_b=b, out=wide, out_coff=8)
            assert got is wide
            assert torch.equal(wide[..., 8:8 + C], want), (heads, impl, (wide[..., 8:8 + C].float() - want.float()).abs().max().item())
            assert bool((wide[..., :8] == 777.0).all()) and bool((wide[..., 8 + C:] == 777.0).all())
            assert torch.equal(_run(qkv, heads, kd, hd, impl, pe_w=w, pe_b=b), want)


# ---- engine -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ["s", "n"])
def test_engine_fused_attn_pe_returns_the_unfused_bits(scale, monkeypatch):
    from bs_yolo_amd.plan import Plan
    from bs_yolo_amd.weights import synth_state_dict
    monkeypatch.setenv("BSY_PLAN_GUARD", "4096")  # guard bands behind every workspace buffer (test_engine_no_out_of_bounds_stores)
    cfg = stock_cfg("yolo11", scale, 80, "detect")
    sd = synth_state_dict(Plan(cfg, 1, 64, 64), seed=0)
    fused = YoloEngine(cfg, sd, autotune=False, fuse_attn_pe=True)
    plain = YoloEngine(cfg, sd, autotune=False, fuse_attn_pe=False)
    for S in (64, 320):  # P5 maps of 2 x 2 (N = 4) and 10 x 10
        x = torch.rand(3, 3, S, S, generator=torch.Generator().manual_seed(S)).half().to(DEV)
        yf, rf = fused(x)
        yp, rp = plain(x)
        torch.cuda.synchronize()
        assert torch.equal(yf, yp)
        assert len(rf) == len(rp) == 3
        for a, b in zip(rf, rp):
            assert torch.equal(a, b)
        pf, _ = fused.plan_for(3, S, S, x.dtype, x.dtype)
        pp, _ = plain.plan_for(3, S, S, x.dtype, x.dtype)
        assert len(pf.ops) == len(pp.ops) - 1
        assert [o["name"] for o in pf.ops if o["name"].endswith("attn+pe")] == ["model.10.m.0.attn+pe"]
        assert not any(o["name"].endswith(".attn.pe") for o in pf.ops)
    assert fused.check_guards() == [] and plain.check_guards() == []
    fused.close()
    plain.close()
