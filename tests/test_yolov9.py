"""YOLOv9 (GELAN) detect and segment graphs on the engine: the graph family, the pooling front end of AConv / ADown
(csrc/pool_down.hip, bsy_pool_down), the plan lowering of RepNCSPELAN4 / ELAN1 / AConv / ADown / SPPELAN in all three precisions,
the two RepConv weight folds, the arena, the C ABI and plugin.accelerate -- against fixtures made by running the reference
(tests/golden/make_v9_fixtures.py: yolov9c, yolov9c-seg, yolov9m, yolov9t with the fork's own RepConv, yolov9t with upstream's).

Synthetic head scores are far below the score tolerance here (max ~0.005 - 0.01), so the raw level maps (the logits) carry the
engine-against-reference check; every fixture's meta["ref_fp16"] records how far the reference's own fp16 run is from its fp32 run."""
import ctypes as C
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from bs_yolo_amd import lib as L
from bs_yolo_amd.graphs import stock_cfg
from bs_yolo_amd.plan import Plan
from bs_yolo_amd.weights import fold_refconv, fold_repvgg, pack_plan_weights, repconv_form, synth_state_dict
from graph_helpers import RawBounds, RefModel, YBounds, all_equal, cfg_of, check_nms, check_raw, check_y, engine, fixture, outputs, state_dict, x_of
from op_plan_helpers import DEV

NC = 12
GRAPHS = ["yolov9c", "yolov9c_seg", "yolov9m", "yolov9t", "yolov9t_repvgg"]
SHAPES = [(1, 64, 64), (2, 96, 128)]
ANCHORS = [84, 252]
SIZES = [("t", "detect"), ("s", "detect"), ("c", "detect"), ("c", "segment")]
# RepNCSPELAN4 / ELAN1 arguments [c2, c3, c4] of layer 4 (cfg/models/v9/*.yaml), for the cv4 check
L4 = {"t": (64, 64, 32), "s": (128, 128, 64), "m": (240, 240, 120), "c": (512, 256, 128)}
# The bounds test_p2p6.py applies, over the whole of a three-level map.  fp16: score < 1e-2, box < 1 px; fp32x / fp32: 1e-3, 1e-3 * imgsz.
Y_BOUNDS = YBounds(score16=1e-2, p999_16=None, box16=1.0, score32=1e-3, box32=1e-3)
# Raw maps, mask coefficients, prototypes.  fp16: 2e-2 of the map's maximum; fp32x / fp32: 1e-3 * max(1, maximum).
MAP_BOUNDS = RawBounds(rel16=2e-2, strict16=True, floor16=False, rel32=1e-3)


def _damped(name, suffixes):
    return re.search(r"\.m\.\d+\.", name) is not None and any(name.endswith(s) for s in suffixes)


def _damp(name, meta):
    """The rule the generator wrote into meta["damp"] (make_v9_fixtures.py: the tensors that feed the residual gain, times one factor)."""
    return meta["damp"]["factor"] if _damped(name, meta["damp"]["suffixes"]) else 1.0


def _sd_of(tag):
    return state_dict(tag, _damp)


# ---- host side (no GPU) ------------------------------------------------------------------------------------------------
def test_family_table():
    for s, task in SIZES + [("m", "detect")]:
        cfg = stock_cfg("yolov9", s, NC, task)
        assert "scales" not in cfg and cfg["nc"] == NC and cfg["head"][-1][2] == ("Detect" if task == "detect" else "Segment")
        assert cfg["head"][-1][0] == [15, 18, 21] and len(cfg["backbone"]) == 10 and len(cfg["head"]) == 13
    assert stock_cfg("yolov9", "c", NC, "segment")["head"][-1][3] == ["nc", 32, 256]
    for s, task in (("t", "segment"), ("s", "segment"), ("m", "segment"), ("e", "detect"), ("n", "detect"), ("c", "obb"), ("c", "pose")):
        with pytest.raises(ValueError):
            stock_cfg("yolov9", s, NC, task)
    down = {s: {l[2] for l in stock_cfg("yolov9", s, NC)["backbone"] + stock_cfg("yolov9", s, NC)["head"]} for s in "tsmc"}
    assert "ADown" in down["c"] and "AConv" not in down["c"] and all("AConv" in down[s] and "ADown" not in down[s] for s in "tsm")
    assert "ELAN1" in down["t"] and "ELAN1" in down["s"] and "ELAN1" not in down["m"] and "ELAN1" not in down["c"]
    assert stock_cfg("yolo11", "n")["scales"]  # the other families keep their table


@pytest.mark.parametrize("precision", ["fp16", "fp32x", "fp32"])
@pytest.mark.parametrize("size,task", SIZES)
def test_v9_plans(size, task, precision):
    cfg = stock_cfg("yolov9", size, NC, task)
    for (b, h, w), A in zip(SHAPES, ANCHORS):
        plan = Plan(cfg, b, h, w, precision=precision)
        m = plan.meta
        assert m["strides"] == [8.0, 16.0, 32.0] and m["A"] == A and m["levels"] == [(h // s, w // s) for s in (8, 16, 32)]
        assert m["legacy"] and m["nm"] == (32 if task == "segment" else 0)
        pools = [o for o in plan.ops if o["kind"] == L.OP_POOL_DOWN]
        modes = sorted(o["level"] for o in pools)
        if size == "c":  # five ADown blocks: one launch per half
            assert modes == [0] * 5 + [1] * 5
            for a, mx in zip(pools[0::2], pools[1::2]):
                assert (a["level"], mx["level"]) == (0, 1) and a["src0"].buf == mx["src0"].buf and a["src0"].C == mx["src0"].C
                assert a["src0"].coff == 0 and mx["src0"].coff == a["src0"].C and a["src0"].ld == 2 * a["src0"].C
                assert (a["OH"], a["OW"]) == (a["H"], a["W"]) and (mx["OH"], mx["OW"]) == (mx["H"] // 2, mx["W"] // 2)
        else:  # five AConv blocks: one launch over all channels
            assert modes == [0] * 5 and all(o["src0"].coff == 0 and o["src0"].C == o["src0"].ld for o in pools)
        for o in pools:
            assert o["dst"].C == o["src0"].C and o["dst"].buf != o["src0"].buf and o["H"] % 2 == 0 and o["W"] % 2 == 0
            assert set(plan.op_buffers(o)) == {o["src0"].buf, o["dst"].buf}
        assert sum(o["kind"] == L.OP_SPPF_POOL for o in plan.ops) == 1 and not any(o["kind"] == L.OP_BNECK for o in plan.ops)
        c2, c3, c4 = L4[size]
        cv4 = [o for o in plan.ops if o["name"] == "model.4.cv4"]
        assert len(cv4) == 1 and cv4[0]["src0"].C + (cv4[0]["src1"].C if cv4[0]["src1"] else 0) == c3 + 2 * c4 and cv4[0]["dst"].C == c2
        pack_plan_weights(plan, synth_state_dict(plan))
        ops = plan.c_ops()
        assert [o.level for o in ops if o.kind == L.OP_POOL_DOWN] == [o["level"] for o in pools]


@pytest.mark.parametrize("size,header", [("t", 7.7), ("s", 26.4), ("m", 77.9), ("c", 102.1)])
def test_conv_flops_at_640(size, header):
    """Dense-conv FLOPs of the plan at 1 x 640 x 640, nc = 80, within 1 % of the count of the reference's own convs
    (make_v9_fixtures.py conv_gflops_640, stored in every fixture's meta).  The yaml headers (7.7 / 26.4 / 77.9 / 102.1) come from
    another counter: the reference's convs give 8.23 / 26.89 / 76.82 / 102.65, so only c is within 1 % of its header.  yolov9m's
    fp16 plan carries its 180- and 90-channel pieces on 184 and 96 (zero weights in the padding) and so multiplies 1.8 % more:
    it is counted in the fp32 plan, which has no padding."""
    want = fixture("yolov9t")[1]["ref_conv_gflops_640"][size]
    for precision in ("fp32",) if size == "m" else ("fp16", "fp32"):
        plan = Plan(stock_cfg("yolov9", size, 80), 1, 640, 640, precision=precision)
        got = sum(o.get("mfma_flops", 0) for o in plan.ops) / 1e9
        print(size, precision, f"plan {got:.4f} reference convs {want:.4f} header {header}")
        assert abs(got - want) <= 0.01 * want
    if size == "c":
        assert abs(got - header) <= 0.01 * header


def test_what_is_refused_and_yolov9m():
    from bs_yolo_amd.plugin import graph_support, max_stride
    # yolov9e's layers (cfg/models/v9/yolov9e.yaml: an Identity in front, CBLinear taps, CBFuse merges)
    e = stock_cfg("yolov9", "c", NC)
    e["backbone"] = e["backbone"][:3] + [[1, 1, "CBLinear", [[64]]], [[3, -1], 1, "CBFuse", [[0]]]] + e["backbone"][3:]
    f = stock_cfg("yolov9", "c", NC)
    f["backbone"] = [[-1, 1, "nn.Identity", []]] + f["backbone"]
    for cfg in (e, f):
        for precision in ("fp16", "fp32x", "fp32"):
            with pytest.raises(NotImplementedError):
                Plan(cfg, 1, 64, 64, precision=precision)
        assert graph_support(cfg) == {"fp16": False, "fp32": False}
        with pytest.raises(NotImplementedError):
            max_stride(cfg)
    k7 = stock_cfg("yolov9", "t", NC)
    k7["backbone"][9] = [-1, 1, "SPPELAN", [128, 64, 7]]
    with pytest.raises(NotImplementedError):
        Plan(k7, 1, 64, 64)
    with pytest.raises(NotImplementedError):  # 72 / 8 = 9: an odd map in front of the second AConv
        Plan(stock_cfg("yolov9", "t", NC), 1, 72, 72)
    with pytest.raises(ValueError):
        Plan(stock_cfg("yolov9", "t", NC), 1, 64, 64, repconv="upstream")
    for s, task in SIZES:
        assert graph_support(stock_cfg("yolov9", s, NC, task)) == {"fp16": True, "fp32": True}
        assert max_stride(stock_cfg("yolov9", s, NC, task)) == 32
    # yolov9m: 184-channel AConv, chunks of 180, RepCSP hidden widths 60 / 90 -- plans (padded pieces on the fp16 path) or raises
    # NotImplementedError from Plan; graph_support says whichever holds
    m = stock_cfg("yolov9", "m", NC)
    built = {}
    for precision in ("fp16", "fp32"):
        try:
            plan = Plan(m, 2, 96, 128, precision=precision)
            built[precision] = True
            assert plan.meta["A"] == 252 and sum(o["kind"] == L.OP_POOL_DOWN for o in plan.ops) == 5
            assert any(o["kind"] == L.OP_POOL_DOWN and o["src0"].C == 240 for o in plan.ops)
            assert any(o["name"] == "model.16.cv1" and o["dst"].C == 184 for o in plan.ops)
        except NotImplementedError as err:
            built[precision] = False
            assert re.search(r"\d+", str(err)), err  # names the width that stops it
    assert graph_support(m) == built


@pytest.mark.parametrize("tag", GRAPHS)
def test_weights_pack_from_the_reference_state_dict(tag):
    _, meta = fixture(tag)
    sd = _sd_of(tag)
    assert repconv_form(sd) == meta["repconv"]
    seen = set()

    class Recording(dict):
        def __getitem__(self, k):
            seen.add(k)
            return dict.__getitem__(self, k)

    for precision in ("fp16", "fp32x"):
        plan = Plan(cfg_of(meta), 1, 64, 64, precision=precision, repconv=meta["repconv"])
        pack_plan_weights(plan, Recording(sd))
        kinds = {r.kind for r in plan.wrecs.values()}
        assert meta["repconv"] in kinds and ({"refconv", "repvgg"} - {meta["repconv"]}).isdisjoint(kinds)
        assert set(synth_state_dict(plan)) == {n for n in sd if not n.endswith(".dfl.conv.weight")}  # the keys of the plan's form
    assert {n for n in sd if n not in seen and not n.endswith("num_batches_tracked")} == {n for n in sd if n.endswith(".dfl.conv.weight")}
    gone = dict(sd)
    del gone[next(n for n in sd if _damped(n, meta["damp"]["suffixes"]))]
    with pytest.raises(KeyError):
        pack_plan_weights(Plan(cfg_of(meta), 1, 64, 64, repconv=meta["repconv"]), gone)
    other = "repvgg" if meta["repconv"] == "refconv" else "refconv"
    with pytest.raises(KeyError):  # the other form's keys are not in this model
        pack_plan_weights(Plan(cfg_of(meta), 1, 64, 64, repconv=other), sd)


def test_refconv_fold():
    """weights.py "refconv" against this test's fp64 restatement of the fork's RepConv.forward (block.py:813-815)."""
    sd = _sd_of("yolov9t")
    names = [n[:-len(".convmap.weight")] for n in sd if n.endswith(".convmap.weight")]
    assert len(names) == 7 * 2 * 3  # seven RepNCSPELAN4 blocks, two RepCSPs each, n = 3
    for p in names:
        w, cm = sd[p + ".weight"].double(), sd[p + ".convmap.weight"].double()
        co, ci = w.shape[:2]
        want = w + F.conv2d(w.view(1, co * ci, 3, 3), cm, stride=1, padding=1, groups=co * ci).view(co, ci, 3, 3)
        got, bias = fold_refconv(sd, p)
        assert got.dtype == torch.float32 and tuple(got.shape) == (co, ci, 3, 3) and torch.equal(bias, torch.zeros(co))
        assert float((got.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


def test_repvgg_fold():
    """weights.py "repvgg" from un-fused keys against the fold from keys fused by this test's fp64 restatement of
    RepConv.get_equivalent_kernel_bias / _fuse_bn_tensor (conv.py:328-369)."""
    _, meta = fixture("yolov9t_repvgg")
    sd = _sd_of("yolov9t_repvgg")
    names = [n[:-len(".conv1.conv.weight")] for n in sd if n.endswith(".cv1.conv1.conv.weight")]
    assert len(names) == 7 * 2 * 3
    eps = 1e-3

    def branch(p):
        k = sd[p + ".conv.weight"].double()
        std = (sd[p + ".bn.running_var"].double() + eps).sqrt()
        t = (sd[p + ".bn.weight"].double() / std).reshape(-1, 1, 1, 1)
        return k * t, sd[p + ".bn.bias"].double() - sd[p + ".bn.running_mean"].double() * sd[p + ".bn.weight"].double() / std

    fused = {}
    for p in names:
        (k3, b3), (k1, b1) = branch(p + ".conv1"), branch(p + ".conv2")
        fused[p + ".conv.weight"], fused[p + ".conv.bias"] = (k3 + F.pad(k1, [1, 1, 1, 1])).float(), (b3 + b1).float()
    assert repconv_form(fused) == "repvgg" and repconv_form(sd) == "repvgg" and repconv_form({}) == "refconv"
    for p in names:
        (w, b), (wf, bf) = fold_repvgg(sd, p, eps), fold_repvgg(fused, p, eps)
        assert torch.equal(wf, fused[p + ".conv.weight"]) and torch.equal(bf, fused[p + ".conv.bias"])  # taken as they are
        assert float((w - wf).abs().max()) <= 1e-6 * float(wf.abs().max()) and float((b - bf).abs().max()) <= 1e-6 * float(bf.abs().max())
    # a whole fused model packs through the same records
    full = {n: t for n, t in sd.items() if ".cv1.conv1." not in n and ".cv1.conv2." not in n}
    full.update(fused)
    a, b = (Plan(cfg_of(meta), 1, 64, 64, repconv="repvgg") for _ in range(2))
    blob_u, blob_f = pack_plan_weights(a, sd), pack_plan_weights(b, full)
    assert len(blob_u) == len(blob_f)
    for key, r in a.wrecs.items():
        if r.kind == "repvgg":
            n = (r.b_off - r.w_off) // 2
            wu = np.frombuffer(blob_u, dtype=np.float16, count=n, offset=r.w_off).astype(np.float32)
            wf = np.frombuffer(blob_f, dtype=np.float16, count=n, offset=b.wrecs[key].w_off).astype(np.float32)
            assert np.abs(wu - wf).max() <= 2.0 ** -10 * max(np.abs(wf).max(), 1e-30)  # one f16 ulp of the largest weight


@pytest.mark.parametrize("tag", ["yolov9c", "yolov9c_seg", "yolov9t", "yolov9t_repvgg"])
def test_arena_keeps_live_buffers_apart(tag, monkeypatch):
    """No op writes into a buffer that is still live: any two buffers whose lifetimes meet have disjoint address ranges, and every op's
    buffers (the pool-down ops' source and destination among them) are alive at that op."""
    monkeypatch.delenv("BSY_LANES", raising=False)
    _, meta = fixture(tag)
    for precision in ("fp16", "fp32"):
        plan = Plan(cfg_of(meta), 2, 96, 128, precision=precision, repconv=meta["repconv"])
        offs, top = plan.assign_offsets()
        life = plan.buffer_lifetimes()
        size = [(b + 255) & ~255 for b in plan.buf_bytes]
        assert top < sum(size)  # buffers are shared at all
        for i, o in enumerate(plan.ops):
            bufs = plan.op_buffers(o)
            assert all(life[b][0] <= i <= life[b][1] for b in bufs)
            if o["kind"] == L.OP_POOL_DOWN:
                s, d = o["src0"].buf, o["dst"].buf
                assert s in bufs and d in bufs and (offs[s] + size[s] <= offs[d] or offs[d] + size[d] <= offs[s])
        used = [b for b in range(len(size)) if life[b] is not None and size[b]]
        for a in used:
            for b in used:
                if a < b and not (life[a][1] < life[b][0] or life[b][1] < life[a][0]):
                    assert offs[a] + size[a] <= offs[b] or offs[b] + size[b] <= offs[a], (tag, precision, a, b)


def test_abi():
    header = (ROOT / "include" / "bsyolo.h").read_text()
    assert re.search(r"int\s+bsy_pool_down\s*\(", header) and re.search(r"BSY_OP_POOL_DOWN\s*=\s*22\b", header)
    assert "bsy_pool_down" in L.SYMBOLS and hasattr(L.lib, "bsy_pool_down") and L.OP_POOL_DOWN == 22 and L.OP_CHAIN == 21
    assert L.lib.bsy_sizeof_op() == C.sizeof(L.Op) == 624


# ---- device ---------------------------------------------------------------------------------------------------------------
POOL_CASES = [(1, 2, 2, 8), (1, 2, 8, 8), (3, 4, 6, 24), (2, 16, 16, 64), (1, 40, 40, 256)]
SENTINEL = 777.0


def _pool_ref(x, mode):
    """torch on the CPU, NCHW in, NHWC out: mode 0 the averaged map inside an H x W map of zeros, mode 1 the stride-2 max of it."""
    a = F.avg_pool2d(x, 2, 1, 0, False, True)
    if mode:
        return F.max_pool2d(a, 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    out = torch.zeros_like(x)
    out[:, :, :-1, :-1] = a
    return out.permute(0, 2, 3, 1).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("case", POOL_CASES)
def test_pool_down_matches_torch(case, dtype):
    from bs_yolo_amd import ops as O
    B, H, W, Cc = case
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W * 10 + Cc)
    inputs = {"mixed": (torch.randn(B, Cc, H, W, generator=g) * 3).to(dtype),
              "negative": (-torch.rand(B, Cc, H, W, generator=g) - 0.5).to(dtype)}  # a max that sees mode 0's zero border returns 0
    for what, x in inputs.items():
        nhwc = x.permute(0, 2, 3, 1).contiguous()
        for mode in (0, 1):
            want = _pool_ref(x, mode)
            # contiguous tensors
            out = torch.full(want.shape, SENTINEL, dtype=dtype, device=DEV)
            got = O.pool_down_nhwc(nhwc.to(DEV), mode, out=out)
            assert got is out and torch.equal(got.cpu(), want), (case, dtype, what, mode, "contiguous")
            # a channel slice of a wider buffer on both sides: coff != 0, ld > C; the rest of the buffers keeps its bytes
            lds, soff, ldd, doff = Cc + 16, 8, Cc + 24, 16
            src = torch.full((B, H, W, lds), SENTINEL, dtype=dtype)
            src[..., soff:soff + Cc] = nhwc
            dst = torch.full(tuple(want.shape[:3]) + (ldd,), SENTINEL, dtype=dtype, device=DEV)
            dsrc = src.to(DEV)
            O.pool_down_nhwc(dsrc, mode, C=Cc, coff=soff, out=dst, out_coff=doff)
            d = dst.cpu()
            assert torch.equal(d[..., doff:doff + Cc], want), (case, dtype, what, mode, "slice")
            assert bool((d[..., :doff] == SENTINEL).all()) and bool((d[..., doff + Cc:] == SENTINEL).all()) and torch.equal(dsrc.cpu(), src)
    # fresh output of the wrapper's own
    assert torch.equal(O.pool_down_nhwc(nhwc.to(DEV), 1).cpu(), _pool_ref(x, 1))


@pytest.mark.gpu
def test_pool_down_refuses_bad_arguments():
    x = torch.zeros(1, 4, 4, 16, dtype=torch.float16, device=DEV)
    y = torch.full((1, 4, 4, 16), SENTINEL, dtype=torch.float16, device=DEV)
    s = L.stream_ptr(x.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    f = L.lib.bsy_pool_down
    assert f(p(x), 16, 0, p(y), 16, 0, 1, 4, 4, 16, 0, L.BSY_F16, s) == 0
    bad = [
        f(p(x), 16, 0, p(y), 16, 0, 1, 3, 4, 16, 0, L.BSY_F16, s),    # odd H
        f(p(x), 16, 0, p(y), 16, 0, 1, 4, 5, 16, 1, L.BSY_F16, s),    # odd W
        f(p(x), 16, 0, p(y), 16, 0, 1, 0, 4, 16, 0, L.BSY_F16, s),    # H < 2
        f(p(x), 16, 0, p(y), 16, 0, 1, 4, 4, 12, 0, L.BSY_F16, s),    # C not a multiple of 8 (fp16)
        f(p(x), 16, 0, p(y), 16, 0, 1, 4, 4, 6, 0, L.BSY_F32, s),     # C not a multiple of 4 (fp32)
        f(p(x), 16, 4, p(y), 16, 0, 1, 4, 4, 8, 0, L.BSY_F16, s),     # misaligned source offset
        f(p(x), 16, 0, p(y), 12, 0, 1, 4, 4, 8, 0, L.BSY_F16, s),     # misaligned destination stride
        f(p(x), 16, 8, p(y), 16, 0, 1, 4, 4, 16, 0, L.BSY_F16, s),    # the view runs past its row
        f(None, 16, 0, p(y), 16, 0, 1, 4, 4, 16, 0, L.BSY_F16, s),    # null pointers
        f(p(x), 16, 0, None, 16, 0, 1, 4, 4, 16, 0, L.BSY_F16, s),
        f(p(x), 16, 0, p(y), 16, 0, 1, 4, 4, 16, 2, L.BSY_F16, s),    # no such mode
        f(p(x), 16, 0, p(y), 16, 0, 1, 4, 4, 16, 0, L.BSY_U8, s),     # no such storage
    ]
    assert bad == [-1] * len(bad) and b"pool_down" in L.lib.bsy_last_error()
    torch.cuda.synchronize()
    y[...] = SENTINEL
    for args in ((1, 3, 4, 16, 0), (1, 4, 4, 12, 0)):
        assert f(p(x), 16, 0, p(y), 16, 0, *args, L.BSY_F16, s) == -1
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())  # nothing was launched


def _engine(tag, precision, **kw):
    return engine(tag, precision, _damp, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp16", "fp32x", "fp32"])
@pytest.mark.parametrize("tag", GRAPHS)
def test_v9_graph_matches_reference(tag, precision):
    """y, the raw maps of every level (the logits: synthetic scores are below the score tolerance), mc and proto of the segment graph,
    and NMS at the fixture's conf.  NMS: on the fixture's own y the device NMS returns the fixture's rows (count, 1e-5, as
    test_p2p6.py); on the engine's y it is the oracle's NMS of that same y bit for bit; and in the fp32-storage modes, whose y is
    within 1e-3 / 1e-3 * imgsz of the reference's, the rows it keeps are the fixture's: the same count, the same classes, boxes and
    scores within those bounds (the scores nearest the threshold are 8e-6 away from it, the modes' score error here is below 1e-6)."""
    z, meta = fixture(tag)
    assert meta["repconv"] == ("repvgg" if tag.endswith("repvgg") else "refconv")
    eng = _engine(tag, precision)
    assert eng.repconv == meta["repconv"]
    seg = meta["task"] == "segment"
    kept = 0
    for si, (b, h, w) in enumerate(meta["shapes"]):
        x = x_of(meta, si)
        y, aux = eng((x.half() if precision == "fp16" else x).to(DEV))
        raws = aux[0] if seg else aux
        torch.cuda.synchronize()
        levels = [(h // int(s), w // int(s)) for s in meta["stride"]]
        assert tuple(y.shape) == (b, 4 + NC + (32 if seg else 0), sum(lh * lw for lh, lw in levels)) and len(raws) == 3
        assert [tuple(r.shape) for r in raws] == [(b, 64 + NC, lh, lw) for lh, lw in levels]
        yr = y.float().cpu().numpy()
        assert np.isfinite(yr).all()
        check_y(yr, z[f"y{si}"], None, None, max(h, w), precision, f"{tag} shape {si}", NC, Y_BOUNDS)
        assert si in meta["raw_shapes"]
        for l, r in enumerate(raws):
            check_raw(r.float().cpu().numpy(), z[f"raw{si}_{l}"], precision, f"{tag} shape {si} raw {l}", MAP_BOUNDS)
        if seg:
            assert torch.equal(aux[1], y[:, 4 + NC:])
            check_raw(yr[:, 4 + NC:], z[f"mc{si}"], precision, f"{tag} shape {si} mc", MAP_BOUNDS)
            check_raw(aux[2].float().cpu().numpy(), z[f"proto{si}"], precision, f"{tag} shape {si} proto", MAP_BOUNDS)
        kept += check_nms(z, meta, si, y, b, h, w, precision, NC, seg=seg, what=tag)
    assert kept > 0
    eng.close()


SWITCHES = {"untuned": dict(autotune=False), "fuse_bneck_off": dict(autotune=False, fuse_bneck=False), "fuse_head_off": dict(autotune=False, fuse_head=False)}


@pytest.mark.gpu
@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("tag", ["yolov9t", "yolov9t_repvgg"])
def test_fusion_switches_are_not_a_different_answer(tag, switch):
    """Tuned and untuned, fuse_bneck on and off, fuse_head on and off: the same bits (torch.equal), in both RepConv forms.  With
    fuse_head off a Detect plan's decode launch sums the DFL in the fused epilogue's order (plan.py detect(), bsy_op.act), so the
    switch returns the fused head's bits at three levels as it does at four."""
    _, meta = fixture(tag)
    base, other = _engine(tag, "fp16"), _engine(tag, "fp16", **SWITCHES[switch])
    outs = [outputs(e, meta, torch.float16) for e in (base, other)]
    for b, h, w in meta["shapes"]:
        p0, p1 = (e.plan_for(b, h, w, torch.float16, torch.float16)[0] for e in (base, other))
        assert [sum(o["kind"] == L.OP_DECODE for o in p.ops) for p in (p0, p1)] == [0, int(switch == "fuse_head_off")]
        assert all(sum(o["kind"] == L.OP_POOL_DOWN for o in p.ops) == 5 for p in (p0, p1))
    assert all(len(o) == 1 + 3 for o in outs[0] + outs[1])
    same = all_equal(outs[0], outs[1], f"{tag} {switch}")
    assert base.tuning(*meta["shapes"][1]) and not other.tuning(*meta["shapes"][1])
    base.close()
    other.close()
    assert same, (tag, switch)


def convmap_buffer(name, leaf, sd):
    """RefModel's buffer rule of the v9 graphs: the fork's RepConv keeps its kernel in a buffer."""
    return leaf == "weight" and name + ".convmap.weight" in sd


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["yolov9t", "yolov9t_repvgg"])
def test_accelerate_a_v9_model(tag):
    from bs_yolo_amd import plugin
    z, meta = fixture(tag)
    m = RefModel(cfg_of(meta), _sd_of(tag), buffer=convmap_buffer).to(DEV)
    plugin.accelerate(m)
    x = x_of(meta, 1)
    y, raws = m(x.to(DEV))  # fp32 input: the fp32x engine
    st = m._bsy_state
    assert m.calls == 0 and len(raws) == 3 and st["fp32_calls"] == 1 and st["rebuilds"] == 1 and st["repconv"] == meta["repconv"]
    assert st["engine32"].repconv == meta["repconv"] and st["support"] == {"fp16": True, "fp32": True}
    check_y(y.cpu().numpy(), z["y1"], None, None, max(x.shape[2:]), "fp32x", f"accelerate {tag} fp32x", NC, Y_BOUNDS)
    for l, r in enumerate(raws):
        check_raw(r.cpu().numpy(), z[f"raw1_{l}"], "fp32x", f"accelerate {tag} raw {l}", MAP_BOUNDS)
    y16, raws16 = m(x.half().to(DEV))  # fp16 input: the product path
    assert st["engine_calls"] == 1 and st["rebuilds"] == 2 and st["engine"].repconv == meta["repconv"]
    check_y(y16.float().cpu().numpy(), z["y1"], None, None, max(x.shape[2:]), "fp16", f"accelerate {tag} fp16", NC, Y_BOUNDS)
    for l, r in enumerate(raws16):
        check_raw(r.float().cpu().numpy(), z[f"raw1_{l}"], "fp16", f"accelerate {tag} fp16 raw {l}", MAP_BOUNDS)
    # a weight change (in place, as an EMA update or load_state_dict's copy_ makes it): the engines are rebuilt, in the same form
    with torch.no_grad():
        m.get_submodule("model.22.cv3.0.2").bias.add_(1.0)  # the class bias of level 0
    y2, _ = m(x.to(DEV))
    assert st["rebuilds"] == 3 and st["repconv"] == meta["repconv"] and st["engine32"].repconv == meta["repconv"] and m.calls == 0
    lvl0 = (x.shape[2] // 8) * (x.shape[3] // 8)
    assert not torch.equal(y2[:, 4:, :lvl0], y[:, 4:, :lvl0]) and torch.equal(y2[:, :4], y[:, :4]) and torch.equal(y2[:, 4:, lvl0:], y[:, 4:, lvl0:])
    plugin.restore(m)


def test_accelerate_refuses_yolov9e_layers():
    from bs_yolo_amd import plugin
    _, meta = fixture("yolov9c")
    cfg = cfg_of(meta)
    cfg["backbone"] = [[-1, 1, "nn.Identity", []]] + cfg["backbone"][:3] + [[1, 1, "CBLinear", [[64]]]] + cfg["backbone"][3:]
    m = RefModel(cfg, {"model.0.conv.weight": torch.zeros(64, 3, 3, 3)}, buffer=convmap_buffer)
    with pytest.raises(NotImplementedError):
        plugin.accelerate(m)
    assert not hasattr(m, "_bsy_state") and m(torch.zeros(1, 3, 64, 64)) == "original"
