"""Classification models (yolo11-cls, yolov8-cls) on the engine: the graph tables, the Classify head in the plan, the tail kernel
(csrc/classify.hip: softmax, logit copy and top-k in one launch), the forward against fixtures made by running the reference
(tests/golden/make_cls_fixtures.py), and the plugin hooks.  The CPU oracle has no Classify: parity is against the fixtures only."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from bs_yolo_amd import lib as L
from bs_yolo_amd.graphs import stock_cfg
from bs_yolo_amd.plan import Plan
from bs_yolo_amd.weights import pack_plan_weights, synth_state_dict
from graph_helpers import fixture, state_dict, x_of

DEV = "cuda:0"
GRAPHS = ["yolo11n_cls", "yolov8n_cls", "yolo11n_cls1000"]
PRECISIONS = ["fp16", "fp32x", "fp32"]
# Largest |x - fixture x| of the fp16 engine over every fixture graph and stored shape, measured on an MI355X and recorded in
# docs/experiments.md ("Classification graphs: first measurement"): yolo11n_cls 1.98e-3, yolov8n_cls 3.95e-4, yolo11n_cls1000 3.502e-3.
# The bound is twice the largest.  The engine is bit-reproducible, so the margin is for fixtures not enumerated here, not for
# run-to-run noise.  The pooled vector takes the same bound (largest measured: 3.92e-3).
FP16_LOGIT_BOUND = 2 * 3.502e-3


def _sd(tag):
    """A copy of the reference's un-fused state dict (no damping rule), for the callers that add or drop keys."""
    return dict(state_dict(tag, None))


def _cfg(meta):
    return stock_cfg(meta["family"], meta["scale"], meta["nc"], "classify")


def _stable_topk(y, k):
    """(indices, values) of the k largest entries per row of y, ties to the lower index: a stable descending sort (on the CPU, in
    fp32 -- exact for f16 values, and the order is the same)."""
    v, i = torch.sort(y.detach().float().cpu(), dim=1, descending=True, stable=True)
    return i[:, :k].to(torch.int32), v[:, :k]


# ---- host side (no GPU) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["yolo11n_cls", "yolov8n_cls"])
def test_stock_cfg_restates_the_reference_yaml(tag):
    _, meta = fixture(tag)
    cfg = _cfg(meta)
    want = meta["yaml"]  # yaml.safe_load of the reference's file, recorded by make_cls_fixtures.py
    assert cfg["backbone"] == want["backbone"] and cfg["scales"] == want["scales"]
    assert cfg["head"] == want["head"] == [[-1, 1, "Classify", ["nc"]]]
    assert cfg["nc"] == meta["nc"] and cfg["scale"] == "n"
    assert not any(m == "SPPF" for _, _, m, _ in cfg["backbone"])  # its own backbone, not detect's with another last line


def test_stock_cfg_classify_families_and_pose():
    for fam in ("yolo11", "yolov8"):
        for scale in "nsmlx":
            cfg = stock_cfg(fam, scale, 10, "classify")
            assert cfg["head"] == [[-1, 1, "Classify", ["nc"]]] and cfg["scale"] == scale and scale in cfg["scales"]
    for fam in ("bsyolo11", "yolov5", "yolov8-p2", "yolov8-p6", "yolov5-p6", "yolov9"):
        with pytest.raises(ValueError):
            stock_cfg(fam, "n" if fam != "yolov9" else "t", 10, "classify")
    for fam in ("yolo11", "yolov8", "yolov5", "yolov9"):
        with pytest.raises(ValueError):
            stock_cfg(fam, "n" if fam != "yolov9" else "t", 10, "pose")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nc", [10, 1000, 3])
@pytest.mark.parametrize("family", ["yolo11", "yolov8"])
def test_classify_plan(family, nc, precision):
    plan = Plan(stock_cfg(family, "n", nc, "classify"), 2, 224, 224, precision=precision)
    kinds = [o["kind"] for o in plan.ops]
    assert kinds.count(L.OP_GAP) == 1 and kinds.count(L.OP_CLASSIFY_TAIL) == 1 and L.OP_DECODE not in kinds
    gap, lin, tail = plan.ops[-3:]
    assert (gap["kind"], lin["kind"], tail["kind"]) == (L.OP_GAP, L.OP_CONV, L.OP_CLASSIFY_TAIL)
    assert (gap["H"], gap["W"], gap["src0"].C) == (7, 7, 1280) and lin["src0"] is gap["dst"] and tail["src0"] is lin["dst"]
    rec = plan.wrecs[lin["wkey"]]
    assert rec.kind == "plain" and rec.cin == 1280 and (rec.real_cout or rec.cout) == nc and rec.cout % 8 == 0
    assert lin["act"] == 0 and lin["out_f32"] == 1 and lin["ksize"] == 1
    assert tail["nc"] == nc and tail["ksize"] == min(nc, 5) and tail["src0"].ld % 4 == 0 and tail["src0"].ld >= nc
    m = plan.meta
    assert m["task"] == "classify" and m["nc"] == nc and m["strides"] == [32.0] and m["nm"] == 0 and m["ne"] == 0
    assert m["A"] == 0 and m["levels"] == [] and m["topk"] == min(nc, 5)
    pack_plan_weights(plan, synth_state_dict(plan))
    arr = plan.c_ops()
    t = [o for o in arr if o.kind == L.OP_CLASSIFY_TAIL]
    assert len(t) == 1 and (t[0].nc, t[0].ksize, t[0].B) == (nc, min(nc, 5), 2)
    ext = lambda v: v.buf - L.BSY_EXT_BASE  # noqa: E731
    assert (ext(t[0].dst), ext(t[0].res), ext(t[0].box[0]), ext(t[0].cls[0])) == (1, 2, 3, 4)
    assert t[0].src0.buf == tail["src0"].buf and t[0].src0.ld == tail["src0"].ld
    assert t[0].prec == {"fp16": 0, "fp32": 1, "fp32x": 2}[precision]


@pytest.mark.parametrize("tag", GRAPHS)
def test_classify_weights_pack_from_the_reference_state_dict(tag):
    _, meta = fixture(tag)
    sd = _sd(tag)
    seen = set()

    class Recording(dict):
        def __getitem__(self, k):
            seen.add(k)
            return dict.__getitem__(self, k)

    for precision in PRECISIONS:
        plan = Plan(_cfg(meta), 1, 64, 64, precision=precision)
        pack_plan_weights(plan, Recording(sd))  # a missing key raises KeyError
    head = f"model.{len(meta['yaml']['backbone'])}"
    assert {head + ".linear.weight", head + ".linear.bias", head + ".conv.conv.weight"} <= seen
    assert set(sd) == seen  # every parameter and buffer the reference model holds is consumed
    assert tuple(sd[head + ".linear.weight"].shape) == (meta["nc"], 1280)


def test_classify_graph_support_and_stride():
    from bs_yolo_amd.plugin import SUPPORTED_HEADS, graph_support, max_stride
    assert "Classify" in SUPPORTED_HEADS
    for fam in ("yolo11", "yolov8"):
        cfg = stock_cfg(fam, "n", 10, "classify")
        assert graph_support(cfg) == {"fp16": True, "fp32": True} and max_stride(cfg) == 32


def test_classify_head_arguments():
    cfg = stock_cfg("yolo11", "n", 10, "classify")
    cfg["head"][-1] = [-1, 1, "Classify", ["nc", 1, 1]]  # the defaults spelt out
    assert Plan(cfg, 1, 64, 64).meta["task"] == "classify"
    cfg["head"][-1] = [-1, 1, "Classify", ["nc", 3]]
    with pytest.raises(NotImplementedError):
        Plan(cfg, 1, 64, 64)
    cfg["head"][-1] = [[-1, 8], 1, "Classify", ["nc"]]  # fed by a list (head.py:297-298)
    with pytest.raises(NotImplementedError):
        Plan(cfg, 1, 64, 64)
    resnet = {"nc": 10, "backbone": [[-1, 1, "ResNetLayer", [3, 64, 1, True, 1]]], "head": [[-1, 1, "Classify", ["nc"]]]}
    with pytest.raises(NotImplementedError):  # yolov8-cls-resnet50.yaml stays on the reference
        Plan(resnet, 1, 64, 64)


def test_classify_tail_is_declared_and_checks_its_arguments():
    header = (ROOT / "include" / "bsyolo.h").read_text()
    assert "bsy_classify_tail(" in header and "BSY_OP_CLASSIFY_TAIL = 23" in header
    assert "bsy_classify_tail" in L.SYMBOLS and L.OP_CLASSIFY_TAIL == 23
    f = L.lib.bsy_classify_tail
    d = C.c_void_p(64)  # never dereferenced: every check below fails before a launch
    with pytest.raises(L.BsyError, match="null pointer"):
        L.check(f(None, 12, 1, 10, None, None, L.BSY_F32, 0, None, None, None))
    with pytest.raises(L.BsyError, match="null pointer"):
        L.check(f(d, 12, 1, 10, None, d, L.BSY_F32, 0, None, None, None))
    with pytest.raises(L.BsyError, match="without top-k outputs"):
        L.check(f(d, 12, 1, 10, d, d, L.BSY_F32, 5, None, d, None))
    for nc in (0, 65537):
        with pytest.raises(L.BsyError, match="nc %d out of range" % nc):
            L.check(f(d, 65540, 1, nc, d, d, L.BSY_F32, 0, None, None, None))
    with pytest.raises(L.BsyError, match="k 4 out of range"):  # k > nc
        L.check(f(d, 4, 1, 3, d, d, L.BSY_F32, 4, d, d, None))
    with pytest.raises(L.BsyError, match="k 17 out of range"):
        L.check(f(d, 100, 1, 100, d, d, L.BSY_F32, 17, d, d, None))
    with pytest.raises(L.BsyError, match="k -1 out of range"):
        L.check(f(d, 100, 1, 100, d, d, L.BSY_F32, -1, d, d, None))
    with pytest.raises(L.BsyError, match="ld 10 must be a multiple of 4"):
        L.check(f(d, 10, 1, 10, d, d, L.BSY_F32, 0, None, None, None))
    with pytest.raises(L.BsyError, match="ld 8 must be"):  # ld < nc
        L.check(f(d, 8, 1, 10, d, d, L.BSY_F32, 0, None, None, None))
    for B in (0, 65536):
        with pytest.raises(L.BsyError, match="B %d out of range" % B):
            L.check(f(d, 12, B, 10, d, d, L.BSY_F32, 0, None, None, None))
    with pytest.raises(L.BsyError, match="dtype 2 unsupported"):
        L.check(f(d, 12, 1, 10, d, d, L.BSY_U8, 0, None, None, None))
    with pytest.raises(L.BsyError, match="misaligned"):
        L.check(f(C.c_void_p(72), 12, 1, 10, d, d, L.BSY_F32, 0, None, None, None))  # logits: 16 bytes
    with pytest.raises(L.BsyError, match="misaligned"):
        L.check(f(d, 12, 1, 10, C.c_void_p(66), d, L.BSY_F32, 0, None, None, None))  # y: 4 bytes for f32


class ClassificationValidator:
    """What install_val_metrics reads of a ClassificationValidator (models/yolo/classify/val.py:36-60)."""

    def __init__(self, nc):
        self.names = {i: str(i) for i in range(nc)}
        self.pred, self.targets, self.orig_calls = [], [], 0

    def update_metrics(self, preds, batch):  # val.py:56-60
        self.orig_calls += 1
        n5 = min(len(self.names), 5)
        self.pred.append(preds.argsort(1, descending=True)[:, :n5].type(torch.int32).cpu())
        self.targets.append(batch["cls"].type(torch.int32).cpu())


@pytest.mark.parametrize("nc", [3, 10])
def test_install_val_metrics_on_a_classification_validator(nc, monkeypatch):
    from bs_yolo_amd import plugin
    v = plugin.install_val_metrics(ClassificationValidator(nc))
    with pytest.raises(TypeError):
        plugin.install_val_metrics(object())  # neither kind of validator
    k = min(nc, 5)
    g = torch.Generator().manual_seed(nc)
    preds = torch.rand(4, nc, generator=g).softmax(1)
    batch = {"cls": torch.tensor([0.0, 1.0, 2.0, 1.0])}
    v.update_metrics(preds, batch)  # a CPU tensor: the original method
    assert v.orig_calls == 1 and len(v.pred) == 1
    # the y of an accelerated model: a device tensor that carries the launch's own top-k rows (recorded here: distinct from argsort's)
    rows = torch.arange(k, dtype=torch.int64).flip(0).repeat(4, 1)
    preds._bsy_topk = rows
    v.update_metrics(preds, batch)  # still on the CPU: the original
    assert v.orig_calls == 2
    monkeypatch.setattr(plugin, "_on_device", lambda t: True)
    v.update_metrics(preds, batch)
    assert v.orig_calls == 2 and len(v.pred) == 3 and len(v.targets) == 3
    got = v.pred[-1]
    assert got.dtype == torch.int32 and got.device.type == "cpu" and tuple(got.shape) == (4, k) and torch.equal(got, rows.int())
    assert torch.equal(v.targets[-1], torch.tensor([0, 1, 2, 1], dtype=torch.int32)) and v.targets[-1].dtype == torch.int32
    preds._bsy_topk = rows[:, :1] if k > 1 else rows.repeat(1, 2)  # rows of another shape than (B, min(nc, 5)): not this model's
    v.update_metrics(preds, batch)
    assert v.orig_calls == 3
    del preds._bsy_topk
    v.update_metrics(preds, batch)  # a device tensor of another origin: the original
    assert v.orig_calls == 4


# ---- device: the kernel alone ----------------------------------------------------------------------------------------------
CASES = [(1, 1, 4), (3, 2, 4), (2, 10, 12), (5, 1000, 1000), (2, 1003, 1004), (1, 20000, 20000), (1, 65536, 65536)]


def _logits(B, nc, ld):
    """B seeded rows and three hand-made ones (all equal; +-80 mixed; exact duplicates), (B + 3, ld) with zeros past nc."""
    g = torch.Generator().manual_seed(1000 * B + nc)
    rows = torch.randn(B + 3, nc, generator=g) * 3.0
    rows[B] = 1.25
    rows[B + 1] = torch.where(torch.rand(nc, generator=g) < 0.5, 80.0, -80.0)
    rows[B + 1, 0] = 80.0
    dup = torch.randint(-4, 5, (nc,), generator=g).float() * 0.5  # nine distinct values: duplicates from nc = 10 on, all over above
    rows[B + 2] = dup
    out = torch.zeros(B + 3, ld)
    out[:, :nc] = rows
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("B,nc,ld", CASES)
def test_classify_tail_kernel(B, nc, ld):
    from bs_yolo_amd import ops as O
    lg = _logits(B, nc, ld)
    ref = torch.softmax(lg[:, :nc].double(), 1)
    dev = lg.to(DEV)
    inf = lg.clone()
    inf[:, nc:] = float("inf")
    inf = inf.to(DEV)
    y32 = None
    for dt in (torch.float32, torch.float16):
        for k in sorted({1, min(nc, 5), min(nc, 16)}):
            y, x, idx, val = O.classify_tail(dev, nc, k, dt)
            yi, xi, idxi, vali = O.classify_tail(inf, nc, k, dt)  # +inf in the padding columns changes nothing
            torch.cuda.synchronize()
            assert y.dtype == dt and x.dtype == dt and tuple(y.shape) == (B + 3, nc) and tuple(x.shape) == (B + 3, nc)
            assert idx.dtype == torch.int32 and val.dtype == torch.float32 and tuple(idx.shape) == (B + 3, k) == tuple(val.shape)
            assert torch.equal(y, yi) and torch.equal(x, xi) and torch.equal(idx, idxi) and torch.equal(val, vali)
            yc = y.cpu()
            if dt == torch.float32:
                err = float((yc.double() - ref).abs().max())
                print(f"B={B} nc={nc} f32: max |y - softmax64| = {err:.3e}")
                assert err <= 1e-6, (B, nc, err)
                assert bool((yc[B] == yc[B, 0]).all()) and abs(float(yc[B, 0]) - 1.0 / nc) <= 1e-6  # equal logits: 1 / nc
                assert bool(torch.isfinite(yc).all())
                if y32 is None:
                    y32 = yc
                assert torch.equal(yc, y32)  # k changes nothing about y
            else:
                ulp = torch.from_numpy(np.spacing(np.abs(y32.numpy()).astype(np.float16)).astype(np.float32))
                d = (yc.float() - y32).abs()
                assert bool((d <= ulp).all()), (B, nc, float((d / ulp).max()))
            assert torch.equal(x.cpu(), lg[:, :nc].to(dt))  # the logits in the output dtype, bit for bit
            wi, wv = _stable_topk(y, k)
            assert torch.equal(idx.cpu(), wi), (B, nc, str(dt), k)
            assert torch.equal(val.cpu(), wv), (B, nc, str(dt), k)
    y, x, idx, val = O.classify_tail(dev, nc, 0, torch.float32)  # k = 0: no rows
    torch.cuda.synchronize()
    assert idx is None and val is None and torch.equal(y.cpu(), y32)


@pytest.mark.gpu
def test_classify_tail_ranks_nan_first():
    from bs_yolo_amd import ops as O
    lg = torch.zeros(2, 12)
    lg[0, :10] = torch.arange(10.0)
    lg[1, :10] = torch.arange(10.0)
    lg[1, 3] = float("nan")  # a NaN logit: the whole row of y is NaN, as torch's softmax gives; equal keys go to the lower class
    y, x, idx, val = O.classify_tail(lg.to(DEV), 10, 5, torch.float32)
    torch.cuda.synchronize()
    assert idx[0].tolist() == [9, 8, 7, 6, 5] and bool(torch.isnan(y[1]).all()) and bool(torch.isnan(val[1]).all())
    assert idx[1].tolist() == [0, 1, 2, 3, 4]
    assert torch.equal(torch.isnan(x.cpu()), torch.isnan(lg[:, :10]))


# ---- device: the forward ---------------------------------------------------------------------------------------------------
def _engine(tag, precision, **kw):
    from bs_yolo_amd.engine import YoloEngine
    _, meta = fixture(tag)
    return YoloEngine(_cfg(meta), _sd(tag), precision=precision, bn_eps=meta["bn_eps"], **kw)  # 1e-5, not DetectionModel's 1e-3


def _input(tag, si, precision):
    x = x_of(fixture(tag)[1], si)
    return (x.half() if precision == "fp16" else x).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", GRAPHS)
def test_classify_graph_matches_reference(tag, precision):
    """fp32x / fp32: the project's 1e-3 on y and on the logits (O(1) on these fixtures), and the fixture's own top-k order (its
    smallest top-5 logit gap is 3e-3).  fp16: the project's 1e-2 on y; FP16_LOGIT_BOUND on the logits; the top-k against a stable sort
    of the engine's own y (fp16 error is not small against the fixtures' gaps)."""
    z, meta = fixture(tag)
    eng = _engine(tag, precision)
    nc, k = meta["nc"], min(meta["nc"], 5)
    assert eng.task == "classify" and eng.max_stride == 32 and eng.nc == nc
    for si, (b, h, w) in enumerate(meta["shapes"]):
        xin = _input(tag, si, precision)
        y, x = eng(xin)
        idx, val = eng.last_topk
        torch.cuda.synchronize()
        assert tuple(y.shape) == (b, nc) == tuple(x.shape) and y.dtype == xin.dtype == x.dtype
        assert tuple(idx.shape) == (b, k) == tuple(val.shape) and idx.dtype == torch.int32 and val.dtype == torch.float32
        ey = float(np.abs(y.float().cpu().numpy() - z[f"y{si}"]).max())
        ex = float(np.abs(x.float().cpu().numpy() - z[f"x{si}"]).max())
        print(f"{tag} {precision} shape {si}: max |dy| = {ey:.3e}  max |dx| = {ex:.3e}")
        wi, wv = _stable_topk(y, k)
        assert torch.equal(idx.cpu(), wi) and torch.equal(val.cpu(), wv), (tag, precision, si)
        if precision == "fp16":
            assert ey < 1e-2, (tag, si, ey)
            assert ex <= FP16_LOGIT_BOUND, (tag, si, ex)
        else:
            assert ey <= 1e-3 and ex <= 1e-3, (tag, precision, si, ey, ex)
            fi, _ = _stable_topk(torch.from_numpy(z[f"y{si}"]), k)
            assert torch.equal(idx.cpu(), fi), (tag, precision, si, idx.cpu().tolist(), fi.tolist())
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", GRAPHS)
def test_classify_pooled_vector_and_guards(tag, precision, monkeypatch):
    """The (B, 1280) mean behind OP_GAP, read back from the plan's buffer, against the reference's (a forward hook on Classify.pool),
    under the logits' bound of the mode.  The plan runs in a private workspace with guard bands: no op of it stores out of bounds."""
    monkeypatch.setenv("BSY_PLAN_GUARD", "4096")
    z, meta = fixture(tag)
    eng = _engine(tag, precision, autotune=False)
    for si, (b, h, w) in enumerate(meta["shapes"]):
        xin = _input(tag, si, precision)
        eng(xin)
        plan, hnd = eng.plan_for(b, h, w, xin.dtype, xin.dtype)
        pooled = eng.read_view(plan, hnd, plan.pooled).reshape(b, 1280).numpy()
        ep = float(np.abs(pooled - z[f"pool{si}"]).max())
        print(f"{tag} {precision} shape {si}: max |dpool| = {ep:.3e}")
        assert ep <= (FP16_LOGIT_BOUND if precision == "fp16" else 1e-3), (tag, precision, si, ep)
    assert eng.check_guards() == []
    eng.close()


@pytest.mark.gpu
def test_classify_forward_is_reproducible(monkeypatch):
    tag = "yolo11n_cls"
    xin = _input(tag, 1, "fp16")  # (2, 96, 128)
    tuned, plain = _engine(tag, "fp16", autotune=True), _engine(tag, "fp16", autotune=False)
    y, x = (t.clone() for t in tuned(xin))
    top = tuple(t.clone() for t in tuned.last_topk)
    y2, x2 = plain(xin)
    torch.cuda.synchronize()
    assert tuned.tune_stats["autotune_calls"] == 1 and plain.tune_stats["autotune_calls"] == 0
    assert torch.equal(y, y2) and torch.equal(x, x2) and all(torch.equal(a, b) for a, b in zip(top, plain.last_topk))
    # a batch of 2 equals its two images run singly
    for i in range(2):
        yi, xi = plain(xin[i:i + 1].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(yi[0], y[i]) and torch.equal(xi[0], x[i]) and torch.equal(plain.last_topk[0][0], top[0][i])
    # without the logits, and in chunks (the large-batch path)
    yn, xn = plain(xin, want_raw=False)
    torch.cuda.synchronize()
    assert xn is None and torch.equal(yn, y)
    monkeypatch.setattr(plain, "_max_view_elems", lambda H, W: (1 << 31) // 2)
    yc, xc = plain(xin)
    torch.cuda.synchronize()
    assert torch.equal(yc, y) and torch.equal(xc, x) and all(torch.equal(a, b) for a, b in zip(top, plain.last_topk))
    ya, xa = plain(xin, augment=True)  # the reference augments DetectionModel only (tasks.py:356-358): the plain forward
    torch.cuda.synchronize()
    assert torch.equal(ya, y) and torch.equal(xa, x)
    tuned.close()
    plain.close()
    # eager == graph replay
    graph = _engine(tag, "fp16", autotune=False, graph=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        outs = []
        for _ in range(4):  # ring of 3: the fourth forward replays the first slot's graph
            yg, xg = graph(xin)
            outs.append((yg.clone(), xg.clone(), graph.last_topk[0].clone(), graph.last_topk[1].clone()))
    s.synchronize()
    torch.cuda.synchronize()
    assert graph.graph_stats["captures"] >= 1 and graph.graph_stats["replays"] >= 1, graph.graph_stats
    for yg, xg, ig, vg in outs:
        assert torch.equal(yg, y) and torch.equal(xg, x) and torch.equal(ig, top[0]) and torch.equal(vg, top[1])
    graph.close()


# ---- device: the plugin ----------------------------------------------------------------------------------------------------
class ClassificationModel(torch.nn.Module):
    """Stand-in for the reference's ClassificationModel: `.yaml`, the reference's parameter names with the fixture's values -- every
    `bn` a real BatchNorm2d with the model's eps (1e-5: accelerate reads it off the modules, plugin.model_bn_eps) --, and an original
    forward that only counts its calls and returns a sentinel (the engine must not reach it)."""

    def __init__(self, tag):
        super().__init__()
        meta = fixture(tag)[1]
        self.yaml = _cfg(meta)
        for name, t in _sd(tag).items():
            mod = self
            *path, leaf = name.split(".")
            for p in path:
                if not hasattr(mod, p):
                    mod.add_module(p, torch.nn.BatchNorm2d(t.numel(), eps=meta["bn_eps"]) if p == "bn" else torch.nn.Module())
                mod = getattr(mod, p)
            if isinstance(mod, torch.nn.BatchNorm2d):
                with torch.no_grad():
                    getattr(mod, leaf).copy_(t)
            else:
                mod.register_parameter(leaf, torch.nn.Parameter(t.clone(), requires_grad=False))
        self.calls = 0
        self.eval()

    def forward(self, x, *args, **kwargs):
        self.calls += 1
        return "original"


@pytest.mark.gpu
def test_accelerate_classification_model_and_validator_hook():
    from bs_yolo_amd import plugin
    tag = "yolo11n_cls"
    z, meta = fixture(tag)
    m = ClassificationModel(tag).to(DEV)
    assert plugin.accelerate(m) is m
    x = x_of(meta, 1).to(DEV)
    y, lg = m(x)  # fp32 input: the fp32x engine
    torch.cuda.synchronize()
    assert m.calls == 0 and m._bsy_state["fp32_calls"] == 1
    assert y.dtype == torch.float32 and tuple(y.shape) == (2, 10) == tuple(lg.shape)
    assert np.abs(y.cpu().numpy() - z["y1"]).max() <= 1e-3 and np.abs(lg.cpu().numpy() - z["x1"]).max() <= 1e-3
    yh, lh = m(x.half())  # fp16 input: the fp16 engine
    torch.cuda.synchronize()
    assert m.calls == 0 and yh.dtype == torch.float16 and np.abs(yh.float().cpu().numpy() - z["y1"]).max() < 1e-2
    # the validator takes the launch's own top-k rows
    v = plugin.install_val_metrics(ClassificationValidator(10))
    v.update_metrics(y, {"cls": torch.tensor([3.0, 7.0], device=DEV)})
    assert v.orig_calls == 0 and torch.equal(v.pred[0], _stable_topk(y, 5)[0]) and v.pred[0].dtype == torch.int32
    assert torch.equal(v.pred[0], _stable_topk(torch.from_numpy(z["y1"]), 5)[0])  # = the reference's argsort on its own y
    assert torch.equal(v.targets[0], torch.tensor([3, 7], dtype=torch.int32))
    v.update_metrics(y.clone(), {"cls": torch.tensor([3.0, 7.0], device=DEV)})  # a tensor without the rows: the original
    assert v.orig_calls == 1 and torch.equal(v.pred[1], v.pred[0])
    # what stays on the original forward
    n = 0
    m.train(); assert m(x) == "original"; n += 1; m.eval()
    assert m(x, augment=True) == "original"; n += 1
    assert m(torch.rand(1, 3, 100, 100, device=DEV)) == "original"; n += 1  # any size is legal for this task; multiples of 32 run here
    assert m(x.cpu()) == "original"; n += 1
    for kw in (dict(visualize=True), dict(embed=[1]), dict(profile=True)):
        assert m(x, **kw) == "original"; n += 1
    head = list(m.model.children())[-1]
    head.export = True  # Classify.export: y alone (head.py:304)
    assert m(x) == "original"; n += 1
    head.export = False
    assert m.calls == n and m._bsy_state["fallbacks"] == n
    y3, _ = m(x)
    assert m.calls == n and torch.equal(y3, y)
    plugin.restore(m)
    assert not hasattr(m, "_bsy_state") and m(x) == "original" and m.calls == n + 1
