"""Test-time augmentation (augment=True, nn/tasks.py:354-391) on the engine: bs_yolo_amd/tta.py's geometry, the two HIP kernels of
csrc/tta.hip against torch on the device, the engine's TTA forward against the reference's (tests/golden/tta.npz, written by
tests/golden/make_tta_fixtures.py from the reference's own DetectionModel(x, augment=True)), and the plugin's routing."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

from bs_yolo_amd import tta as T
from bs_yolo_amd.graphs import stock_cfg
from bs_yolo_amd.plan import Plan
from oracle import yolo_ref as R

if torch.cuda.is_available():
    from bs_yolo_amd import letterbox as HLB
    from bs_yolo_amd import nms as HN
    from bs_yolo_amd import ops as O
    from bs_yolo_amd import plugin
    from bs_yolo_amd.engine import YoloEngine

DEV = "cuda:0"


def _fixture():
    z = np.load(GOLDEN / "tta.npz")
    return z, json.loads(str(z["meta"]))


def _case_input(case):
    """The graph case's x, regenerated from its seed (the fixture keeps its checksum, not the pixels)."""
    xs = case["x"]
    return torch.rand(*xs["shape"], generator=torch.Generator().manual_seed(xs["seed"]))


def test_fixture_inputs_regenerate_from_their_seeds():
    _, meta = _fixture()
    for case in meta["cases"].values():
        x = _case_input(case)
        assert x.flatten()[:8].tolist() == case["x"]["x_first"]
        assert abs(float(x.double().sum()) - case["x"]["x_sum"]) <= 1e-9 * case["x"]["x_sum"]


# ---- 1. geometry (no GPU) ------------------------------------------------------------------------------------------------------
def test_geometry_matches_the_reference_tables():
    """Pass sizes, kept windows and total anchors of tta.geometry (windows from the plans' detection levels) equal what the reference's
    scale_img / _clip_augmented produced, and the level-based windows equal the reference's own g = sum 4**k formula."""
    _, meta = _fixture()
    assert [float(s) for s in meta["scales"]] == [float(s) for s in T.SCALES] and meta["flips"] == list(T.FLIPS)
    cfg = stock_cfg("yolo11", "n")
    levels = lambda h, w: Plan(cfg, 1, h, w).meta["levels"]  # noqa: E731
    for key, g in meta["geometry"].items():
        h, w = map(int, key.split("x"))
        passes = T.geometry(h, w, 32, levels)
        assert [list(p.padded) for p in passes] == g["padded"], key
        assert [list(p.size) for p in passes] == g["resized"], key
        assert [list(p.window) for p in passes] == g["windows"], key
        assert sum(e - b for b, e in (p.window for p in passes)) == g["total"], key
        anchors = [sum(lh * lw for lh, lw in levels(*p.padded)) for p in passes]
        assert anchors == g["anchors"], key
        assert T.reference_windows(anchors, 3) == [tuple(p.window) for p in passes], key
    assert meta["geometry"]["640x640"]["total"] == 8000 + 6069 + 980
    assert meta["geometry"]["640x480"]["total"] == 6000 + 4641 + 770


# ---- 2. bsy_scale_img vs torch on the device --------------------------------------------------------------------------------------
def _ulp16(t):
    a = t.abs().half()
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).float()


SCALE_CASES = [  # (B, H, W, ratio, flip, gs)
    (1, 640, 640, 0.83, 3, 32), (2, 640, 480, 0.67, None, 32), (3, 96, 160, 0.83, None, 32), (1, 480, 640, 0.83, 3, 32),
    (2, 128, 192, 0.67, 3, 32), (1, 64, 96, 0.83, 2, 32), (2, 97, 131, 0.83, 3, 1), (1, 50, 77, 0.67, None, 1), (3, 33, 45, 1.0, 3, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("case", SCALE_CASES)
def test_scale_img_matches_torch_on_the_device(case, dtype):
    B, H, W, r, flip, gs = case
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(H * W + B)).to(DEV, dtype)
    got = O.scale_img(x, r, flip, gs)
    (oh, ow), (ph, pw) = T.scaled_size(H, W, r, gs)
    xr = x.flip(flip) if flip else x
    ref = F.pad(F.interpolate(xr, size=(oh, ow), mode="bilinear", align_corners=False) if r != 1.0 else xr, [0, pw - ow, 0, ph - oh],
                value=0.447)
    torch.cuda.synchronize()
    assert got.shape == ref.shape and got.dtype == dtype
    assert torch.equal(got[:, :, oh:], ref[:, :, oh:]) and torch.equal(got[..., ow:], ref[..., ow:])  # the pad
    d = (got.float() - ref.float()).abs()
    if dtype == torch.float32:
        assert d.max().item() <= 2.4e-7, d.max().item()
    else:
        assert bool((d <= _ulp16(ref)).all()), d.max().item()
    print(f"scale_img {case} {dtype}: max |d| {d.max().item():.3g}, bit-identical {torch.equal(got, ref)}")


# ---- 3. bsy_tta_merge vs the reference's _descale_pred / _clip_augmented / cat restated in torch on the device -----------------------
def _reference_merge(ys, scales, flips, img_size, nl=3):
    out = []
    for y, si, fi in zip(ys, scales, flips):
        p = y.clone()
        p[:, :4] /= si
        x, yy, wh, cls = p.split((1, 1, 2, p.shape[1] - 4), 1)
        if fi == 2:
            yy = img_size[0] - yy
        elif fi == 3:
            x = img_size[1] - x
        out.append(torch.cat((x, yy, wh, cls), 1))
    g = sum(4 ** x for x in range(nl))
    out[0] = out[0][..., :-(out[0].shape[-1] // g)]
    out[-1] = out[-1][..., (out[-1].shape[-1] // g) * 4 ** (nl - 1):]
    return torch.cat(out, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("B,no,hw,flips", [(2, 84, (640, 640), (None, 3, None)), (3, 16, (128, 192), (None, 2, 3)),
                                           (1, 117, (640, 480), (3, 2, None))])
def test_tta_merge_matches_torch_on_the_device(B, no, hw, flips, dtype):
    gen = torch.Generator().manual_seed(B * no)
    cfg = stock_cfg("yolo11", "n")
    passes = T.geometry(hw[0], hw[1], 32, lambda h, w: Plan(cfg, 1, h, w).meta["levels"])
    assert sum(e - b for b, e in (p.window for p in passes)) % 2 == 1  # odd total: rows start inside a vector
    ys = []
    for p in passes:
        A = sum(lh * lw for lh, lw in Plan(cfg, 1, *p.padded).meta["levels"])
        y = torch.rand(B, no, A, generator=gen) * torch.tensor([hw[1], hw[0], 90.0, 70.0] + [1.0] * (no - 4))[None, :, None]
        ys.append(y.to(DEV, dtype))
    scales = [p.ratio for p in passes]
    assert T.reference_windows([y.shape[2] for y in ys], 3) == [p.window for p in passes]
    got = O.tta_merge(ys, [p.window for p in passes], scales, flips, hw)
    ref = _reference_merge(ys, scales, flips, hw)
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (B, no, sum(e - b for b, e in (p.window for p in passes)))
    d = (got.float() - ref.float()).abs()
    if dtype == torch.float32:
        assert d.max().item() <= 2.4e-7 * max(hw), d.max().item()
    else:
        assert bool((d <= _ulp16(ref)).all()), d.max().item()
    print(f"tta_merge {B}x{no} {hw} {flips} {dtype}: max |d| {d.max().item():.3g}, bit-identical {torch.equal(got, ref)}")


# ---- 4. the engine's TTA vs the reference's (tta.npz) ---------------------------------------------------------------------------
def _engine(case, precision):
    m = R.Model(case["family"], case["scale"], case["nc"], "detect")
    P = R.synth_params(m, case["seed"])
    kw = {} if precision == "fp16" else {"precision": precision}
    return YoloEngine(stock_cfg(case["family"], case["scale"], case["nc"], "detect"), P, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp16", "fp32x", "fp32"])
@pytest.mark.parametrize("tag", ["yolo11n", "bsyolo11n"])
def test_engine_tta_matches_the_reference(tag, precision):
    """fp32x / fp32: the north-star tolerance (|dscore| <= 1e-3, |dbox| <= 1e-3 * max(H, W)).  fp16: the fp16 storage's stated class
    of error -- for YOLO11n the bounds of test_engine_matches_reference_golden.  BS-YOLO11n at this input (160 x 224) is past that
    test's x3 bounds in its plain single-scale forward already, and so is the oracle's CPU emulation of fp16 storage (score max 4.3e-2 /
    p99.9 2.1e-2 / mean 7.1e-4, box max 8.1 px against the reference's fp32 forward, which the fp32 modes meet to 3e-5): its bounds
    are set about 2x above the engine's measurement on the whole y (score max 4.3e-2 / p99.9 1.7e-2 / mean 4.9e-4, box max 5.2 px /
    mean 0.16 px).
    In every precision the first pass's window is the plain forward's, bit for bit: the TTA glue adds no error of its own."""
    z, meta = _fixture()
    case = meta["cases"][tag]
    x, yref = _case_input(case), z[f"{tag}_y"]  # yref: the reference's y at the stored anchors y_idx
    eng = _engine(case, precision)
    xd = x.to(DEV, torch.float16 if precision == "fp16" else torch.float32)
    y, aux = eng(xd, augment=True)
    y1, _ = eng(xd)
    torch.cuda.synchronize()
    assert aux is None and list(y.shape) == list(z[f"{tag}_y_shape"])
    w0 = eng.tta_geometry(*x.shape[2:])[0].window
    assert torch.equal(y[..., :w0[1]], y1[..., w0[0]:w0[1]])
    g = meta["geometry"].get(f"{x.shape[2]}x{x.shape[3]}")
    if g is not None:
        assert y.shape[2] == g["total"]
    nc = case["nc"]
    y = y.float().cpu()[..., torch.from_numpy(z[f"{tag}_y_idx"]).long()].numpy()
    es, eb = np.abs(y[:, 4:4 + nc] - yref[:, 4:4 + nc]), np.abs(y[:, :4] - yref[:, :4])
    print(f"{tag} {precision}: score max {es.max():.3g} mean {es.mean():.3g}; box max {eb.max():.3g} mean {eb.mean():.3g}")
    if precision != "fp16":
        assert es.max() <= 1e-3 and eb.max() <= 1e-3 * max(x.shape[2:]), (es.max(), eb.max())
    elif tag == "yolo11n":
        q = lambda e: float(np.quantile(e, 0.999))  # noqa: E731
        assert es.max() < 1e-2 and q(es) < 5e-3 and es.mean() < 1e-4, (es.max(), q(es), es.mean())
        assert eb.max() < 1.0 and q(eb) < 0.8 and eb.mean() < 0.05, (eb.max(), q(eb), eb.mean())
    else:
        q = lambda e: float(np.quantile(e, 0.999))  # noqa: E731
        assert es.max() < 9e-2 and q(es) < 3.5e-2 and es.mean() < 1e-3, (es.max(), q(es), es.mean())
        assert eb.max() < 10.5 and eb.mean() < 0.35, (eb.max(), eb.mean())
    eng.close()


# ---- 5. bus.jpg end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32x", "fp32", "fp16"])
def test_tta_on_the_reference_image(precision):
    """letterbox -> the engine's TTA -> bsy_nms against the reference's TTA detections on config-1's photograph (its class-bias shift
    puts detections on it): fp32 modes the same count and, matched one for one, boxes within 0.64 px and scores within 1e-3; fp16 the
    bounds of test_config1_on_the_reference_image."""
    z, _ = _fixture()
    zc = np.load(GOLDEN / "config1_bus.npz")
    cmeta = json.loads(str(zc["meta"]))
    m = R.Model("yolo11", "n", 80, "detect")
    P = R.synth_params(m, cmeta["seed"])
    for k in P:
        if ".cv3." in k and k.endswith(".2.bias"):
            P[k] = P[k] + cmeta["cls_shift"]
    half = precision == "fp16"
    xd = HLB.preprocess([zc["bgr"]], (640, 640), half=half, pt=True, stride=32, device=DEV)
    eng = YoloEngine(stock_cfg("yolo11", "n"), P, **({} if half else {"precision": precision}))
    y, _ = eng(xd, augment=True)
    assert list(y.shape) == list(z["bus_y_shape"]) == [1, 84, 11411]
    ytop = y[0].float().cpu()[:, torch.from_numpy(z["bus_y_idx"]).long()].numpy()
    det, counts = HN.nms_batched(y, cmeta["conf"], cmeta["iou"], max_det=300)
    torch.cuda.synchronize()
    es, eb = np.abs(ytop[4:] - z["bus_y_top"][4:]).max(), np.abs(ytop[:4] - z["bus_y_top"][:4]).max()
    n, ref = int(counts[0]), z["bus_pred"]
    got = det[0, :n].cpu().numpy()
    print(f"bus TTA {precision}: score max {es:.3g}, box max {eb:.3g} px, detections {n} (reference {len(ref)})")
    eng.close()
    if half:
        assert es < 2e-2 and eb < 4.0, (es, eb)
        assert abs(n - len(ref)) <= max(3, len(ref) // 10), (n, len(ref))
        return
    assert es <= 1e-3 and eb <= 0.64, (es, eb)
    assert n == len(ref) > 0
    free = list(range(n))
    for r in ref:  # one-for-one: same class, nearest box
        cand = [j for j in free if got[j, 5] == r[5]]
        assert cand, r
        j = min(cand, key=lambda j: np.abs(got[j, :4] - r[:4]).max())
        assert np.abs(got[j, :4] - r[:4]).max() <= 0.64 and abs(got[j, 4] - r[4]) <= 1e-3, (got[j], r)
        free.remove(j)


# ---- 6. the plugin --------------------------------------------------------------------------------------------------------------
class _StandIn(torch.nn.Module):
    """A reference model as `accelerate` sees it (test_boundary.StandIn's shape): `.yaml`, the reference's state_dict names, and a
    forward -- the CPU oracle -- that counts the calls which reach it."""

    def __init__(self, task="detect"):
        super().__init__()
        self.yaml = stock_cfg("yolo11", "n", 80, task)
        self.ref = R.Model("yolo11", "n", 80, task)
        for name, t in R.synth_params(self.ref, 0).items():
            mod = self
            *path, leaf = name.split(".")
            for p in path:
                if not hasattr(mod, p):
                    mod.add_module(p, torch.nn.Module())
                mod = getattr(mod, p)
            if leaf in ("running_mean", "running_var", "num_batches_tracked"):
                mod.register_buffer(leaf, t.clone())
            else:
                mod.register_parameter(leaf, torch.nn.Parameter(t.clone(), requires_grad=False))
        self.calls = 0
        self.eval()

    def forward(self, x, *args, **kwargs):
        self.calls += 1
        P = {k: v.detach().float().cpu() for k, v in self.state_dict().items()}
        with torch.inference_mode():
            y, aux = self.ref.forward(P, x.detach().float().cpu())
        return y.to(x.device, x.dtype), [a.to(x.device, x.dtype) for a in aux]


class DetectionModel(_StandIn):  # the class name the reference's _predict_augment requires (tasks.py:356)
    pass


def _xb(B=2, H=64, W=96, seed=0):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed))


@pytest.mark.gpu
def test_accelerate_routes_augment_to_the_engine_tta():
    m = DetectionModel().to(DEV)
    plugin.accelerate(m)
    x = _xb().half().to(DEV)
    y, aux = m(x, augment=True)
    st = m._bsy_state
    assert aux is None and m.calls == 0 and st["fallbacks"] == 0 and st["tta_calls"] == 1
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    eng = YoloEngine(m.yaml, sd)
    y2, aux2 = eng(x, augment=True)
    torch.cuda.synchronize()
    assert aux2 is None and torch.equal(y, y2)
    y3, _ = m(x, augment=True, visualize=True, embed=[1], profile=True)  # ignored under augment (tasks.py:134-136)
    assert m.calls == 0 and st["tta_calls"] == 2 and torch.equal(y3, y)
    y4, _ = m(x, augment=True)
    assert torch.equal(y4, y)
    y32, _ = m(x.float(), augment=True)  # an fp32 caller: the fp32x engine's TTA
    assert m.calls == 0 and st["tta_calls"] == 4 and st["fp32_calls"] == 1 and y32.dtype == torch.float32 and y32.shape == y.shape
    eng.close()
    plugin.restore(m)
    for mod, kw in ((DetectionModel(), {"tta": "reference"}), (_StandIn(), {})):  # opt-out; any other class keeps its own forward
        mod = plugin.accelerate(mod.to(DEV), **kw)
        mod(x, augment=True)
        assert mod.calls == 1 and mod._bsy_state["tta_calls"] == 0 and mod._bsy_state["fallbacks"] == 1
        plugin.restore(mod)
    with pytest.raises(ValueError):
        plugin.accelerate(DetectionModel(), tta="sometimes")


@pytest.mark.gpu
def test_engine_tta_on_segment_graphs_is_the_single_scale_forward():
    P = R.synth_params(R.Model("yolo11", "n", 80, "segment"), 0)
    eng = YoloEngine(stock_cfg("yolo11", "n", 80, "segment"), P)
    x = _xb().half().to(DEV)
    y, (raws, mc, proto) = eng(x, augment=True)
    y2, (raws2, mc2, proto2) = eng(x)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(mc, mc2) and torch.equal(proto, proto2)
    assert all(torch.equal(a, b) for a, b in zip(raws, raws2))
    with pytest.raises(NotImplementedError):
        eng(x, visualize=True)
    eng.close()


@pytest.mark.gpu
def test_engine_tta_graph_mode_equals_eager_and_replays():
    P = R.synth_params(R.Model("yolo11", "n", 80, "detect"), 0)
    x = _xb(B=3, H=128, W=192, seed=5).half().to(DEV)
    eager = YoloEngine(stock_cfg("yolo11", "n"), P)
    graph = YoloEngine(stock_cfg("yolo11", "n"), P, graph=True)
    y0, _ = eager(x, augment=True)
    ys = [graph(x, augment=True)[0] for _ in range(graph.graph_ring)]  # one capture per pass and output-ring slot
    caps = graph.graph_stats["captures"]
    y2, _ = graph(x, augment=True)
    torch.cuda.synchronize()
    assert all(torch.equal(y0, y) for y in ys + [y2])
    assert graph.graph_stats["captures"] == caps and graph.graph_stats["replays"] >= 3  # persistent scaled inputs: no re-capture
    eager.close()
    graph.close()
