"""OBB (oriented-box) models on the engine: the OBB head in the plan, its angle decode, the device rotated NMS (the reference's
fast-NMS on probiou) and the batched OBB postprocess, against fixtures made by running the reference
(tests/golden/make_obb_fixtures.py)."""
import ctypes as C
import json
import math
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from bs_yolo_amd import lib as L
from bs_yolo_amd.graphs import stock_cfg
from bs_yolo_amd.plan import Plan
from bs_yolo_amd.weights import pack_plan_weights, synth_state_dict
from graph_helpers import RefModel, engine, fixture, state_dict, x_of

DEV = "cuda:0"
GRAPHS = ["yolo11n_obb", "yolov8n_obb"]
HEAD = {"yolo11": 23, "yolov8": 22}  # index of the OBB layer


# ---- host side (no GPU) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "fp32"])
@pytest.mark.parametrize("family", ["yolo11", "yolov8"])
def test_obb_plan_has_the_angle_branch_and_the_decode_launch(family, precision):
    plan = Plan(stock_cfg(family, "n", nc=15, task="obb"), 1, 64, 64, precision=precision)
    head = f"model.{HEAD[family]}"
    for i in range(3):
        for j in range(3):
            assert f"{head}.cv4.{i}.{j}" in plan.wrecs
        assert plan.wrecs[f"{head}.cv4.{i}.2"].real_cout == 1
    dec = [o for o in plan.ops if o["kind"] == L.OP_DECODE]
    assert len(dec) == 1 and dec[0]["ne"] == 1 and dec[0]["nm"] == 0 and dec[0]["dst"].C == 4 + 15 + 1
    assert all(t.ld % 4 == 0 for t in dec[0]["msk"]) and len(dec[0]["msk"]) == 3
    assert not any(o.get("out_f32", 0) >= 2 for o in plan.ops)  # no fused-decoder epilogue: the box needs the angle
    assert plan.meta["ne"] == 1 and plan.meta["nm"] == 0
    # yolov8 keeps the legacy head (3x3 Conv class branch), yolo11 the DWConv one
    assert (f"{head}.cv3.0.0.0" in plan.wrecs) == (family == "yolo11")
    pack_plan_weights(plan, synth_state_dict(plan))
    arr = plan.c_ops()
    assert [o.ne for o in arr if o.kind == L.OP_DECODE] == [1]


def test_detect_and_segment_plans_carry_no_angle():
    for task in ("detect", "segment"):
        plan = Plan(stock_cfg("yolo11", "n", task=task), 1, 64, 64)
        assert plan.meta["ne"] == 0 and all(o.get("ne", 0) == 0 for o in plan.ops)


@pytest.mark.parametrize("tag", GRAPHS)
def test_obb_weights_pack_from_the_reference_state_dict(tag):
    _, meta = fixture(tag)
    sd = state_dict(tag, None)
    seen = set()

    class Recording(dict):
        def __getitem__(self, k):
            seen.add(k)
            return dict.__getitem__(self, k)

    for precision in ("fp16", "fp32x"):
        plan = Plan(stock_cfg(meta["family"], meta["scale"], meta["nc"], "obb"), 1, 64, 64, precision=precision)
        pack_plan_weights(plan, Recording(sd))  # a missing key raises KeyError
    cv4 = {n for n in sd if ".cv4." in n}
    assert len(cv4) == 3 * (2 * 5 + 2) and cv4 <= seen


def test_obb_head_arguments():
    cfg = stock_cfg("yolo11", "n", nc=15, task="obb")
    cfg["head"][-1] = [[16, 19, 22], 1, "OBB", ["nc", 1, [64, 128, 256]]]  # parse_model's form: channel list appended
    assert Plan(cfg, 1, 64, 64).meta["ne"] == 1
    cfg["head"][-1] = [[16, 19, 22], 1, "OBB", ["nc", 2]]
    with pytest.raises(NotImplementedError):
        Plan(cfg, 1, 64, 64)


def test_obb_graph_support():
    from bs_yolo_amd.plugin import SUPPORTED_HEADS, graph_support
    assert "OBB" in SUPPORTED_HEADS
    for fam in ("yolo11", "yolov8"):
        assert graph_support(stock_cfg(fam, "n", nc=15, task="obb")) == {"fp16": True, "fp32": True}


def test_rotated_nms_and_obb_scale_are_declared_and_check_their_arguments():
    header = (ROOT / "include" / "bsyolo.h").read_text()
    for s in ("bsy_nms_rotated_workspace_bytes", "bsy_nms_rotated", "bsy_obb_scale"):
        assert s + "(" in header and s in L.SYMBOLS
    with pytest.raises(L.BsyError, match="null pointer"):
        L.check(L.lib.bsy_nms_rotated(None, 0, 1, 15, 1, 84, 0.25, 0.7, None, 0, 0, 0, 300, 30000, 7680.0, None, None, None, 0, None))
    dummy = C.c_void_p(16)  # never dereferenced: every check below fails before a launch
    with pytest.raises(L.BsyError, match="Invalid IoU"):
        L.check(L.lib.bsy_nms_rotated(dummy, 0, 1, 15, 1, 84, 0.25, 1.5, None, 0, 0, 0, 300, 30000, 7680.0, dummy, dummy, dummy, 1 << 30, None))
    with pytest.raises(L.BsyError, match="workspace"):
        L.check(L.lib.bsy_nms_rotated(dummy, 0, 1, 15, 1, 84, 0.25, 0.7, None, 0, 0, 0, 300, 30000, 7680.0, dummy, dummy, dummy, 16, None))
    with pytest.raises(L.BsyError, match="bad sizes"):
        L.check(L.lib.bsy_nms_rotated(dummy, 0, 1, 15, -1, 84, 0.25, 0.7, None, 0, 0, 0, 300, 30000, 7680.0, dummy, dummy, dummy, 1 << 30, None))
    with pytest.raises(L.BsyError, match="obb_scale"):
        L.check(L.lib.bsy_obb_scale(None, None, 1, 300, 7, None, None, None, None, None, None))
    with pytest.raises(L.BsyError, match="obb_scale"):
        L.check(L.lib.bsy_obb_scale(dummy, dummy, 1, 300, 6, dummy, dummy, dummy, dummy, dummy, None))  # no angle column
    assert L.lib.bsy_nms_rotated_workspace_bytes(16, 21504, 15, 0, 30000) >= 16 * (21504 * 8 + 21504 * 68)


# ---- device ---------------------------------------------------------------------------------------------------------------
def _cfg(meta):
    return stock_cfg(meta["family"], meta["scale"], meta["nc"], "obb")


def _engine(tag, precision):
    return engine(tag, precision, None, cfg=_cfg(fixture(tag)[1]))


TOL = {"fp16": (1e-2, 1.0, 2e-2), "fp32x": (1e-3, None, 1e-3), "fp32": (1e-3, None, 1e-3)}  # score, box (None: 1e-3 imgsz), angle


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp16", "fp32x", "fp32"])
@pytest.mark.parametrize("tag", GRAPHS)
def test_obb_graph_matches_reference(tag, precision):
    z, meta = fixture(tag)
    eng = _engine(tag, precision)
    nc = meta["nc"]
    ts, tb, ta = TOL[precision]
    for si in range(len(meta["shapes"])):
        x = x_of(meta, si)
        xin = (x.half() if precision == "fp16" else x).to(DEV)
        y, (raws, angle) = eng(xin)
        y = y.clone()
        angle_t = angle.clone()
        y2, (_, angle2) = eng(xin)
        torch.cuda.synchronize()
        assert torch.equal(y, y2) and torch.equal(angle_t, angle2)  # the same input twice: the same bits
        A = y.shape[-1]
        assert tuple(y.shape) == (x.shape[0], 4 + nc + 1, A) and tuple(angle_t.shape) == (x.shape[0], 1, A)
        assert torch.equal(angle_t, y[:, 4 + nc:])
        yr, yref = y.float().cpu().numpy(), z[f"y{si}"]
        imgsz = max(x.shape[2], x.shape[3])
        es = np.abs(yr[:, 4:4 + nc] - yref[:, 4:4 + nc]).max()
        eb = np.abs(yr[:, :4] - yref[:, :4]).max()
        ea = np.abs(angle_t.float().cpu().numpy() - z[f"angle{si}"]).max()
        assert es < ts, (tag, precision, si, "score", es)
        assert eb < (tb if tb is not None else 1e-3 * imgsz), (tag, precision, si, "box", eb)
        assert ea < ta, (tag, precision, si, "angle", ea)
        for l, r in enumerate(raws):
            rr = z[f"raw{si}_{l}"]
            rel = 3e-2 if precision == "fp16" else 1e-3
            assert np.abs(r.float().cpu().numpy() - rr).max() <= rel * max(1.0, np.abs(rr).max()), (tag, precision, si, "raw", l)
        print(tag, precision, si, f"score {es:.2e} box {eb:.2e} angle {ea:.2e}")
    eng.close()


@pytest.mark.gpu
def test_obb_graph_without_raw_maps_and_in_chunks(monkeypatch):
    z, meta = fixture("yolo11n_obb")
    eng = _engine("yolo11n_obb", "fp32")
    x = x_of(meta, 1).to(DEV)
    y, (raws, angle) = eng(x, want_raw=False)
    assert raws == [None, None, None] and torch.equal(angle, y[:, -1:])
    y_full = y.clone()
    monkeypatch.setattr(eng, "_max_view_elems", lambda H, W: (1 << 31) // 2)  # forces the chunked large-batch path
    yc, (rc, ac) = eng(x)
    assert torch.equal(yc, y_full) and torch.equal(ac, yc[:, -1:]) and len(rc) == 3 and rc[0].shape[0] == x.shape[0]
    eng.close()


def _probiou64(b1, b2):
    """batch_probiou's formula (metrics.py:327-358) in float64: b1 (N, 5), b2 (M, 5) -> (N, M)."""
    def cov(b):
        a, c_, t = b[:, 2] ** 2 / 12, b[:, 3] ** 2 / 12, b[:, 4]
        co, si = np.cos(t), np.sin(t)
        return a * co ** 2 + c_ * si ** 2, a * si ** 2 + c_ * co ** 2, (a - c_) * co * si
    a1, bb1, c1 = (v[:, None] for v in cov(b1))
    a2, bb2, c2 = (v[None] for v in cov(b2))
    x1, y1, x2, y2 = b1[:, 0:1], b1[:, 1:2], b2[None, :, 0], b2[None, :, 1]
    eps = 1e-7
    den = (a1 + a2) * (bb1 + bb2) - (c1 + c2) ** 2
    t1 = ((a1 + a2) * (y1 - y2) ** 2 + (bb1 + bb2) * (x1 - x2) ** 2) / (den + eps) * 0.25
    t2 = ((c1 + c2) * (x2 - x1) * (y1 - y2)) / (den + eps) * 0.5
    t3 = np.log(den / (4 * np.sqrt(np.clip(a1 * bb1 - c1 ** 2, 0, None) * np.clip(a2 * bb2 - c2 ** 2, 0, None)) + eps) + eps) * 0.5
    bd = np.clip(t1 + t2 + t3, eps, 100.0)
    return 1 - np.sqrt(1 - np.exp(-bd) + eps)


def _near_threshold(pred, b, kw, rows):
    """Rows (of either side) whose keep decision a float64 restatement puts within 1e-5 of the threshold."""
    p = pred[b].astype(np.float64).T  # (A, C)
    nc = kw.get("nc") or p.shape[1] - 4
    sc = p[:, 4:4 + nc]
    if kw.get("multi_label") and nc > 1:
        i, j = np.nonzero(sc > kw["conf_thres"])
        cand = np.concatenate([p[i, :4], sc[i, j, None], j[:, None], p[i, -1:]], 1)
    else:
        j = sc.argmax(1)
        cand = np.concatenate([p[:, :4], sc.max(1, keepdims=True), j[:, None], p[:, -1:]], 1)
        cand = cand[cand[:, 4] > kw["conf_thres"]]
    if kw.get("classes") is not None:
        cand = cand[np.isin(cand[:, 5], kw["classes"])]
    cand = cand[np.argsort(-cand[:, 4], kind="stable")][:kw.get("max_nms", 30000)]
    off = cand[:, 5:6] * (0 if kw.get("agnostic") else 7680)
    boxes = np.concatenate([cand[:, :2] + off, cand[:, 2:4], cand[:, 6:7]], 1)
    out = set()
    thr = kw["iou_thres"]
    for r in rows:
        k = np.nonzero((np.abs(cand[:, 0] - r[0]) < 1e-4) & (np.abs(cand[:, 4] - r[4]) < 1e-7) & (cand[:, 5] == r[5]))[0]
        for i in k:
            if i and abs(_probiou64(boxes[:i], boxes[i:i + 1]).max() - thr) <= 1e-5:
                out.add(tuple(np.round(r[:6], 3)))
    return out


@pytest.mark.gpu
def test_rotated_nms_matches_reference():
    from bs_yolo_amd import nms as HN
    z = np.load(GOLDEN / "obb_nms.npz")
    cases = json.loads(str(z["cases"]))
    excused = 0
    for tag, kw, n_img in cases:
        pred = z[tag + ".pred"]
        got = HN.non_max_suppression(torch.from_numpy(pred).to(DEV), rotated=True, **kw)
        assert len(got) == n_img
        for b in range(n_img):
            g, w = got[b].float().cpu().numpy(), z[f"{tag}.out{b}"]
            assert g.shape[1:] == (7,) and w.shape[1:] == (7,)
            if g.shape == w.shape and np.allclose(g, w, atol=1e-5, rtol=0):
                continue
            # equal scores (fp16 predictions have many) have no pinned order in the reference (torch.argsort is not stable): the same
            # kept set in another order among ties is the same answer
            srt = lambda r: r[np.lexsort(r[:, ::-1].T)]  # noqa: E731
            if g.shape == w.shape and np.array_equal(np.sort(g[:, 4]), np.sort(w[:, 4])) and np.allclose(srt(g), srt(w), atol=1e-5, rtol=0):
                continue
            # a difference is allowed only for candidates whose deciding probiou sits within 1e-5 of the threshold
            key = lambda r: tuple(np.round(r[:6], 3))  # noqa: E731
            diff = {key(r) for r in g} ^ {key(r) for r in w}
            near = _near_threshold(pred, b, kw, list(g) + list(w))
            assert diff and diff <= near, (tag, b, len(g), len(w), sorted(diff - near)[:4])
            excused += len(diff)
    print(f"rotated NMS: {excused} candidate(s) excused as within 1e-5 of the threshold")
    chain = HN.non_max_suppression(torch.from_numpy(z["chain.pred"]).to(DEV), 0.25, 0.5, nc=2, rotated=True)
    assert len(chain[0]) == 1  # fast-NMS: the third box goes with the second (greedy NMS would keep it)


@pytest.mark.gpu
def test_rotated_nms_on_the_graph_output_matches_reference():
    from bs_yolo_amd import nms as HN
    for tag in GRAPHS:
        z, meta = fixture(tag)
        y = torch.from_numpy(z["y1"]).to(DEV)
        got = HN.non_max_suppression(y, meta["nms_conf"], meta["nms_iou"], nc=meta["nc"], rotated=True)
        for b, g in enumerate(got):
            w = z[f"nms1_{b}"]
            assert g.shape == w.shape and np.allclose(g.cpu().numpy(), w, atol=1e-5, rtol=0), (tag, b)
        assert tag != "yolo11n_obb" or sum(len(g) for g in got) > 0


@pytest.mark.gpu
def test_obb_postprocess_matches_reference():
    from bs_yolo_amd import obb as OB
    z = np.load(GOLDEN / "obb_scale.npz")
    for ci, (s1, s0, rp) in enumerate(json.loads(str(z["cases"]))):
        rows = torch.from_numpy(z[f"case{ci}.rows"])
        n = rows.shape[0]
        det = torch.zeros(2, 128, 7)
        det[1, :n] = rows
        counts = torch.tensor([0, n], dtype=torch.int32)
        got = OB.postprocess(det.to(DEV), counts.to(DEV), s1, [s0, s0], None if rp is None else [rp, rp])
        assert got[0].shape == (0, 7)
        g, w = got[1].cpu().numpy(), z[f"case{ci}.obb"]
        assert g.shape == w.shape
        ulp = np.spacing(np.abs(w).astype(np.float32))
        bad = np.abs(g - w) > ulp
        assert not bad.any(), (ci, np.argwhere(bad)[:4], g[bad][:4], w[bad][:4])


@pytest.mark.gpu
def test_accelerate_obb_model_and_rotated_nms_hook():
    from bs_yolo_amd import nms as HN
    from bs_yolo_amd import plugin
    z, meta = fixture("yolo11n_obb")
    m = RefModel(_cfg(meta), state_dict("yolo11n_obb", None)).to(DEV)
    plugin.accelerate(m)
    x = x_of(meta, 1).to(DEV)
    y, (raws, angle) = m(x)  # fp32 input: the fp32x engine
    assert m.calls == 0 and len(raws) == 3
    nc = meta["nc"]
    yr = y.cpu().numpy()
    assert np.abs(yr[:, 4:4 + nc] - z["y1"][:, 4:4 + nc]).max() <= 1e-3
    assert np.abs(yr[:, :4] - z["y1"][:, :4]).max() <= 1e-3 * 128
    assert np.abs(angle.cpu().numpy() - z["angle1"]).max() <= 1e-3
    assert m(x, augment=True) == "original" and m.calls == 1  # the reference runs OBB single-scale (tasks.py:356-358)
    plugin.restore(m)

    calls = []

    def ref_nms(prediction, *a, **k):
        calls.append(k.get("rotated", False))
        return "reference"

    ops = types.SimpleNamespace(non_max_suppression=ref_nms)
    plugin.install_nms(ops)  # default: rotated calls stay on the original
    assert ops.non_max_suppression(y, 0.25, 0.7, nc=nc, rotated=True) == "reference" and calls == [True]
    f = plugin.install_nms(ops, rotated=True)
    assert ops.non_max_suppression is f and plugin.install_nms(ops, rotated=True) is f
    got = ops.non_max_suppression(y, 0.25, 0.7, nc=nc, rotated=True)
    assert calls == [True] and isinstance(got, list) and len(got) == x.shape[0]
    want = HN.non_max_suppression(y, 0.25, 0.7, nc=nc, rotated=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert sum(len(g) for g in got) > 0
    # labels are ignored for rotated calls, as in the reference (ops.py:256)
    got_l = ops.non_max_suppression(y, 0.25, 0.7, None, False, False, [torch.zeros(0, 5)] * 2, nc=nc, rotated=True)
    assert calls == [True] and all(torch.equal(a, b) for a, b in zip(got_l, want))
