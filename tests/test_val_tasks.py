"""Segment and OBB validator matching on the device: mask IoU on bit planes (csrc/val_masks.hip: bsy_pack_masks, bsy_val_match_masks)
and probiou matching (csrc/val_match.hip: bsy_val_match_rotated), through bs_yolo_amd.val and plugin.install_val_metrics, against
fixtures made by running the reference's own SegmentationValidator._process_batch / OBBValidator._process_batch
(tests/golden/make_val_task_fixtures.py).

Masks are exact: the IoU matrix must equal the reference's mask_iou with torch.equal, tp_m its _process_batch(..., masks=True).
Rotated is banded: device cosf / sinf / logf / expf need not equal the CPU libm to the last ulp.  ROT_ERR is
max |iou_out - reference IoU| over the fixture as measured on an MI355X (the test prints the figure and keeps it inside the band);
a detection is compared only if none of its class-matching reference IoUs lies within 4 x ROT_ERR of a threshold, all others must
match the reference's tp exactly, and at most 1 % of the detections may be left out that way."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import ROOT
from bs_yolo_amd import lib as L
from bs_yolo_amd import val as V  # at the parent commit: no match_masks_batched -> every test below fails
from val_task_helpers import (IOUV, comparable, label_masks, mask_case, mask_cases, matmul_iou, popcount_iou, rotated_cases, to_words)

match_masks_batched, match_rotated_batched = V.match_masks_batched, V.match_rotated_batched

DEV = "cuda:0"
ROT_ERR = 1.848e-6  # measured on an MI355X over the whole fixture; the CPU's own fp32 is 2.3e-6 off float64
ROT_BAND = 4 * ROT_ERR


def torch_resize(gt, shape):
    """segment/val.py:210-212 with the reference's own torch call (CPU here; the wrapper makes the same call on the device)."""
    t = torch.nn.functional.interpolate(torch.from_numpy(gt).float()[None], tuple(shape), mode="bilinear", align_corners=False)[0]
    return t.gt_(0.5).numpy().astype(np.uint8)


# ---- host side (no GPU) ------------------------------------------------------------------------------------------------
def test_iouv_is_the_validators():
    assert np.array_equal(IOUV, torch.linspace(0.5, 0.95, 10).numpy())


def test_new_entries_are_declared_and_bound():
    header = (ROOT / "include" / "bsyolo.h").read_text()
    for s in ("bsy_pack_masks", "bsy_val_match_masks_workspace_bytes", "bsy_val_match_masks", "bsy_val_match_rotated"):
        assert s + "(" in header and s in L.SYMBOLS and hasattr(L.lib, s)
    assert L.lib.bsy_val_match_masks_workspace_bytes(16, 300, 64) == 16 * 300 * 64 * 4
    assert L.lib.bsy_val_match_masks_workspace_bytes(0, 300, 64) == 0


def test_new_entries_reject_bad_arguments_before_any_launch():
    d = C.c_void_p(64)  # never dereferenced: every check below fails before a launch
    iouv = (C.c_float * 10)(*IOUV.tolist())
    with pytest.raises(L.BsyError, match="null pointer"):
        L.check(L.lib.bsy_pack_masks(None, L.BSY_F32, 4, 25600, 0, d, d, None))
    with pytest.raises(L.BsyError, match="bad sizes"):
        L.check(L.lib.bsy_pack_masks(d, L.BSY_F32, 0, 25600, 0, d, d, None))
    with pytest.raises(L.BsyError, match="bad sizes"):
        L.check(L.lib.bsy_pack_masks(d, L.BSY_F32, 4, (1 << 24) + 1, 0, d, d, None))
    with pytest.raises(L.BsyError, match="dtype"):
        L.check(L.lib.bsy_pack_masks(d, 7, 4, 25600, 1, d, d, None))
    with pytest.raises(L.BsyError, match="aligned"):
        L.check(L.lib.bsy_pack_masks(d, L.BSY_U8, 4, 25600, 0, C.c_void_p(68), d, None))

    def masks(det=d, row=6, B=1, max_det=300, words=400, Lmax=8, n_iou=10, out=d, iou_out=d, ws=None, ws_bytes=0, pp=d):
        return L.lib.bsy_val_match_masks(det, row, d, B, max_det, pp, d, d, d, words, d, d, Lmax, iouv, n_iou, out, iou_out, ws, ws_bytes, None)

    with pytest.raises(L.BsyError, match="null pointer"):
        L.check(masks(det=None))
    with pytest.raises(L.BsyError, match="null pointer"):
        L.check(masks(out=None))
    for kw in (dict(B=0), dict(max_det=1025), dict(max_det=0), dict(row=5), dict(Lmax=0), dict(Lmax=8193), dict(n_iou=17), dict(words=0),
               dict(words=(1 << 18) + 1)):
        with pytest.raises(L.BsyError, match="bad sizes"):
            L.check(masks(**kw))
    with pytest.raises(L.BsyError, match="aligned"):
        L.check(masks(pp=C.c_void_p(68)))
    with pytest.raises(L.BsyError, match="workspace"):  # neither iou_out nor a workspace
        L.check(masks(iou_out=None))
    with pytest.raises(L.BsyError, match="workspace"):
        L.check(masks(iou_out=None, ws=d, ws_bytes=300 * 8 * 4 - 1))

    def rot(det=d, row=7, B=1, max_det=300, Lmax=8, n_iou=10, out=d):
        return L.lib.bsy_val_match_rotated(det, row, d, B, max_det, d, d, d, Lmax, iouv, n_iou, out, None, None)

    with pytest.raises(L.BsyError, match="null pointer"):
        L.check(rot(det=None))
    with pytest.raises(L.BsyError, match="null pointer"):
        L.check(rot(out=None))
    for kw in (dict(B=0), dict(row=6), dict(max_det=1025), dict(Lmax=0), dict(Lmax=8193), dict(n_iou=0), dict(n_iou=17)):
        with pytest.raises(L.BsyError, match="bad sizes"):
            L.check(rot(**kw))


def test_popcount_iou_equals_the_reference_bit_for_bit():
    """The premise of the device kernel, on the host: integer popcounts, then the reference's fp32 operations == its matmul form."""
    z, meta = mask_cases()
    for m in meta:
        c = mask_case(z, m)
        got = popcount_iou(to_words(label_masks(c, torch_resize)), to_words(c["pred"]))
        assert got.dtype == np.float32 and np.array_equal(got, c["iou"]), m["tag"]
    e = mask_case(z, next(m for m in meta if m["tag"] == "edges"))["iou"]
    assert e[0, 0] == 1.0 and e[1, 1] == np.float32(1.0) / (np.float32(1.0) + np.float32(1e-7)) and e[1, 1] < 1.0  # identical; union of 1 pixel
    assert (e[2] == 0).all() and (e[:, 2] == 0).all()  # an empty label, an empty prediction: 0 / 1e-7


def test_fixture_covers_the_cases():
    z, meta = mask_cases()
    tags = {m["tag"]: m for m in meta}
    assert {(m["overlap"], m["pred_shape"][1:] == m["gt_shape"][1:]) for m in meta} == {(a, b) for a in (False, True) for b in (False, True)}
    assert (tags["odd"]["pred_shape"][1] * tags["odd"]["pred_shape"][2]) % 64 != 0 and tags["d1024"]["pred_shape"][0] == 1024
    cases, rmeta = rotated_cases()
    assert rmeta["excluded_f64_band"] < 0.01 * rmeta["detections"]
    assert max(len(c["det"]) for c in cases) == 1024


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, name):
        def f(*a, **k):
            self.calls.append((name, len(a), dict(k)))
            return name
        return f


def test_hook_dispatches_on_the_call(monkeypatch):
    """install_val_metrics with recording stand-ins, no GPU: the segment signature, the 5-column labels and the CPU fallthrough."""
    from bs_yolo_amd import plugin
    rec = _Recorder()
    for n in ("process_batch", "process_batch_masks", "process_batch_rotated"):
        monkeypatch.setattr(V, n, rec(n))

    class Seg:  # models/yolo/segment/val.py:173
        iouv = torch.linspace(0.5, 0.95, 10)

        def _process_batch(self, detections, gt_bboxes, gt_cls, pred_masks=None, gt_masks=None, overlap=False, masks=False):
            rec.calls.append(("orig", masks, overlap))
            return "orig"

    class Det:  # models/yolo/detect/val.py:209, obb/val.py:53: three arguments
        iouv = torch.linspace(0.5, 0.95, 10)

        def _process_batch(self, detections, gt_bboxes, gt_cls):
            rec.calls.append(("orig3",))
            return "orig3"

    det, box, rbox, cls = torch.zeros(3, 6), torch.zeros(2, 4), torch.zeros(2, 5), torch.zeros(2)
    pm, gm = torch.zeros(3, 8, 8), torch.zeros(1, 8, 8)
    v, w = plugin.install_val_metrics(Seg()), plugin.install_val_metrics(Det())
    # CPU tensors fall through to the original method with the arguments they came with
    assert v._process_batch(det, box, cls) == "orig" and v._process_batch(det, box, cls, pm, gm, True, masks=True) == "orig"
    assert w._process_batch(det, rbox, cls) == "orig3"
    assert rec.calls == [("orig", False, False), ("orig", True, True), ("orig3",)]
    rec.calls.clear()
    monkeypatch.setattr(plugin, "_on_device", lambda t: True)  # the recorders stand for the device calls
    assert v._process_batch(det, box, cls) == "process_batch"
    assert v._process_batch(det, box, cls, pm, gm, True, masks=True) == "process_batch_masks"
    assert w._process_batch(torch.zeros(3, 7), rbox, cls) == "process_batch_rotated"
    assert w._process_batch(det, box, cls) == "process_batch"
    assert [c[0] for c in rec.calls] == ["process_batch", "process_batch_masks", "process_batch_rotated", "process_batch"]
    rec.calls.clear()
    assert v._process_batch(torch.zeros(1025, 6), box, cls, pm, gm, False, masks=True) == "orig"  # more than 1024 detections
    assert rec.calls == [("orig", True, False)]


# ---- device: masks -----------------------------------------------------------------------------------------------------
def _dev_case(c, dtype=torch.float32):
    pred = torch.from_numpy(c["pred"]).to(DEV).to(dtype)
    # the index map keeps a dtype that holds its values (bool cannot); masks take every dtype
    gt = torch.from_numpy(c["gt"]).to(DEV).to(torch.float32 if (c["overlap"] and dtype == torch.bool) else dtype)
    return torch.from_numpy(c["det"]).to(DEV), torch.from_numpy(c["gt_cls"]).to(DEV), pred, gt


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.uint8, torch.bool])
def test_pack_masks_and_label_map_bits(dtype):
    """The planes are the documented layout, tail bits zero, areas = pixel counts, for H W a multiple of 64 or not."""
    z, meta = mask_cases()
    for tag in ("plain", "odd", "edges"):
        c = mask_case(z, next(m for m in meta if m["tag"] == tag))
        p = V.pack_masks(torch.from_numpy(c["pred"]).to(DEV).to(dtype))
        torch.cuda.synchronize()
        want = to_words(c["pred"])
        assert p.hw == c["pred"].shape[1] * c["pred"].shape[2] and p.planes.dtype == torch.int64
        assert np.array_equal(p.planes.cpu().numpy().view(np.uint64), want), tag
        assert np.array_equal(p.areas.cpu().numpy(), c["pred"].reshape(len(want), -1).sum(1)), tag
    if dtype != torch.bool:
        for tag in ("overlap", "odd_overlap"):
            c = mask_case(z, next(m for m in meta if m["tag"] == tag))
            nl = len(c["gt_cls"])
            p = V.pack_label_map(torch.from_numpy(c["gt"]).to(DEV).to(dtype), nl)
            torch.cuda.synchronize()
            lm = label_masks(c, None)
            assert np.array_equal(p.planes.cpu().numpy().view(np.uint64), to_words(lm)), tag
            assert np.array_equal(p.areas.cpu().numpy(), lm.reshape(nl, -1).sum(1)), tag


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.uint8, torch.bool])
def test_masks_per_image_equal_the_reference(dtype):
    z, meta = mask_cases()
    for m in meta:
        c = mask_case(z, m)
        det, cls, pred, gt = _dev_case(c, dtype)
        if gt.shape[1:] != pred.shape[1:] and not gt.is_floating_point():
            gt = gt.float()  # the reference resizes float label masks (segment/val.py:211)
        nl, nd = c["iou"].shape
        iou = torch.full((1, nl, nd), -1.0, device=DEV)
        tp = V.process_batch_masks(det, cls, pred, gt, c["overlap"], iou_out=iou)
        torch.cuda.synchronize()
        print(m["tag"], dtype, "iou max |diff|", float((iou[0].cpu() - torch.from_numpy(c["iou"])).abs().max()))
        assert torch.equal(iou[0].cpu(), torch.from_numpy(c["iou"])), m["tag"]
        assert tp.dtype == torch.bool and torch.equal(tp.cpu(), torch.from_numpy(c["tp_m"])), m["tag"]
        again = V.process_batch_masks(det, cls, pred, gt, c["overlap"])  # the matrix in the workspace instead
        assert torch.equal(again, tp), m["tag"]


def _ragged_masks(cases, extra_empty=True):
    """One padded batch from cases of one prediction resolution, plus an image without detections and one without labels."""
    H, W = cases[0]["pred"].shape[1:]
    words = (H * W + 63) // 64
    B = len(cases) + (2 if extra_empty else 0)
    max_det, Lmax = max(len(c["det"]) for c in cases), max(len(c["gt_cls"]) for c in cases)
    det = torch.zeros((B, max_det, 6), device=DEV)
    counts, gcounts = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    pp, pa = torch.zeros((B, max_det, words), dtype=torch.int64, device=DEV), torch.zeros((B, max_det), dtype=torch.int32, device=DEV)
    gp, ga = torch.zeros((B, Lmax, words), dtype=torch.int64, device=DEV), torch.zeros((B, Lmax), dtype=torch.int32, device=DEV)
    gcls = torch.zeros((B, Lmax), device=DEV)
    for b, c in enumerate(cases):
        d, cls, pred, gt = _dev_case(c)
        nd, nl = len(d), len(cls)
        p, g = V.pack_masks(pred), V.label_planes(gt, nl, c["overlap"], (H, W))
        det[b, :nd], pp[b, :nd], pa[b, :nd] = d, p.planes, p.areas
        gp[b, :nl], ga[b, :nl], gcls[b, :nl] = g.planes, g.areas, cls
        counts[b], gcounts[b] = nd, nl
    if extra_empty:  # rows of garbage that the counts must keep out
        b = len(cases)
        pp[b:], pa[b:], gp[b:], ga[b:] = -1, H * W, -1, H * W
        counts[b], gcounts[b] = 0, Lmax
        counts[b + 1], gcounts[b + 1] = max_det, 0
    return det, counts, V.PackedMasks(pp, pa, H * W), V.PackedMasks(gp, ga, H * W), gcls, gcounts


@pytest.mark.gpu
def test_masks_ragged_batch_equals_the_reference():
    z, meta = mask_cases()
    by_shape = {}
    for m in meta:
        by_shape.setdefault(tuple(m["pred_shape"][1:]), []).append(mask_case(z, m))
    assert len(by_shape[(160, 160)]) >= 3 and len(by_shape[(100, 150)]) >= 3
    for shape, cases in by_shape.items():
        det, counts, pp, gp, gcls, gcounts = _ragged_masks(cases)
        B, max_det, Lmax = det.shape[0], det.shape[1], gp.planes.shape[1]
        iou = torch.full((B, Lmax, max_det), -1.0, device=DEV)
        tp = match_masks_batched(det, counts, pp, gp, gcls, gcounts, iou_out=iou)
        torch.cuda.synchronize()
        tp, iou = tp.cpu(), iou.cpu()
        for b, c in enumerate(cases):
            nl, nd = c["iou"].shape
            assert torch.equal(iou[b, :nl, :nd], torch.from_numpy(c["iou"])), (shape, c["tag"])
            assert (iou[b, nl:] == 0).all() and (iou[b, :, nd:] == 0).all()
            assert torch.equal(tp[b, :nd], torch.from_numpy(c["tp_m"])) and not tp[b, nd:].any(), (shape, c["tag"])
        assert not tp[len(cases):].any() and (iou[len(cases):] == 0).all()  # no detections; no labels


@pytest.mark.gpu
def test_masks_zero_detections_and_zero_labels_per_image():
    pm, gm = torch.ones((3, 16, 16), device=DEV), torch.ones((2, 16, 16), device=DEV)
    det, cls = torch.zeros((3, 6), device=DEV), torch.zeros(2, device=DEV)
    a = V.process_batch_masks(det[:0], cls, pm[:0], gm)
    b = V.process_batch_masks(det, cls[:0], pm, gm[:0])
    assert a.shape == (0, 10) and b.shape == (3, 10) and a.dtype == b.dtype == torch.bool and not b.any()
    r = V.process_batch_rotated(torch.zeros((3, 7), device=DEV), torch.zeros((0, 5), device=DEV), cls[:0])
    assert r.shape == (3, 10) and not r.any()


@pytest.mark.gpu
def test_large_masks_and_many_labels_against_popcounts():
    """Sizes past the fixture: 640 x 640 (6 400 words, 13 LDS passes) with 300 detections x 70 labels, and 100 x 150 (an odd word count:
    8-byte loads) with 1024 detections, and 1030 labels, against mask_iou restated on the host in the reference's matmul form."""
    g = torch.Generator().manual_seed(3)
    for (H, W, nd, nl) in ((640, 640, 300, 70), (100, 150, 1024, 9), (36, 36, 17, 1030)):
        base = torch.rand((nl, H // 4, W // 4), generator=g) < 0.3
        gt = torch.nn.functional.interpolate(base[None].float(), (H, W))[0] > 0.5
        src = torch.randint(0, nl, (nd,), generator=g)
        pred = gt[src] ^ (torch.rand((nd, H, W), generator=g) < 0.05)
        want = matmul_iou(gt.numpy(), pred.numpy())
        det = torch.zeros((nd, 6))
        det[:, 5] = (src % 3).float()
        cls = (torch.arange(nl) % 3).float()
        iou = torch.empty((1, nl, nd), device=DEV)
        V.process_batch_masks(det.to(DEV), cls.to(DEV), pred.to(DEV), gt.to(DEV), False, iou_out=iou)
        torch.cuda.synchronize()
        assert np.array_equal(iou[0].cpu().numpy(), want), (H, W, nd, nl)


@pytest.mark.gpu
def test_tie_rule_known_answer():
    """Our documented rule, not the reference's (its argsort is unstable on exact ties): the lower label index wins an exact tie,
    and per label the lowest-index detection wins.  Labels 0 and 1 are the same mask / box; detection 0 overlaps both with IoU 0.8,
    detection 1 equals both (IoU 1): both choose label 0 (never label 1); label 0 goes to detection 0 at every threshold detection 0
    reaches, and to detection 1 only above that."""
    gm = torch.zeros((3, 20, 20), device=DEV)
    gm[0, 0:10, 0:10] = 1
    gm[1, 0:10, 0:10] = 1
    gm[2, 12:20, 12:20] = 1
    pm = torch.zeros((2, 20, 20), device=DEV)
    pm[0, 0:8, 0:10] = 1
    pm[1, 0:10, 0:10] = 1
    det = torch.zeros((2, 6), device=DEV)
    cls = torch.zeros(3, device=DEV)
    tp = V.process_batch_masks(det, cls, pm, gm).cpu()
    want = torch.zeros((2, 10), dtype=torch.bool)
    iou = torch.empty((1, 3, 2), device=DEV)
    V.process_batch_masks(det, cls, pm, gm, iou_out=iou)
    assert iou[0, 0, 0].item() == iou[0, 1, 0].item() and iou[0, 0, 1].item() == iou[0, 1, 1].item() == 1.0
    want[0] = torch.from_numpy(IOUV <= iou[0, 0, 0].item())  # 80 / 100 pixels
    want[1] = ~want[0]  # had detection 1 taken label 1 on the tie, it would be True at every threshold
    assert want[0, :6].all() and want[1, -2:].all() and torch.equal(tp, want)
    # the same shape of tie with rotated boxes: two identical labels
    gt = torch.tensor([[50.0, 50, 40, 20, 0.3], [50.0, 50, 40, 20, 0.3], [200.0, 200, 30, 30, 0.0]], device=DEV)
    rd = torch.tensor([[52.0, 50, 40, 20, 0.9, 0, 0.3], [50.0, 50, 40, 20, 0.8, 0, 0.3]], device=DEV)
    riou = torch.empty((1, 3, 2), device=DEV)
    rtp = V.process_batch_rotated(rd, gt, cls, iou_out=riou).cpu()
    assert riou[0, 0, 0].item() == riou[0, 1, 0].item() and riou[0, 0, 0].item() >= 0.5
    rwant = torch.zeros((2, 10), dtype=torch.bool)
    rwant[0] = torch.from_numpy(IOUV <= riou[0, 0, 0].item())
    rwant[1] = ~rwant[0] & torch.from_numpy(IOUV <= riou[0, 0, 1].item())
    assert rwant[0, 0] and torch.equal(rtp, rwant)


# ---- device: rotated -----------------------------------------------------------------------------------------------------
def _rot_check(tp, iou, c, stats):
    ref_iou, ref_tp = c["iou"], c["tp"]
    fin = np.isfinite(ref_iou)
    assert np.array_equal(np.isfinite(iou), fin), c["tag"]
    err = float(np.abs(iou[fin] - ref_iou[fin]).max()) if fin.any() else 0.0
    ok = comparable(ref_iou, c["det"][:, 5], c["gt_cls"], ROT_BAND)
    stats["err"] = max(stats["err"], err)
    stats["excluded"] += int((~ok).sum())
    stats["n"] += len(ok)
    stats["mismatch"] += int((tp[ok] != ref_tp[ok]).any(1).sum())
    stats["mismatch_all"] += int((tp != ref_tp).any(1).sum())


def _rot_assert(stats, what):
    print(f"rotated {what}: max |iou_out - reference| = {stats['err']:.3e} (ROT_ERR {ROT_ERR:.1e}, band {ROT_BAND:.1e}); excluded "
          f"{stats['excluded']} of {stats['n']} detections; rows differing: {stats['mismatch']} compared, {stats['mismatch_all']} in all")
    assert stats["err"] <= ROT_BAND  # an error past the band would void the argument that decisions outside it cannot flip
    assert stats["excluded"] <= 0.01 * stats["n"]
    assert stats["mismatch"] == 0


@pytest.mark.gpu
def test_rotated_per_image_against_the_reference():
    cases, _ = rotated_cases()
    stats = dict(err=0.0, excluded=0, n=0, mismatch=0, mismatch_all=0)
    for c in cases:
        det, gt, cls = (torch.from_numpy(c[k]).to(DEV) for k in ("det", "gt", "gt_cls"))
        iou = torch.empty((1, len(gt), len(det)), device=DEV)
        tp = V.process_batch_rotated(det, gt, cls, iou_out=iou)
        torch.cuda.synchronize()
        _rot_check(tp.cpu().numpy(), iou[0].cpu().numpy(), c, stats)
    _rot_assert(stats, "per image")


@pytest.mark.gpu
def test_rotated_ragged_batch_against_the_reference():
    cases, _ = rotated_cases()
    B, max_det, Lmax = len(cases) + 2, max(len(c["det"]) for c in cases), max(len(c["gt"]) for c in cases)
    det, gt, gcls = torch.full((B, max_det, 7), 7.0), torch.full((B, Lmax, 5), 3.0), torch.zeros((B, Lmax))
    counts, gcounts = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b, c in enumerate(cases):
        nd, nl = len(c["det"]), len(c["gt"])
        det[b, :nd], gt[b, :nl], gcls[b, :nl] = torch.from_numpy(c["det"]), torch.from_numpy(c["gt"]), torch.from_numpy(c["gt_cls"])
        counts[b], gcounts[b] = nd, nl
    counts[-2], gcounts[-2] = 0, Lmax
    counts[-1], gcounts[-1] = max_det, 0
    iou = torch.full((B, Lmax, max_det), -1.0, device=DEV)
    tp = match_rotated_batched(det.to(DEV), counts, gt.to(DEV), gcls.to(DEV), gcounts, iou_out=iou)
    torch.cuda.synchronize()
    tp, iou = tp.cpu().numpy(), iou.cpu().numpy()
    stats = dict(err=0.0, excluded=0, n=0, mismatch=0, mismatch_all=0)
    for b, c in enumerate(cases):
        nd, nl = len(c["det"]), len(c["gt"])
        _rot_check(tp[b, :nd], iou[b, :nl, :nd], c, stats)
        assert not tp[b, nd:].any() and (iou[b, nl:] == 0).all() and (iou[b, :, nd:] == 0).all()
    assert not tp[-2:].any() and (iou[-2:] == 0).all()
    _rot_assert(stats, "ragged batch")
    again = match_rotated_batched(det.to(DEV), counts, gt.to(DEV), gcls.to(DEV), gcounts)  # without the matrix
    assert np.array_equal(again.cpu().numpy(), tp)


# ---- device: the hook ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hook_segment_signature_returns_the_fixture():
    from bs_yolo_amd import plugin

    class Seg:
        def __init__(self):
            self.iouv, self.calls = torch.linspace(0.5, 0.95, 10).to(DEV), 0

        def _process_batch(self, detections, gt_bboxes, gt_cls, pred_masks=None, gt_masks=None, overlap=False, masks=False):
            self.calls += 1
            return None

    v = plugin.install_val_metrics(Seg())
    z, meta = mask_cases()
    for m in meta:
        c = mask_case(z, m)
        det, cls, pred, gt = _dev_case(c)
        box = torch.from_numpy(c["gt_boxes"]).to(DEV)
        tp = v._process_batch(det, box, cls)  # at the parent commit the next call raises TypeError: seven arguments
        tp_m = v._process_batch(det, box, cls, pred, gt, c["overlap"], masks=True)
        assert torch.equal(tp.cpu(), torch.from_numpy(c["tp"])) and torch.equal(tp_m.cpu(), torch.from_numpy(c["tp_m"])), m["tag"]
    assert v.calls == 0
    c = mask_case(z, meta[0])
    det, cls, pred, gt = (t.cpu() for t in _dev_case(c))
    assert v._process_batch(det, torch.from_numpy(c["gt_boxes"]), cls, pred, gt, c["overlap"], masks=True) is None and v.calls == 1


@pytest.mark.gpu
def test_hook_five_column_labels_take_the_rotated_path():
    from bs_yolo_amd import plugin

    class Obb:  # models/yolo/obb/val.py:53
        def __init__(self):
            self.iouv, self.calls = torch.linspace(0.5, 0.95, 10).to(DEV), 0

        def _process_batch(self, detections, gt_bboxes, gt_cls):
            self.calls += 1
            return None

    v = plugin.install_val_metrics(Obb())
    cases, _ = rotated_cases()
    stats = dict(err=0.0, excluded=0, n=0, mismatch=0, mismatch_all=0)
    for c in cases:
        det, gt, cls = (torch.from_numpy(c[k]).to(DEV) for k in ("det", "gt", "gt_cls"))
        tp = v._process_batch(det, gt, cls)  # at the parent commit: box_iou on xywh rows, the wrong matrix
        _rot_check(tp.cpu().numpy(), c["iou"], c, stats)  # (the hook returns no matrix: the reference's stands in for the error term)
    assert v.calls == 0 and stats["excluded"] <= 0.01 * stats["n"] and stats["mismatch"] == 0 and stats["n"] > 1500
    assert v._process_batch(*(torch.from_numpy(cases[0][k]) for k in ("det", "gt", "gt_cls"))) is None and v.calls == 1


# ---- device: graph capture -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batched_matchers_replay_in_a_captured_graph():
    """One batched call of each matcher, captured on a single stream (no parallel branches), replays with equal output."""
    z, meta = mask_cases()
    cases = [mask_case(z, m) for m in meta if tuple(m["pred_shape"][1:]) == (160, 160)]
    det, counts, pp, gp, gcls, gcounts = _ragged_masks(cases)
    counts, gcounts = counts.to(DEV), gcounts.to(DEV)
    rc, _ = rotated_cases()
    c = rc[1]
    rdet, rgt, rcls = (torch.from_numpy(c[k]).to(DEV)[None].contiguous() for k in ("det", "gt", "gt_cls"))
    rn = torch.tensor([len(c["det"])], dtype=torch.int32, device=DEV)
    rl = torch.tensor([len(c["gt"])], dtype=torch.int32, device=DEV)
    iouv = IOUV.tolist()  # a host list: nothing in the captured region reads the device back
    eager_m = match_masks_batched(det, counts, pp, gp, gcls, gcounts, iouv)
    eager_r = match_rotated_batched(rdet, rn, rgt, rcls, rl, iouv)
    eager_b = V.match_batched(rdet[..., :6].contiguous(), rn, rgt[..., :4], rcls, rl, iouv)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_m = match_masks_batched(det, counts, pp, gp, gcls, gcounts, iouv)
        out_r = match_rotated_batched(rdet, rn, rgt, rcls, rl, iouv)
        out_b = V.match_batched(rdet[..., :6].contiguous(), rn, rgt[..., :4], rcls, rl, iouv)
    for o in (out_m, out_r, out_b):
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_m, eager_m) and torch.equal(out_r, eager_r) and torch.equal(out_b, eager_b)
    assert eager_m.any() and eager_r.any()
