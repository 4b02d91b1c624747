"""The detect / segment postprocess (csrc/nms.hip, csrc/masks.hip, scale_boxes) on the dispatch paths and edges that the
per-kernel parity file does not reach.

NMS is compared bit-exactly with oracle.postproc_ref.non_max_suppression; 0/1 masks with a float64 restatement that also
gives an fp32 error band per pixel (oracle.postproc_ref.process_mask64 & co.): a device pixel may differ from `v > 0`
only where |v| <= e, and the share of such pixels -- a property of the inputs, computed from the reference alone -- is at
most 1e-4.  The CPU tests of this file pin the new references and run the hand-written known answers through the oracle;
the GPU tests (``pytest -m gpu``) run the same cases on the device.
"""
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from postproc_helpers import DEV, fp16_reference, nms_compare, nms_compare_fp16, rand_pred

from oracle import postproc_ref as PP

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from bs_yolo_amd import lib as L  # noqa: F401  (fails loudly when the .so is missing)
    from bs_yolo_amd import masks as HM
    from bs_yolo_amd import nms as HN


# ------------------------------------------------------------------------------------------------------------
# input builders
# ------------------------------------------------------------------------------------------------------------
def grid_boxes(A):
    """Well-separated xywh boxes: 24-pixel pitch, 8..16 pixels wide -- nothing overlaps, NMS keeps every candidate."""
    a = torch.arange(A)
    return torch.stack(((a % 256) * 24.0 + 12, (a // 256) * 24.0 + 12, 8.0 + (a % 5) * 2, 8.0 + (a % 3) * 4), 0)


def cluster_boxes(A, k=97):
    """Heavy duplicates: k locations, every anchor a slightly different box at one of them."""
    a = torch.arange(A)
    c = a % k
    return torch.stack(((c % 10) * 60.0 + 40 + (a % 7) * 0.5, (c // 10) * 60.0 + 40 + (a % 3) * 0.75, 40.0 + (a % 4), 36.0 + (a % 5)), 0)


def exact_pred(ns, nc, A, conf, multi_label, boxes, seed, nm=0):
    """(len(ns), 4+nc+nm, A) predictions with EXACTLY ns[b] scores above `conf` in image b (multi_label: over all
    (anchor, class) pairs, several classes of one anchor among them; best-class: ns[b] anchors, one class each)."""
    g = torch.Generator().manual_seed(seed)
    B = len(ns)
    pred = torch.zeros(B, 4 + nc + nm, A)
    pred[:, :4] = (grid_boxes(A) if boxes == "grid" else cluster_boxes(A))[None]
    pred[:, 4:4 + nc] = torch.rand(B, nc, A, generator=g) * conf * 0.9
    if nm:
        pred[:, 4 + nc:] = torch.randn(B, nm, A, generator=g)
    for b, n in enumerate(ns):
        hi = conf + 0.01 + torch.rand(n, generator=g) * (0.98 - conf)
        if multi_label:
            pool = min(A * nc, max(n + nc, (3 * n) // 2))       # dense: most anchors of the pool carry several classes
            flat = torch.randperm(pool, generator=g)[:n]
            pred[b, 4 + flat % nc, flat // nc] = hi
        else:
            an = torch.randperm(A, generator=g)[:n]
            pred[b, 4 + torch.randint(0, nc, (n,), generator=g), an] = hi
    assert [(pred[b, 4:4 + nc] > conf).sum().item() for b in range(B)] == list(ns)
    return pred


# ------------------------------------------------------------------------------------------------------------
# A. NMS -- hand-written known answers (exact in fp32), run through the oracle on the CPU and the kernels on the GPU
# ------------------------------------------------------------------------------------------------------------
BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0)))


def _ka_iou_equality(thr):
    """Class 1 (offset 7680, exact): xyxy [0,0,4,4] and [0,0,4,2] -- intersection 8, union 16, IoU exactly 0.5."""
    pred = torch.zeros(1, 6, 3)
    pred[0, :4, 0] = torch.tensor([2.0, 2.0, 4.0, 4.0])
    pred[0, :4, 1] = torch.tensor([2.0, 1.0, 4.0, 2.0])
    pred[0, :4, 2] = torch.tensor([100.0, 100.0, 4.0, 4.0])
    pred[0, 5] = torch.tensor([0.75, 0.5, 0.125])  # anchor 2 is below conf
    kw = dict(conf_thres=0.25, iou_thres=thr)
    rows = [[0.0, 0.0, 4.0, 4.0, 0.75, 1.0]]
    if thr >= 0.5:  # `iou > thr` is strict: equality keeps both
        rows.append([0.0, 0.0, 4.0, 2.0, 0.5, 1.0])
    return pred, kw, [torch.tensor(rows)]


def _ka_ties_across_chunk():
    """520 anchors, every score 0.5 (order = anchor index), separated boxes except three identical pairs: (255, 256)
    straddles the first 256-candidate chunk, (100, 400) and (511, 512) later ones -- the second of each pair goes."""
    A = 520
    pred = torch.zeros(1, 6, A)
    a = torch.arange(A)  # 64 columns: every coordinate an integer below 2048, exact in fp16 too
    pred[0, :4] = torch.stack(((a % 64) * 24.0 + 12, (a // 64) * 24.0 + 12, 8.0 + (a % 5) * 2, 8.0 + (a % 3) * 4), 0)
    for keep, drop in ((255, 256), (100, 400), (511, 512)):
        pred[0, :4, drop] = pred[0, :4, keep]
    pred[0, 4] = 0.5
    kept = [a for a in range(A) if a not in (256, 400, 512)]
    xyxy = PP.xywh2xyxy(pred[0, :4].T)[kept]  # halves of even sizes: exact
    rows = torch.cat((xyxy, torch.full((len(kept), 1), 0.5), torch.zeros(len(kept), 1)), 1)
    return pred, dict(conf_thres=0.25, iou_thres=0.5, max_det=1000), [rows]


def _ka_multilabel_class_tie():
    """Multi-label, equal scores: candidates are ordered by anchor * nc + class, so anchor 0's classes 0 and 2 come
    before anchor 1's class 0 (a class-major order would put (1, 0) second)."""
    pred = torch.zeros(1, 7, 2)
    pred[0, :4, 0] = torch.tensor([10.0, 10.0, 4.0, 4.0])
    pred[0, :4, 1] = torch.tensor([50.0, 50.0, 8.0, 2.0])
    pred[0, 4:, 0] = torch.tensor([0.5, 0.125, 0.5])
    pred[0, 4:, 1] = torch.tensor([0.5, 0.0, 0.125])
    rows = torch.tensor([[8.0, 8.0, 12.0, 12.0, 0.5, 0.0], [8.0, 8.0, 12.0, 12.0, 0.5, 2.0], [46.0, 49.0, 54.0, 51.0, 0.5, 0.0]])
    return pred, dict(conf_thres=0.25, iou_thres=0.5, multi_label=True), [rows]


KNOWN_ANSWERS = {
    "iou_equal_thr_0.5_keeps_both": lambda: _ka_iou_equality(0.5),
    "iou_equal_thr_just_below_keeps_one": lambda: _ka_iou_equality(BELOW_HALF),
    "ties_across_256_chunk": _ka_ties_across_chunk,
    "multilabel_tie_order_a_nc_c": _ka_multilabel_class_tie,
}


@pytest.mark.parametrize("name", list(KNOWN_ANSWERS))
def test_nms_known_answers_oracle(name):
    pred, kw, want = KNOWN_ANSWERS[name]()
    got = PP.non_max_suppression(pred.clone(), **kw)
    assert len(got) == len(want)
    for g_, w_ in zip(got, want):
        assert tuple(g_.shape) == tuple(w_.shape) and torch.equal(g_, w_)


@gpu
@pytest.mark.parametrize("name", list(KNOWN_ANSWERS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_nms_known_answers_device(name, dtype):
    """The same answers from the kernels (every value is a small dyadic number: exact in fp16 as well), and the oracle."""
    pred, kw, want = KNOWN_ANSWERS[name]()
    got = HN.non_max_suppression(pred.to(dtype).to(DEV), **kw)
    for g_, w_ in zip(got, want):
        assert tuple(g_.shape) == tuple(w_.shape) and torch.equal(g_.float().cpu(), w_), (g_, w_)
    if dtype == torch.float32:
        nms_compare(pred, kw)
    else:
        nms_compare_fp16(pred.half(), kw)


def test_exact_pred_counts_and_closed_form_oracle():
    """The builder's counts are exact, and on separated boxes the oracle keeps min(n, max_nms, max_det) rows: the
    highest scores in order."""
    ns = [1, 2, 255, 257]
    for ml in (False, True):
        pred = exact_pred(ns, 3, 600, 0.3, ml, "grid", 5)
        out = PP.non_max_suppression(pred.clone(), 0.3, 0.5, multi_label=ml, max_det=200, max_nms=256)
        assert [len(o) for o in out] == [min(n, 200, 256) for n in ns]
        sc = pred[3, 4:7]
        top = sc[sc > 0.3].sort(descending=True).values[:200]
        assert torch.equal(out[3][:, 4], top)


# ------------------------------------------------------------------------------------------------------------
# A. NMS on the GPU
# ------------------------------------------------------------------------------------------------------------
def _which_filter(ml, A, misaligned=False):
    return "filter4" if (not ml and A % 4 == 0 and not misaligned) else "filter_half"


FP16_MATRIX = [pytest.param(ml, A, nm, ip, id=f"{'multilabel' if ml else 'bestclass'}-A{A}-nm{nm}-{'inplace' if ip else 'copy'}-{_which_filter(ml, A)}")
               for ml in (False, True) for A in (2000, 2001, 315, 9261) for nm in (0, 32) for ip in (True, False)]


@gpu
@pytest.mark.parametrize("ml,A,nm,in_place", FP16_MATRIX)
def test_nms_fp16_dispatch_matrix(ml, A, nm, in_place):
    """fp16 predictions through both filter kernels: nms_filter4_kernel (best class, A % 4 == 0, 8-byte aligned) and
    nms_filter_kernel<half_t> (everything else: odd A -- 315 = 96x160, 9261 = 672x672 --, multi-label, which also makes
    nms_greedy_kernel<half_t> decode idx / nc); with and without mask coefficients, in place and not."""
    pred = rand_pred(2 if A < 9000 else 1, 6, A, nm, 100 + A + nm).half()
    kw = dict(conf_thres=0.3 if ml else 0.25, iou_thres=0.7, multi_label=ml, in_place=in_place, nc=6)
    got, ref = nms_compare_fp16(pred, kw)
    assert sum(len(r) for r in ref) > 20  # not a vacuous case


@gpu
@pytest.mark.parametrize("ml", [False, True], ids=["bestclass-filter_half", "multilabel-filter_half"])
def test_nms_fp16_misaligned_view(ml):
    pred = rand_pred(2, 6, 2000, 32, 77).half()
    nms_compare_fp16(pred, dict(conf_thres=0.25, iou_thres=0.7, multi_label=ml, nc=6), misaligned=True)


@gpu
def test_nms_fp16_filter_kernels_agree():
    """A % 4 == 0: the aligned tensor goes to nms_filter4_kernel, the same values one element into an allocation to
    nms_filter_kernel<half_t>; rows, counts and the in-place boxes are identical."""
    from postproc_helpers import misaligned_view
    pred = rand_pred(3, 12, 2000, 0, 13).half()
    a, b = pred.clone().to(DEV), misaligned_view(pred)
    assert a.data_ptr() % 8 == 0
    da, ca = HN.nms_batched(a, 0.25, 0.7)
    db, cb = HN.nms_batched(b, 0.25, 0.7)
    torch.cuda.synchronize()
    assert int(ca.sum()) > 50
    assert torch.equal(ca, cb) and torch.equal(da, db) and torch.equal(a, b)


COUNTS_ALL = [1, 2, 255, 256, 257, 511, 513, 4096, 8191, 8192, 8193, 16385]


@gpu
@pytest.mark.parametrize("ml", [False, True], ids=["bestclass", "multilabel"])
@pytest.mark.parametrize("boxes,ns", [("grid", [1, 2, 255, 256, 257, 511, 513, 4096, 8193]), ("cluster", COUNTS_ALL)], ids=["separated", "duplicates"])
def test_nms_exact_candidate_counts(ml, boxes, ns):
    """Exactly n scores above conf_thres, a different n per image of one batch: around the greedy kernel's 256-candidate
    chunk and the sort's LDS / global switch (8192 keys).  Separated boxes: everything is kept, so counts are
    min(n, max_det) in closed form and the cut falls inside a chunk (max_det = 1000).
    Measured CPU oracle time of the slowest case (separated, best-class): 0.5 s (the slowest reference of the file is
    nc80_nm32_A8400_multilabel of test_nms_option_combinations, 0.9 s)."""
    pred = exact_pred(ns, 3, 16800, 0.3, ml, boxes, 31 + ml)
    kw = dict(conf_thres=0.3, iou_thres=0.5, multi_label=ml, max_det=1000)
    got, ref = nms_compare(pred, kw)
    if boxes == "grid":
        assert [len(g_) for g_ in got] == [min(n, 1000) for n in ns]


@gpu
@pytest.mark.parametrize("n", [256, 8193])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_nms_max_nms_at_the_candidate_count(n, d):
    """max_nms in {n - 1, n, n + 1}: the cut drops the lowest score, nothing, nothing."""
    pred = exact_pred([n, n - 1], 3, 9000, 0.3, True, "cluster", 7)
    nms_compare(pred, dict(conf_thres=0.3, iou_thres=0.5, multi_label=True, max_nms=n + d))
    if n == 256:
        sep = exact_pred([n], 3, 600, 0.3, False, "grid", 8)
        got, _ = nms_compare(sep, dict(conf_thres=0.3, iou_thres=0.5, max_nms=n + d, max_det=4096))
        assert len(got[0]) == min(n, n + d)


@gpu
@pytest.mark.parametrize("max_det", [1, 255, 256, 257, 300, 1000, 2048, 4096])
def test_nms_max_det(max_det):
    """The whole accepted range.  Image 0: 5000 separated candidates (more than max_det survive: exactly max_det rows),
    image 1: 200 separated (fewer survive once max_det > 200), image 2: 3000 candidates at 97 locations.  The greedy
    kernel's LDS grows with max_det: 87 152 bytes at 4096."""
    pred = torch.cat((exact_pred([5000, 200], 3, 5120, 0.3, False, "grid", 3), exact_pred([3000], 3, 5120, 0.3, False, "cluster", 4)))
    got, _ = nms_compare(pred, dict(conf_thres=0.3, iou_thres=0.5, max_det=max_det))
    assert [len(got[0]), len(got[1])] == [min(5000, max_det), min(200, max_det)]
    got, _ = nms_compare_fp16(pred.half(), dict(conf_thres=0.3, iou_thres=0.5, max_det=max_det, multi_label=True))


@gpu
def test_nms_max_det_outside_the_range_is_a_clean_error():
    pred = rand_pred(1, 3, 64, 0, 1).to(DEV)
    for bad in (4097, 100000):
        with pytest.raises(RuntimeError, match="max_det 4097 out of range|max_det 100000 out of range"):
            HN.nms_batched(pred.clone(), 0.25, 0.5, max_det=bad)
    with pytest.raises(RuntimeError, match="libbsyolo_hip: nms"):  # an empty output tensor has no address: refused before the range check
        HN.nms_batched(pred.clone(), 0.25, 0.5, max_det=0)
    det, counts = HN.nms_batched(pred.clone(), 0.25, 0.5, max_det=4096)  # and the library still works afterwards
    torch.cuda.synchronize()
    assert 0 <= int(counts[0]) <= 64


def _option_cases():
    return [
        ("nc1_multilabel_switches_off", rand_pred(2, 1, 1500, 0, 41), dict(conf_thres=0.1, iou_thres=0.6, multi_label=True)),
        ("nc1_nm32", rand_pred(2, 1, 700, 32, 42), dict(conf_thres=0.1, iou_thres=0.6, nc=1)),
        ("classes_with_multilabel", rand_pred(2, 8, 1500, 0, 43), dict(conf_thres=0.2, iou_thres=0.6, multi_label=True, classes=[1, 3, 6])),
        ("agnostic_with_multilabel", rand_pred(2, 8, 1500, 0, 44), dict(conf_thres=0.3, iou_thres=0.5, multi_label=True, agnostic=True)),
        ("max_wh_100", rand_pred(2, 8, 1500, 0, 45), dict(conf_thres=0.2, iou_thres=0.5, max_wh=100)),
        ("max_wh_100_multilabel", rand_pred(2, 8, 1500, 0, 46), dict(conf_thres=0.3, iou_thres=0.5, max_wh=100, multi_label=True)),
        ("nc80_nm32_A8400", rand_pred(1, 80, 8400, 32, 47), dict(conf_thres=0.6, iou_thres=0.7, nc=80)),
        ("nc80_nm32_A8400_multilabel", rand_pred(1, 80, 8400, 32, 48), dict(conf_thres=0.9, iou_thres=0.7, nc=80, multi_label=True)),
    ]


@gpu
@pytest.mark.parametrize("idx", range(8), ids=[c[0] for c in _option_cases()])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_nms_option_combinations(idx, dtype):
    _, pred, kw = _option_cases()[idx]
    if dtype == torch.float32:
        _, ref = nms_compare(pred, kw)
    else:
        _, ref = nms_compare_fp16(pred.half(), kw)
    assert sum(len(r) for r in ref) > 10


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_nms_non_contiguous_prediction(dtype):
    """A (B, A, C) tensor transposed to (B, C, A): in_place=False copies (and leaves the caller's tensor alone),
    in_place=True has nothing it could mutate consistently and raises."""
    pred = rand_pred(2, 5, 900, 0, 51).to(dtype)
    kw = dict(conf_thres=0.25, iou_thres=0.6, in_place=False)
    dnc = pred.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    assert not dnc.is_contiguous() and torch.equal(dnc.cpu(), pred)
    got = HN.non_max_suppression(dnc, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dnc.cpu(), pred)
    ref = PP.non_max_suppression(pred.clone(), **kw) if dtype == torch.float32 else [r.half() for r in fp16_reference(pred, kw)[1]]
    assert sum(len(r) for r in ref) > 10
    for g_, r_ in zip(got, ref):
        assert tuple(g_.shape) == tuple(r_.shape) and torch.equal(g_.cpu().float(), r_.float())
    with pytest.raises(ValueError, match="contiguous"):
        HN.non_max_suppression(dnc, conf_thres=0.25, iou_thres=0.6, in_place=True)


# ------------------------------------------------------------------------------------------------------------
# B. masks -- the float64 reference, pinned on the CPU
# ------------------------------------------------------------------------------------------------------------
def mask_inputs(nm, mh, mw, ih, iw, n, seed, pdtype=torch.float32):
    """protos, and an (n, 6 + nm) NMS-like row block whose [:, :4] (xyxy inside ih x iw) and [:, 6:] are the call
    site's non-contiguous views."""
    g = torch.Generator().manual_seed(seed)
    protos = torch.randn(nm, mh, mw, generator=g).to(pdtype)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([iw * 0.6, ih * 0.6])
    wh = torch.rand(n, 2, generator=g) * torch.tensor([iw * 0.4, ih * 0.4]) + 4
    pred = torch.cat((xy, xy + wh, torch.rand(n, 2, generator=g), torch.randn(n, nm, generator=g)), 1)
    return protos, pred


def assert_classified(got, v, e, tag):
    bad, ndiff, amb = PP.classify_masks(got, v, e)
    print(f"{tag}: {ndiff} pixels differ from v > 0, {bad} of them outside the band; ambiguous share {amb:.2e}")
    assert amb <= 1e-4, (tag, amb)  # a condition on the inputs
    assert bad == 0, (tag, bad, ndiff)


def test_mask_reference_reproduces_golden():
    """masks_native.npz (the reference's own outputs): the 0/1 masks under the classification, the resized maps inside
    the band e of the float64 value."""
    z = np.load(GOLDEN / "masks_native.npz")
    for case in json.loads(str(z["cases"])):
        ci, shape = case["ci"], tuple(case["shape"])
        protos, coef, boxes = (torch.from_numpy(z[f"c{ci}.{k}"]) for k in ("protos", "coef", "boxes"))
        if len(coef):
            v, e = PP.process_mask_native64(protos, coef, boxes, shape)
            assert_classified(z[f"c{ci}.native"], v, e, f"golden {ci}")
        for pad, key in ((True, "scaled"), (False, "scaled_nopad")):
            v, e = PP.scale_masks64(protos[None, :2], shape, pad)
            assert (np.abs(z[f"c{ci}.{key}"] - v) <= e).all(), (ci, key)


@pytest.mark.parametrize("nm,mh,mw,ih,iw,n,upsample", [(32, 40, 48, 160, 192, 13, True), (32, 40, 48, 160, 192, 13, False), (16, 27, 35, 108, 140, 9, True),
                                                       (64, 96, 160, 384, 640, 300, False), (32, 160, 160, 640, 640, 9, True)])
def test_mask_reference_agrees_with_oracle(nm, mh, mw, ih, iw, n, upsample):
    """torch's own fp32 process_mask has no mismatch outside the band, and the ambiguous share of these inputs is small."""
    protos, pred = mask_inputs(nm, mh, mw, ih, iw, n, 8)
    ref = PP.process_mask(protos, pred[:, 6:], pred[:, :4], (ih, iw), upsample).numpy()
    v, e = PP.process_mask64(protos, pred[:, 6:], pred[:, :4], (ih, iw), upsample)
    assert v.shape == ref.shape
    assert_classified(ref, v, e, "process_mask")


@pytest.mark.parametrize("nm,mh,mw,shape,n", [(32, 160, 160, (1080, 810), 3), (16, 96, 160, (721, 1279), 2), (32, 160, 160, (333, 500), 9), (8, 160, 160, (100, 75), 8)])
def test_mask_native_reference_agrees_with_oracle(nm, mh, mw, shape, n):
    protos, pred = mask_inputs(nm, mh, mw, shape[0], shape[1], n, 9)
    ref = PP.process_mask_native(protos, pred[:, 6:], pred[:, :4], shape).numpy()
    v, e = PP.process_mask_native64(protos, pred[:, 6:], pred[:, :4], shape)
    assert_classified(ref, v, e, "process_mask_native")
    m = torch.randn(3, 5, mh, mw, generator=torch.Generator().manual_seed(1))
    for pad in (True, False):
        v, e = PP.scale_masks64(m, shape, pad)
        assert (np.abs(PP.scale_masks(m, shape, pad).numpy() - v) <= e).all()


def test_source_index_roundings_differ_by_an_ulp_at_most():
    """fused (ATen) and op-by-op (masks.hip) source coordinates: same cell, weights within one ulp of the coordinate."""
    for n_in, n_out in ((120, 810), (160, 1080), (23, 90), (160, 100), (40, 160)):
        i0, _, _, l1 = PP._src_index(n_in, n_out, True)
        j0, _, _, m1 = PP._src_index(n_in, n_out, False)
        assert np.abs((i0 + l1) - (j0 + m1)).max() <= 2.0 ** -23 * n_in


# box-edge known answers: prototypes of constant +1 and positive coefficients, so every in-box pixel is 1
def _ranges_to_mask(h, w, ranges):
    out = np.zeros((len(ranges), h, w), np.uint8)
    for i, r in enumerate(ranges):
        if r is not None:
            (ya, yb), (xa, xb) = r
            out[i, ya:yb, xa:xb] = 1
    return out


# process_mask, 16 x 16 prototypes of a 64 x 64 image (ratio 0.25): box in image pixels -> ((rows), (cols)) at low resolution
LOW_EDGE = [
    ([8.0, 12.0, 40.0, 52.0], ((3, 13), (2, 10))),      # edges on integer low-res coordinates: x >= 2, x < 10
    ([9.0, 13.0, 39.0, 51.0], ((4, 13), (3, 10))),      # 2.25 .. 9.75, 3.25 .. 12.75
    ([-20.0, -8.0, 30.0, 20.0], ((0, 5), (0, 8))),      # overhangs left and top (x2 = 7.5, y2 = 5)
    ([40.0, 40.0, 100.0, 100.0], ((10, 16), (10, 16))),  # overhangs right and bottom
    ([-8.0, 20.0, 72.0, 24.0], ((5, 6), (0, 16))),      # overhangs left and right, one row
    ([80.0, 80.0, 100.0, 100.0], None),                 # wholly outside
    ([-50.0, -50.0, -10.0, -10.0], None),               # negative coordinates, outside
    ([20.0, 8.0, 20.0, 40.0], None),                    # x2 == x1
    ([40.0, 8.0, 20.0, 40.0], None),                    # x2 < x1
    ([8.0, 40.0, 40.0, 8.0], None),                     # y2 < y1
    ([0.0, 0.0, 64.0, 64.0], ((0, 16), (0, 16))),
]
# the same boxes after the 4x bilinear upsample: low-res columns [a, b) are > 0 on output columns [4a - 2, 4b + 2) clipped
# to the image (the source coordinate 0.25 x - 0.375 is never an integer, so both neighbours always weigh in)
UP_EDGE = [None if r is None else tuple((max(4 * a - 2, 0), min(4 * b + 2, 64)) for a, b in r) for _, r in LOW_EDGE]
# process_mask_native, 40 x 40 prototypes -> a 100 x 80 image: the crop is made in OUTPUT pixels
NATIVE_EDGE = [
    ([10.0, 20.0, 30.0, 50.0], ((20, 50), (10, 30))),
    ([10.5, 20.25, 30.5, 49.75], ((21, 50), (11, 31))),
    ([-5.0, -5.0, 12.0, 8.0], ((0, 8), (0, 12))),
    ([70.0, 90.0, 200.0, 200.0], ((90, 100), (70, 80))),
    ([-3.0, 40.0, 83.0, 41.0], ((40, 41), (0, 80))),
    ([80.0, 0.0, 90.0, 100.0], None),                   # x1 == width: outside
    ([-9.0, -9.0, -1.0, -1.0], None),
    ([25.0, 10.0, 25.0, 60.0], None),
    ([30.0, 10.0, 25.0, 60.0], None),
    ([0.0, 0.0, 80.0, 100.0], ((0, 100), (0, 80))),
]


def _edge_inputs(mh, mw, boxes):
    protos = torch.ones(2, mh, mw)
    coef = torch.tensor([[1.0, 0.5]]).repeat(len(boxes), 1)
    return protos, coef, torch.tensor([b for b, _ in boxes])


def test_mask_box_edges_oracle():
    protos, coef, boxes = _edge_inputs(16, 16, LOW_EDGE)
    assert np.array_equal(PP.process_mask(protos, coef, boxes, (64, 64), False).numpy().astype(np.uint8), _ranges_to_mask(16, 16, [r for _, r in LOW_EDGE]))
    assert np.array_equal(PP.process_mask(protos, coef, boxes, (64, 64), True).numpy().astype(np.uint8), _ranges_to_mask(64, 64, UP_EDGE))
    protos, coef, boxes = _edge_inputs(40, 40, NATIVE_EDGE)
    assert np.array_equal(PP.process_mask_native(protos, coef, boxes, (100, 80)).numpy().astype(np.uint8), _ranges_to_mask(100, 80, [r for _, r in NATIVE_EDGE]))
    for fused in (True, False):
        v, _ = PP.process_mask64(*_edge_inputs(16, 16, LOW_EDGE), (64, 64), True, fused=fused)
        assert np.array_equal((v > 0).astype(np.uint8), _ranges_to_mask(64, 64, UP_EDGE))


# ------------------------------------------------------------------------------------------------------------
# B. masks on the GPU
# ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pdtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_mask_box_edges_device(pdtype):
    for odt in (torch.float32, torch.uint8):
        protos, coef, boxes = _edge_inputs(16, 16, LOW_EDGE)
        args = (protos.to(pdtype).to(DEV), coef.to(DEV), boxes.to(DEV), (64, 64))
        assert np.array_equal(HM.process_mask(*args, False, out_dtype=odt).cpu().numpy().astype(np.uint8), _ranges_to_mask(16, 16, [r for _, r in LOW_EDGE]))
        assert np.array_equal(HM.process_mask(*args, True, out_dtype=odt).cpu().numpy().astype(np.uint8), _ranges_to_mask(64, 64, UP_EDGE))
        protos, coef, boxes = _edge_inputs(40, 40, NATIVE_EDGE)
        got = HM.process_mask_native(protos.to(pdtype).to(DEV), coef.to(DEV), boxes.to(DEV), (100, 80), out_dtype=odt)
        assert np.array_equal(got.cpu().numpy().astype(np.uint8), _ranges_to_mask(100, 80, [r for _, r in NATIVE_EDGE]))


PROCESS_MASK_CASES = [
    # nm, mh, mw, ih, iw, n, upsample
    (32, 40, 48, 160, 192, 13, True), (32, 40, 48, 160, 192, 13, False),
    (32, 160, 160, 640, 640, 37, True),                 # iw = 640: mask_upsample_kernel with blockIdx.x > 0
    (16, 27, 35, 108, 140, 9, True),                    # odd prototype map, 8 + 1 masks
    (64, 96, 160, 384, 640, 300, False),
    (32, 160, 160, 640, 640, 1, True), (8, 160, 160, 640, 640, 8, True), (64, 96, 160, 384, 640, 9, True),
    (32, 192, 320, 768, 1280, 5, True),                 # 1280 wide
    (16, 160, 160, 640, 640, 300, False),
]


@gpu
@pytest.mark.parametrize("pdtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("nm,mh,mw,ih,iw,n,upsample", PROCESS_MASK_CASES)
def test_process_mask_classified(nm, mh, mw, ih, iw, n, upsample, pdtype):
    """Every device pixel that differs from the float64 `v > 0` lies inside the fp32 band of zero; float32 and uint8
    outputs are equal; the arguments are the call site's views of the (n, 6 + nm) rows."""
    protos, pred = mask_inputs(nm, mh, mw, ih, iw, n, 8 + n, pdtype)
    dp, dpred = protos.to(DEV), pred.to(DEV)
    assert n == 1 or (not dpred[:, :4].is_contiguous() and not dpred[:, 6:].is_contiguous())
    got = HM.process_mask(dp, dpred[:, 6:], dpred[:, :4], (ih, iw), upsample)
    got8 = HM.process_mask(dp, dpred[:, 6:], dpred[:, :4], (ih, iw), upsample, out_dtype=torch.uint8)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got8.dtype == torch.uint8 and got.shape == got8.shape
    assert torch.equal(got, got8.float())
    v, e = PP.process_mask64(protos, pred[:, 6:], pred[:, :4], (ih, iw), upsample, fused=False)
    assert tuple(got.shape) == v.shape
    assert_classified(got8.cpu().numpy(), v, e, "process_mask")


NATIVE_CASES = [
    # nm, mh, mw, (oh, ow), n
    (32, 160, 160, (1080, 810), 5), (32, 160, 160, (810, 1080), 1), (32, 160, 160, (333, 500), 9), (16, 160, 160, (500, 333), 8),
    (16, 96, 160, (721, 1279), 8), (8, 160, 160, (100, 75), 9), (64, 40, 40, (31, 23), 300), (32, 184, 320, (720, 1280), 3),
]


@gpu
@pytest.mark.parametrize("pdtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("nm,mh,mw,shape,n", NATIVE_CASES)
def test_process_mask_native_classified(nm, mh, mw, shape, n, pdtype):
    """The retina_masks path: fractional letterbox padding (1080 x 810, 333 x 500, 721 x 1279), downscaling (the original
    smaller than the window), 1280 wide, 1 / 8 / 9 / 300 masks."""
    protos, pred = mask_inputs(nm, mh, mw, shape[0], shape[1], n, 20 + n, pdtype)
    dp, dpred = protos.to(DEV), pred.to(DEV)
    got = HM.process_mask_native(dp, dpred[:, 6:], dpred[:, :4], shape)
    got8 = HM.process_mask_native(dp, dpred[:, 6:], dpred[:, :4], shape, out_dtype=torch.uint8)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got8.dtype == torch.uint8 and torch.equal(got, got8.float())
    v, e = PP.process_mask_native64(protos, pred[:, 6:], pred[:, :4], shape, fused=False)
    assert tuple(got.shape) == v.shape
    assert_classified(got8.cpu().numpy(), v, e, "process_mask_native")


@gpu
@pytest.mark.parametrize("padding", [True, False])
@pytest.mark.parametrize("shape", [(1080, 810), (333, 500), (721, 1279), (100, 75)])
def test_scale_masks_values(shape, padding):
    """scale_masks, N = 3, C = 5: fp32 within the band e of the float64 value; fp16 within e + 2^-11 |v| (one rounding
    to half; + 2^-25, half the spacing of fp16 subnormals, below 2^-14)."""
    m = torch.randn(3, 5, 160, 160, generator=torch.Generator().manual_seed(3))
    v, e = PP.scale_masks64(m, shape, padding, fused=False)
    got = HM.scale_masks(m.to(DEV), shape, padding)
    assert got.dtype == torch.float32 and tuple(got.shape) == v.shape
    r = np.abs(got.cpu().numpy().astype(np.float64) - v) / e
    print(f"scale_masks fp32 {shape} padding={padding}: max |err| / e = {r.max():.3f}")
    assert r.max() <= 1.0
    mh_ = m.half()
    v, e = PP.scale_masks64(mh_, shape, padding, fused=False)
    got = HM.scale_masks(mh_.to(DEV), shape, padding)
    assert got.dtype == torch.float16
    r = np.abs(got.float().cpu().numpy().astype(np.float64) - v) / (e + 2.0 ** -11 * np.abs(v) + 2.0 ** -25)
    print(f"scale_masks fp16 {shape} padding={padding}: max |err| / bound = {r.max():.3f}")
    assert r.max() <= 1.0


# ------------------------------------------------------------------------------------------------------------
# C. scale_boxes
# ------------------------------------------------------------------------------------------------------------
def ulp_distance(a, b):
    """Distance in fp32 ulps (ordered-integer representation; +0 and -0 coincide)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def test_ulp_distance():
    one = np.float32(1)
    assert ulp_distance(one, np.nextafter(one, np.float32(2))) == 1 and ulp_distance(np.float32(0.0), np.float32(-0.0)) == 0
    assert ulp_distance(np.float32(-1e-45), np.float32(1e-45)) == 2


@gpu
@pytest.mark.parametrize("row", [6, 38])
def test_scale_boxes_rows_counts_and_ratio_pads(row):
    """row = 38: the mask coefficients come back untouched; counts of 0, 1 and max_det; ratio_pads for some images; boxes
    that clip on every side.  Box columns within 1 ulp of the oracle's fp32 result, everything else bit-identical."""
    g = torch.Generator().manual_seed(12)
    B, max_det = 5, 33
    det = torch.randn(B, max_det, row, generator=g)
    det[..., :4] = torch.rand(B, max_det, 4, generator=g) * 900 - 130  # beyond every edge of every image below
    counts = torch.tensor([max_det, 1, 0, 17, max_det], dtype=torch.int32)
    shapes = [(1080, 810), (720, 1280), (333, 500), (480, 640), (721, 1279)]
    ratio_pads = [None, ((0.5, 0.5), (3.5, 140.25)), None, ((1.3333334, 1.3333334), (0.0, 0.0)), None]
    for rp in (None, ratio_pads):
        ref = det.clone()
        for b in range(B):
            n = int(counts[b])
            ref[b, :n, :4] = PP.scale_boxes((640, 640), ref[b, :n, :4].clone(), shapes[b], ratio_pad=rp[b] if rp else None)
        d = det.clone().to(DEV)
        HN.scale_boxes_batched(d, counts.to(DEV), (640, 640), shapes, rp)
        torch.cuda.synchronize()
        d = d.cpu()
        assert torch.equal(d[..., 4:], det[..., 4:])
        for b in range(B):
            n = int(counts[b])
            assert torch.equal(d[b, n:], det[b, n:])
            if n:
                got, want = d[b, :n, :4].numpy(), ref[b, :n, :4].numpy()
                assert ulp_distance(got, want).max() <= 1, (b, ulp_distance(got, want).max())
                hi = np.array([shapes[b][1], shapes[b][0]] * 2, np.float32)
                assert (got >= 0).all() and (got <= hi).all()
        full = ref[0, :, :4].numpy()  # the case does clip on every side
        assert (full[:, 0] == 0).any() and (full[:, 1] == 0).any() and (full[:, 2] == 810).any() and (full[:, 3] == 1080).any()
