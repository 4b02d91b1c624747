"""Sliced inference (BASELINE config 5): the oracle's restatement of sahi's slicing / GREEDYNMM against
hand-derived known answers (CPU), and the HIP tile / merge kernels against the oracle (GPU).  Parity is unpinned by the
reference (sahi is not vendored and has no fixture there), see oracle/sahi_ref.py."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import sahi_ref as S  # noqa: E402

DEV = "cuda:0"


# ----------------------------------------------------------------------------------------------------------------------
# CPU: oracle known answers + host slicing arithmetic
# ----------------------------------------------------------------------------------------------------------------------
def test_slice_bboxes_known_answers():
    # BASELINE config 5: 6000 x 4000, 640 crops, stride 640 -> 10 x 7 tiles, the last column / row shifted inwards
    b = S.get_slice_bboxes(4000, 6000, 640, 640, 0, 0)
    assert len(b) == 70
    assert b[0] == [0, 0, 640, 640] and b[9] == [5360, 0, 6000, 640] and b[-1] == [5360, 3360, 6000, 4000]
    assert all(x1 - x0 == 640 and y1 - y0 == 640 for x0, y0, x1, y1 in b)
    # sahi's documented example shape: 20 % overlap -> stride 512 - 102 = 410
    b = S.get_slice_bboxes(1080, 1920, 512, 512, 0.2, 0.2)
    xs = sorted({x0 for x0, _, _, _ in b}); ys = sorted({y0 for _, y0, _, _ in b})
    assert xs == [0, 410, 820, 1230, 1408] and ys == [0, 410, 568]
    # exact fit: no extra slice;  image smaller than the slice: one clipped slice
    assert S.get_slice_bboxes(640, 1280, 640, 640, 0, 0) == [[0, 0, 640, 640], [640, 0, 1280, 640]]
    assert S.get_slice_bboxes(300, 500, 640, 640, 0.2, 0.2) == [[0, 0, 500, 300]]
    # the reference script's setting (detect-sahi.py:9-12): 800 x 800, overlap 0
    assert len(S.get_slice_bboxes(2000, 3000, 800, 800, 0, 0)) == 4 * 3


def test_host_slice_bboxes_equal_oracle():
    from bs_yolo_amd.sahi import get_slice_bboxes  # imports the C-ABI library (no GPU needed for this function)
    rng = np.random.default_rng(0)
    for _ in range(200):
        h, w = int(rng.integers(1, 5000)), int(rng.integers(1, 5000))
        sh, sw = int(rng.integers(32, 1024)), int(rng.integers(32, 1024))
        oh, ow = float(rng.choice([0, 0.1, 0.2, 0.25, 0.5])), float(rng.choice([0, 0.1, 0.2, 0.25, 0.5]))
        assert get_slice_bboxes(h, w, sh, sw, oh, ow) == S.get_slice_bboxes(h, w, sh, sw, oh, ow)
    with pytest.raises(ValueError):
        get_slice_bboxes(100, 100, 64, 64, 1.0, 0.0)


def test_greedy_nmm_known_answers():
    # A (score .9) and B (.8) of class 0 overlap: inter 50 x 100 = 5000, areas 10000 each -> IOS .5, IOU 1/3.
    # C (.7) is class 1 at A's position; D (.6) class 0 far away.
    A = [0, 0, 100, 100, .9, 0]; B = [50, 0, 150, 100, .8, 0]; C = [0, 0, 100, 100, .7, 1]; D = [500, 500, 600, 600, .6, 0]
    boxes = np.array([B, D, A, C], np.float32)
    # greedy_nmm: IOS .5 is NOT < .5 -> B joins A;  has_match: .5 is NOT > .5 -> not merged, B is dropped
    out = S.postprocess(boxes, "GREEDYNMM", "IOS", 0.5)
    np.testing.assert_allclose(out, np.array([A, D, C], np.float32))
    # threshold .4: B merges into A -> union box, max score
    out = S.postprocess(boxes, "GREEDYNMM", "IOS", 0.4)
    np.testing.assert_allclose(out, np.array([[0, 0, 150, 100, .9, 0], D, C], np.float32))
    # IOU 1/3 < .4 -> nothing matches
    out = S.postprocess(boxes, "GREEDYNMM", "IOU", 0.4)
    np.testing.assert_allclose(out, np.array([A, B, D, C], np.float32))
    # class agnostic: C (same box as A) folds into A and keeps A's class; order is by score only
    out = S.postprocess(boxes, "GREEDYNMM", "IOS", 0.4, class_agnostic=True)
    np.testing.assert_allclose(out, np.array([[0, 0, 150, 100, .9, 0], D], np.float32))
    # NMS: same keep set, no union
    out = S.postprocess(boxes, "NMS", "IOS", 0.4)
    np.testing.assert_allclose(out, np.array([A, D, C], np.float32))
    # the growing box: E (.5) overlaps only the part B added; it joined A's list only if it matched A itself, so a box
    # that matches B but not A stays a detection of its own
    E = [110, 0, 150, 100, .5, 0]
    out = S.postprocess(np.array([A, B, E], np.float32), "GREEDYNMM", "IOS", 0.4)
    np.testing.assert_allclose(out, np.array([[0, 0, 150, 100, .9, 0], E], np.float32))
    # a member is re-tested against the grown box: F matches A (IOS .6 of F), and still matches after A grew
    F = [40, 0, 140, 100, .4, 0]
    out = S.postprocess(np.array([A, B, F], np.float32), "GREEDYNMM", "IOS", 0.4)
    np.testing.assert_allclose(out, np.array([[0, 0, 150, 100, .9, 0]], np.float32))
    assert S.postprocess(np.zeros((0, 6), np.float32)).shape == (0, 6)


def test_nmm_known_answers():
    """sahi's non-greedy `nmm`: a chain A-B-C (A~B, B~C, A and C apart).  GREEDYNMM: A takes B, C stays a detection.  NMM: B, already
    A's member, hands C to A as well -- and C is folded because the GROWN box A u B matches it."""
    A = [0, 0, 100, 100, .9, 0]; B = [60, 0, 160, 100, .8, 0]; C = [120, 0, 220, 100, .7, 0]; D = [500, 500, 600, 600, .6, 0]
    boxes = np.array([C, A, D, B], np.float32)   # IOS(A,B) = IOS(B,C) = .4, IOS(A,C) = 0
    assert S.nmm(boxes, "IOS", 0.3) == {1: [3, 0], 2: []}           # keeps A (index 1) and D; A's list: B (own turn), then C (B's turn)
    assert S.greedy_nmm(boxes, "IOS", 0.3) == {1: [3], 0: [], 2: []}
    out = S.postprocess(boxes, "NMM", "IOS", 0.3)
    np.testing.assert_allclose(out, np.array([[0, 0, 220, 100, .9, 0], D], np.float32))   # A u B = [0, 160]: IOS with C = .4 > .3
    out = S.postprocess(boxes, "GREEDYNMM", "IOS", 0.3)
    np.testing.assert_allclose(out, np.array([[0, 0, 160, 100, .9, 0], C, D], np.float32))
    # a member that the grown box does not match is dropped, not re-emitted (as in sahi): E touches only B's far end
    E = [150, 0, 400, 100, .5, 0]                # IOS(B, E) = 10 / 100 = .1, IOS(A u B, E) = 10 / 160 = .0625
    out = S.postprocess(np.array([A, B, E], np.float32), "NMM", "IOS", 0.08)
    np.testing.assert_allclose(out, np.array([[0, 0, 160, 100, .9, 0]], np.float32))
    # within one turn the matches are appended in ASCENDING score order (sahi flips the descending list)
    G = [10, 0, 110, 100, .5, 0]; H = [5, 0, 105, 100, .6, 0]
    assert S.nmm(np.array([A, G, H], np.float32), "IOS", 0.5) == {0: [1, 2]}
    # a keeper is never handed to another keeper: K2 matches member M of K1 but not K1
    K1 = [0, 0, 100, 100, .9, 0]; K2 = [150, 0, 250, 100, .85, 0]; M = [80, 0, 180, 100, .5, 0]   # IOS(K1,M) = .2, IOS(K2,M) = .3
    assert S.nmm(np.array([K1, K2, M], np.float32), "IOS", 0.15) == {0: [2], 1: []}
    # NMM without overlaps is the identity in score order; LSNMS = NMS with IOU, and refuses IOS like sahi
    np.testing.assert_allclose(S.postprocess(np.array([D, A], np.float32), "NMM"), np.array([A, D], np.float32))
    np.testing.assert_allclose(S.postprocess(boxes, "LSNMS", "IOU", 0.2), S.postprocess(boxes, "NMS", "IOU", 0.2))
    with pytest.raises(NotImplementedError):
        S.postprocess(boxes, "LSNMS", "IOS", 0.5)


def test_tile_detections_clamp_shift_and_drop():
    det = np.zeros((2, 3, 6), np.float32)
    det[0, 0] = [-5, 10, 50, 60, .9, 1]       # negative clamped to 0
    det[0, 1] = [30, 30, 30, 80, .8, 1]       # zero width -> dropped
    det[0, 2] = [1, 1, 2, 2, .7, 1]           # beyond counts[0] = 2 -> ignored
    det[1, 0] = [600, 10, 700, 90, .6, 2]     # clamped to the full width 640 (in tile coordinates, as sahi does)
    out = S.tile_detections(det, [2, 1], [[0, 0], [100, 200]], full_shape=(480, 640))
    np.testing.assert_allclose(out, np.array([[0, 10, 50, 60, .9, 1], [700, 210, 740, 290, .6, 2]], np.float32))


# ----------------------------------------------------------------------------------------------------------------------
# GPU: kernels against the oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("half", [True, False])
@pytest.mark.parametrize("hw,tile,swap", [((777, 1001), (64, 128), True), ((640, 640), (640, 640), True),
                                          ((131, 259), (32, 68), False)])
def test_slice_tiles_bit_exact(hw, tile, swap, half):
    from bs_yolo_amd import sahi as HS
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)
    b = S.get_slice_bboxes(hw[0], hw[1], tile[0], tile[1], 0.2, 0.1)
    got = HS.slice_image(img, b, half=half, swap_rb=swap, device=DEV)
    torch.cuda.synchronize()
    ref = torch.from_numpy(S.slice_image(img, b, swap_rb=swap))
    if half:  # `im.half(); im /= 255` (engine/predictor.py:131-133)
        t = torch.from_numpy(np.stack([img[y0:y1, x0:x1][..., ::-1 if swap else 1].transpose(2, 0, 1) for x0, y0, x1, y1 in b]).copy())
        ref = t.half() / 255
    assert got.dtype == ref.dtype and torch.equal(got.cpu(), ref)


@pytest.mark.gpu
def test_slice_tiles_rejects_bad_arguments():
    from bs_yolo_amd import sahi as HS
    from bs_yolo_amd.lib import BsyError
    img = np.zeros((100, 100, 3), np.uint8)
    with pytest.raises(ValueError):
        HS.slice_image(img, [[0, 0, 64, 64], [0, 0, 32, 64]], device=DEV)       # two sizes
    with pytest.raises(ValueError):
        HS.slice_image(img, [[50, 50, 114, 114]], device=DEV)                   # leaves the image
    with pytest.raises(BsyError):
        HS.slice_image(img, [[0, 0, 30, 64]], device=DEV)                       # tw % 4


def _tile_dets(T, max_det, n_obj, seed, nc=3, tile=640, cols=10, fill=1.0):
    """Synthetic per-tile NMS outputs: objects scattered over the full image, every tile sees the part of each object that
    falls inside it (plus jitter), so neighbouring tiles hold overlapping fragments -- the situation GREEDYNMM exists for."""
    rng = np.random.default_rng(seed)
    rows = -(-T // cols)
    W, H = cols * tile, rows * tile
    shifts = [[(t % cols) * tile, (t // cols) * tile] for t in range(T)]
    cx, cy = rng.uniform(0, W, n_obj), rng.uniform(0, H, n_obj)
    w, h = rng.uniform(20, 500, n_obj), rng.uniform(20, 500, n_obj)
    cls = rng.integers(0, nc, n_obj)
    det = np.zeros((T, max_det, 6), np.float32)
    counts = np.zeros(T, np.int32)
    for t, (ox, oy) in enumerate(shifts):
        x1 = np.clip(cx - w / 2 - ox, 0, tile); x2 = np.clip(cx + w / 2 - ox, 0, tile)
        y1 = np.clip(cy - h / 2 - oy, 0, tile); y2 = np.clip(cy + h / 2 - oy, 0, tile)
        vis = np.nonzero((x2 - x1 > 4) & (y2 - y1 > 4))[0]
        rep = np.repeat(vis, rng.integers(1, 3, vis.size))      # some fragments twice (NMS leftovers)
        rng.shuffle(rep)
        rep = rep[: int(max_det * fill)]
        n = rep.size
        jit = rng.normal(0, 3, (n, 4))
        bx = np.stack([x1[rep], y1[rep], x2[rep], y2[rep]], 1) + jit
        det[t, :n, :4] = bx
        det[t, :n, 4] = np.round(rng.uniform(0.25, 1.0, n), 2)    # 2 decimals: plenty of exact score ties
        det[t, :n, 5] = cls[rep]
        det[t, n:, :] = rng.uniform(0, 9, (max_det - n, 6))       # garbage beyond counts must be ignored
        counts[t] = n
    return det, counts, shifts, (H, W)


def _merge_both(det, counts, shifts, full, **kw):
    from bs_yolo_amd import sahi as HS
    ref = S.sliced_merge(det, counts, shifts, full, postprocess_type=kw.get("postprocess_type", "GREEDYNMM"),
                         metric=kw.get("match_metric", "IOS"), threshold=kw.get("match_threshold", 0.5),
                         class_agnostic=kw.get("class_agnostic", False))
    out, n = HS.postprocess(torch.from_numpy(det).to(DEV), torch.from_numpy(counts).to(DEV), shifts, full_shape=full, **kw)
    torch.cuda.synchronize()
    return ref, out[: int(n)].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [
    dict(),
    dict(match_metric="IOU", match_threshold=0.3),
    dict(class_agnostic=True),
    dict(postprocess_type="NMS", match_metric="IOU", match_threshold=0.5),
    dict(match_threshold=0.9),
    dict(match_metric="IOU", match_threshold=0.05, class_agnostic=True),
    dict(postprocess_type="NMM"),                                            # sahi's non-greedy merge (sahi_nmm_kernel)
    dict(postprocess_type="NMM", match_metric="IOU", match_threshold=0.2, class_agnostic=True),
    dict(postprocess_type="LSNMS", match_metric="IOU", match_threshold=0.5),  # runs as NMS
])
@pytest.mark.parametrize("T,max_det,n_obj,seed", [(1, 8, 3, 0), (4, 16, 12, 1), (12, 100, 150, 2), (70, 300, 1200, 3),
                                                  (2, 128, 600, 12), (70, 300, 4000, 4)])
def test_sahi_merge_bit_exact(T, max_det, n_obj, seed, kw):
    """Keep set, merge order, union boxes, scores, classes and output order equal the oracle's bit for bit, from one chunk
    (<= 256 candidates) to BASELINE config 5's 70 x 300 slots.  Valid candidates of the six cases: 1, 5, 235, 3318 (neither a
    multiple of the 256-candidate chunk), exactly 256 (one full chunk), and 10794 (> 8192: the key sort's global-memory path)."""
    det, counts, shifts, full = _tile_dets(T, max_det, n_obj, seed)
    ref, got = _merge_both(det, counts, shifts, full, **kw)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(got, ref), np.abs(got - ref).max()


@pytest.mark.gpu
def test_sahi_merge_edge_cases():
    from bs_yolo_amd import sahi as HS
    # no detections at all; every box invalid; a single box
    det = np.zeros((3, 5, 6), np.float32)
    _, got = _merge_both(det, np.zeros(3, np.int32), [[0, 0]] * 3, (100, 100))
    assert got.shape == (0, 6)
    det[0, 0] = [10, 10, 10, 50, .9, 0]
    det[1, 0] = [5, 5, 60, 70, .8, 2]
    ref, got = _merge_both(det, np.array([1, 1, 0], np.int32), [[0, 0], [640, 0], [0, 640]], (1280, 1280))
    assert np.array_equal(got, ref) and got.shape == (1, 6) and got[0, 0] == 645
    # all boxes identical, one class: one output;  identical boxes, all classes different: all survive
    det = np.zeros((2, 300, 6), np.float32)
    det[:, :, :4] = [10, 20, 110, 220]
    det[:, :, 4] = np.linspace(0.3, 0.9, 600).reshape(2, 300)
    ref, got = _merge_both(det, np.array([300, 300], np.int32), [[0, 0], [0, 0]], None)
    assert np.array_equal(got, ref) and got.shape == (1, 6) and got[0, 4] == np.float32(0.9)
    det[:, :, 5] = np.arange(600).reshape(2, 300)
    ref, got = _merge_both(det, np.array([300, 300], np.int32), [[0, 0], [0, 0]], None)
    assert np.array_equal(got, ref) and got.shape == (600, 6)
    # max_out truncates in keep order
    out, n = HS.postprocess(torch.from_numpy(det).to(DEV), torch.tensor([300, 300], dtype=torch.int32, device=DEV),
                            [[0, 0], [0, 0]], max_out=50)
    assert int(n) == 50 and np.array_equal(out.cpu().numpy(), ref[:50])
    with pytest.raises(Exception):
        HS.postprocess(torch.zeros((300, 300, 6), device=DEV), torch.zeros(300, dtype=torch.int32, device=DEV),
                       [[0, 0]] * 300)  # > 65536 slots


@pytest.mark.gpu
def test_sahi_merge_properties_at_full_size():
    """70 tiles x 300 full slots (21 000 candidates): class-ascending / score-descending order, no two kept ORIGINAL boxes
    of one class match (checked through a second NMS-type pass being the identity), GREEDYNMM keeps exactly the NMS keep
    set's scores, and the merged boxes contain the kept originals."""
    from bs_yolo_amd import sahi as HS
    det, counts, shifts, full = _tile_dets(70, 300, 4000, 7, nc=80, fill=1.0)
    d, c = torch.from_numpy(det).to(DEV), torch.from_numpy(counts).to(DEV)
    o1, n1 = HS.postprocess(d, c, shifts, "NMS", "IOS", 0.5, full_shape=full)
    o2, n2 = HS.postprocess(d, c, shifts, "GREEDYNMM", "IOS", 0.5, full_shape=full)
    n1, n2 = int(n1), int(n2)
    assert n1 == n2 and 100 < n1 < int(counts.sum())
    a, b = o1[:n1].cpu().numpy(), o2[:n2].cpu().numpy()
    key = a[:, 5] * 10 - a[:, 4]
    assert np.all(np.diff(key) >= 0)
    assert np.array_equal(a[:, 4:], b[:, 4:])
    assert np.all(b[:, :2] <= a[:, :2]) and np.all(b[:, 2:4] >= a[:, 2:4])
    # idempotence of the keep set: NMS over its own output keeps everything
    o3, n3 = HS.postprocess(o1[:n1][None].contiguous(), torch.tensor([n1], dtype=torch.int32, device=DEV), [[0, 0]], "NMS",
                            "IOS", 0.5)
    assert int(n3) == n1 and torch.equal(o3[:n1], o1[:n1])


@pytest.mark.gpu
def test_sliced_prediction_pipeline_matches_oracle():
    """Config-5 shape of work at an affordable size: YOLO11n over a 1500 x 1100 u8 image in 640-pixel tiles (3 x 2, border
    tiles shifted inwards), every stage on the device (tiles -> forward -> NMS -> cross-tile GREEDYNMM), against the same
    pipeline through the oracle.  NMS / merge decisions are discrete and fp16 storage moves scores by ~5e-3, so the bar
    is the one of the config-1 pipeline test: same count within 5 %, >= 90 % of the detections matched (same class, IoU >
    0.9, |dscore| < 1e-2)."""
    from bs_yolo_amd import sahi as HS
    from bs_yolo_amd.engine import YoloEngine
    from bs_yolo_amd.graphs import stock_cfg
    from oracle import postproc_ref as PP
    from oracle import val_ref as V
    from oracle import yolo_ref as R
    m = R.Model("yolo11", "n", 80, "detect")
    P = R.synth_params(m, 0)
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (1100, 1500, 3), dtype=np.uint8)
    bb = S.get_slice_bboxes(1100, 1500, 640, 640, 0.0, 0.0)
    assert len(bb) == 6
    xt = torch.from_numpy(S.slice_image(img, bb))
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.inference_mode():
        _, raw0 = m.forward(P, xt)
        top = torch.cat([r[:, 64:].flatten(2) for r in raw0], 2).amax(1).flatten()
        shift = float(np.log(0.25 / 0.75) - torch.quantile(top, 0.99))
        for k in P:
            if ".cv3." in k and k.endswith(".2.bias"):
                P[k] = P[k] + shift
        yr, _ = m.forward(P, xt)
    dets = PP.non_max_suppression(yr.clone(), 0.25, 0.7)
    det = np.zeros((6, 300, 6), np.float32)
    cnt = np.zeros(6, np.int32)
    for t, d in enumerate(dets):
        det[t, : d.shape[0]] = d.numpy(); cnt[t] = d.shape[0]
    ref = S.sliced_merge(det, cnt, [[b[0], b[1]] for b in bb], (1100, 1500))
    eng = YoloEngine(stock_cfg("yolo11", "n"), P, autotune=False)
    got, bb2 = HS.get_sliced_prediction(img, eng, 640, 640, 0.0, 0.0, perform_standard_pred=False, conf=0.25, iou=0.7)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert bb2 == bb
    assert 20 <= ref.shape[0] and abs(got.shape[0] - ref.shape[0]) <= max(2, ref.shape[0] // 20), (got.shape, ref.shape)
    iou = V.box_iou(ref[:, :4], got[:, :4]) * (ref[:, 5:6] == got[:, 5][None])
    j = iou.argmax(1)
    ok = (iou.max(1) > 0.9) & (np.abs(ref[:, 4] - got[j, 4]) < 1e-2)
    assert ok.mean() >= 0.9, (ok.mean(), got.shape, ref.shape)
    # with the full-image prediction added (sahi's perform_standard_pred): runs, and only adds or merges detections
    got2, _ = HS.get_sliced_prediction(img, eng, 640, 640, 0.0, 0.0, perform_standard_pred=True, conf=0.25, iou=0.7)
    assert got2.shape[1] == 6 and got2.shape[0] >= 1
    eng.close()


@pytest.mark.gpu
def test_sliced_prediction_config5_full_size():
    """BASELINE config 5 at full size on one GPU: YOLO11x, one seeded 6000 x 4000 u8 image -> 70 tiles of 640 x 640 ->
    forward + NMS -> cross-tile merge.  The 70-tile CPU forward (13.6 TFLOP) is out of reach for a test, so the forward is
    covered by test_engine_yolo11x_config5_crops and this test checks the full-size plumbing: tile pixels against the
    oracle's crops, and the merge of the GPU's own 70 x 300 detections against the oracle merge, bit for bit."""
    from bs_yolo_amd import sahi as HS
    from bs_yolo_amd import nms as HN
    from bs_yolo_amd.engine import YoloEngine
    from bs_yolo_amd.graphs import stock_cfg
    from oracle import yolo_ref as R
    m = R.Model("yolo11", "x", 80, "detect")
    P = {n: (v * 0.8 if n.endswith("bn.weight") else v) for n, v in R.synth_params(m, 5).items()}
    img = torch.randint(0, 256, (4000, 6000, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).numpy()
    bb = HS.get_slice_bboxes(4000, 6000, 640, 640, 0, 0)
    assert len(bb) == 70
    tiles = HS.slice_image(img, bb, device=DEV)
    for t in (0, 9, 33, 69):
        x0, y0, x1, y1 = bb[t]
        ref = torch.from_numpy(img[y0:y1, x0:x1, ::-1].transpose(2, 0, 1).copy()).half() / 255
        assert torch.equal(tiles[t].cpu(), ref)
    eng = YoloEngine(stock_cfg("yolo11", "x"), P, autotune=False)
    y, raws = eng(tiles, want_raw=True)
    # calibrate the class scores so that ~1 % of the anchors pass conf 0.25 (as bench.py does for its workload)
    top = torch.cat([r[:, 64:].flatten(2) for r in raws], 2).amax(1).float().flatten()
    thr = float(torch.quantile(top[torch.randperm(top.numel(), device=top.device)[:1_000_000]], 0.99))
    y[:, 4:] = torch.sigmoid(torch.logit(y[:, 4:].float().clamp(1e-6, 1 - 1e-6)) - thr + float(np.log(0.25 / 0.75))).half()
    det, cnt = HN.nms_batched(y, 0.25, 0.7, max_det=300)
    out, n = HS.postprocess(det, cnt, [[b[0], b[1]] for b in bb], full_shape=(4000, 6000))
    torch.cuda.synchronize()
    n = int(n)
    assert int(cnt.sum()) > 500 and 0 < n <= int(cnt.sum())
    ref = S.sliced_merge(det.cpu().numpy(), cnt.cpu().numpy(), [[b[0], b[1]] for b in bb], (4000, 6000))
    assert ref.shape[0] == n and np.array_equal(out[:n].cpu().numpy(), ref)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hw,slice_hw,imgsz", [((900, 1300), (500, 500), 320), ((300, 700), (800, 800), None), ((640, 1280), (640, 640), 320)])
def test_sliced_prediction_letterboxes_slices_like_the_predictor(hw, slice_hw, imgsz):
    """The reference's flow -- sahi hands every slice to the ultralytics predictor, which letterboxes it to imgsz and scales the boxes
    back (detect-sahi.py: 800 x 800 slices at imgsz 640) -- for slice sizes that are not multiples of 32, slices larger than the image
    (they shrink to it) and an explicit imgsz: equal, bit for bit, to the same stages called one by one (preprocess -> engine -> NMS ->
    scale_boxes -> merge), each of which has its own parity test."""
    from bs_yolo_amd import letterbox as HLB, nms as HN, sahi as HS
    from bs_yolo_amd.engine import YoloEngine
    from bs_yolo_amd.graphs import stock_cfg
    from oracle import yolo_ref as R
    m = R.Model("yolo11", "n", 80, "detect")
    P = R.synth_params(m, 0)
    for k in P:
        if ".cv3." in k and k.endswith(".2.bias"):
            P[k] = P[k] + 2.5
    eng = YoloEngine(stock_cfg("yolo11", "n"), P, autotune=False)
    H, W = hw
    img = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    out, bboxes = HS.get_sliced_prediction(img, eng, slice_hw[0], slice_hw[1], 0.2, 0.2, perform_standard_pred=False, imgsz=imgsz,
                                           batch=3)
    assert bboxes == S.get_slice_bboxes(H, W, slice_hw[0], slice_hw[1], 0.2, 0.2)
    assert all(b[2] <= W and b[3] <= H for b in bboxes)
    size = imgsz or 640
    dimg = torch.from_numpy(img).to(DEV)
    dets, cnts = [], []
    for x0, y0, x1, y1 in bboxes:
        t = HLB.preprocess([dimg[y0:y1, x0:x1]], imgsz=(size, size), half=True, device=DEV)
        d, c = HN.nms_batched(eng(t, want_raw=False)[0], 0.25, 0.7, max_det=300)
        HN.scale_boxes_batched(d, c, t.shape[2:], [(y1 - y0, x1 - x0)])
        dets.append(d)
        cnts.append(c)
    ref, n = HS.postprocess(torch.cat(dets), torch.cat(cnts), [[b[0], b[1]] for b in bboxes], full_shape=(H, W))
    n = int(n)
    assert n > 0 and out.shape == (n, 6) and torch.equal(out, ref[:n])
    assert float(out[:, 2].max()) <= W and float(out[:, 3].max()) <= H
    eng.close()
