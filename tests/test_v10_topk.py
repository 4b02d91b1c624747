"""The NMS-free end-to-end top-k of YOLOv10 (v10Detect.postprocess, nn/modules/head.py:151-172) as a device op, bsy_end2end_topk
(csrc/topk.hip), against fixtures made by running the reference (tests/golden/make_v10_fixtures.py) and against a host model of
the documented tie rule (higher score, then lower anchor, then lower class)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from bs_yolo_amd import lib as L

DEV = "cuda:0"


def topk_input(B, nc, A, seed, dtype, tie_q=0):
    """make_v10_fixtures.topk_input: the fixtures' predictions regenerated from their seeds."""
    g = torch.Generator().manual_seed(seed)
    box = torch.rand(B, 4, A, generator=g) * 640
    sc = torch.rand(B, nc, A, generator=g) ** 3
    if tie_q:
        sc = torch.floor(sc * tie_q) / tie_q
    return torch.cat([box, sc], 1).to(dtype)


def _cases():
    z = np.load(GOLDEN / "v10_topk.npz")
    return z, json.loads(str(z["meta"]))


def _input(c):
    x = topk_input(c["B"], c["nc"], c["A"], c["seed"], getattr(torch, c["dtype"]), c["tie_q"])
    assert abs(float(x.double().sum()) - c["sum"]) < 1e-6 * x.numel() and x.flatten()[:8].float().tolist() == c["first"]
    return x


def host_topk(x: np.ndarray, max_det: int) -> np.ndarray:
    """The two-stage selection with bsy_end2end_topk's tie rule, on the host: x (B, 4+nc, A) of the stored values."""
    x = x.astype(np.float64)
    B, Cc, A = x.shape
    nc, K = Cc - 4, min(max_det, A)
    out = np.zeros((B, K, 6), np.float32)
    for b in range(B):
        sc = x[b, 4:]
        sel = np.lexsort((np.arange(A), -sc.max(0)))[:K]              # stage 1: amax desc, anchor asc
        s = sc[:, sel].T.ravel()                                       # (K, nc) anchor-rank-major, as the reference flattens
        a = np.repeat(sel, nc)
        c = np.tile(np.arange(nc), K)
        o = np.lexsort((c, a, -s))[:K]                                 # stage 2: score desc, anchor asc, class asc
        out[b, :, :4] = x[b, :4][:, a[o]].T
        out[b, :, 4] = s[o]
        out[b, :, 5] = c[o]
    return out


def assert_matches_reference(got: np.ndarray, ref: np.ndarray):
    """Rows equal where the reference's order is defined: the score column exactly; every group of equal scores above the last one
    as a multiset of (box, score, class) -- an untied row is compared exactly; the last group by its scores only.
    Why only the last group is open, for any input: let v be the best-class score of stage 1's K-th anchor.  Every anchor stage 1
    keeps has a class score >= v, so stage 2 sees at least K scores >= v and its K-th score s is >= v.  Which of the anchors tied
    at v stage 1 keeps decides only scores <= v (their best is v).  Hence every row of score > s comes from anchors that any tie
    order keeps, and is the same multiset under any tie order; only the group at s -- stage 2's own boundary, and stage 1's when
    s == v -- depends on how ties fall."""
    assert got.shape == ref.shape
    for b in range(ref.shape[0]):
        assert np.array_equal(got[b, :, 4], ref[b, :, 4]), f"image {b}: score sequences differ"
        last = ref[b, -1, 4]
        for s in np.unique(ref[b, :, 4]):
            if s == last:
                continue
            g = sorted(map(tuple, got[b][got[b, :, 4] == s].tolist()))
            r = sorted(map(tuple, ref[b][ref[b, :, 4] == s].tolist()))
            assert g == r, f"image {b}: rows of score {s} differ"


# ---- host side (no GPU) ------------------------------------------------------------------------------------------------
def test_end2end_topk_is_declared_and_bound():
    header = (ROOT / "include" / "bsyolo.h").read_text()
    for s in ("bsy_end2end_topk_workspace_bytes", "bsy_end2end_topk"):
        assert s + "(" in header and s in L.SYMBOLS
    # stage-1 keys (B x A) + stage-2 keys (B x K x nc), each 256-aligned, + alignment slack
    assert L.lib.bsy_end2end_topk_workspace_bytes(16, 8400, 80, 300) == 256 + 16 * 8400 * 4 + 16 * 300 * 80 * 8
    assert L.lib.bsy_end2end_topk_workspace_bytes(1, 100, 3, 300) == 256 + 512 + 2560  # K = A when A < max_det
    assert L.lib.bsy_end2end_topk_workspace_bytes(0, 100, 3, 300) == 0


def test_end2end_topk_rejects_bad_arguments_before_any_launch():
    dummy = C.c_void_p(16)  # never dereferenced: every check below fails before a launch
    big = 1 << 40
    with pytest.raises(L.BsyError, match="null pointer"):
        L.check(L.lib.bsy_end2end_topk(None, L.BSY_F16, 1, 80, 8400, 300, dummy, dummy, big, None))
    with pytest.raises(L.BsyError, match="bad sizes"):
        L.check(L.lib.bsy_end2end_topk(dummy, L.BSY_F16, 1, 0, 8400, 300, dummy, dummy, big, None))
    with pytest.raises(L.BsyError, match="bad sizes"):
        L.check(L.lib.bsy_end2end_topk(dummy, L.BSY_F16, 0, 80, 8400, 300, dummy, dummy, big, None))
    with pytest.raises(L.BsyError, match="max_det"):
        L.check(L.lib.bsy_end2end_topk(dummy, L.BSY_F16, 1, 80, 8400, 0, dummy, dummy, big, None))
    with pytest.raises(L.BsyError, match="max_det"):
        L.check(L.lib.bsy_end2end_topk(dummy, L.BSY_F16, 1, 80, 8400, 4097, dummy, dummy, big, None))
    with pytest.raises(L.BsyError, match="too large"):
        L.check(L.lib.bsy_end2end_topk(dummy, L.BSY_F32, 1, 1 << 16, 1 << 15, 300, dummy, dummy, big, None))
    with pytest.raises(L.BsyError, match="too large"):  # A * nc = 2^30 + 2 (loop indices and key indices stay in int up to 2^30)
        L.check(L.lib.bsy_end2end_topk(dummy, L.BSY_F32, 1, 2, (1 << 29) + 1, 300, dummy, dummy, big, None))
    with pytest.raises(L.BsyError, match="workspace"):  # A * nc = 2^30 is in bounds: the next check is the workspace
        L.check(L.lib.bsy_end2end_topk(dummy, L.BSY_F32, 1, 2, 1 << 29, 300, dummy, dummy, 16, None))
    with pytest.raises(L.BsyError, match="dtype"):
        L.check(L.lib.bsy_end2end_topk(dummy, L.BSY_U8, 1, 80, 8400, 300, dummy, dummy, big, None))
    with pytest.raises(L.BsyError, match="workspace"):
        L.check(L.lib.bsy_end2end_topk(dummy, L.BSY_F16, 1, 80, 8400, 300, dummy, dummy, 1024, None))


@pytest.mark.parametrize("tag", ["a_lt_maxdet", "nc1", "maxdet100", "a8400", "a8400_f16", "ties_f16"])
def test_host_model_of_the_tie_rule_agrees_with_the_reference(tag):
    """The host model the GPU tests hold the kernel to is itself the reference's postprocess wherever that one is defined."""
    z, meta = _cases()
    c = next(m for m in meta if m["tag"] == tag)
    x = _input(c)
    assert_matches_reference(host_topk(x.float().numpy(), c["max_det"]), z[f"out_{tag}"])


def test_tie_fixture_ties_at_the_boundary():
    """ties_f16 exercises what it is for: equal scores inside the result and across its K-th row."""
    z, meta = _cases()
    c = next(m for m in meta if m["tag"] == "ties_f16")
    x = _input(c).float().numpy()
    ref = z["out_ties_f16"]
    for b in range(c["B"]):
        s = ref[b, :, 4]
        assert len(np.unique(s)) < len(s) - 4
        kth = s[-1]
        assert (x[b, 4:] == kth).sum() > (s == kth).sum()  # more candidates hold the K-th score than the result keeps


# ---- device ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["a_lt_maxdet", "nc1", "maxdet100", "a8400", "a8400_f16", "ties_f16"])
def test_end2end_topk_matches_the_reference(tag):
    from bs_yolo_amd import ops as O
    z, meta = _cases()
    c = next(m for m in meta if m["tag"] == tag)
    x = _input(c)
    got = O.end2end_topk(x.to(DEV), c["max_det"])
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (c["B"], min(c["max_det"], c["A"]), 6)
    got = got.cpu().numpy()
    assert_matches_reference(got, z[f"out_{tag}"])
    assert np.array_equal(got, host_topk(x.float().numpy(), c["max_det"]))  # ties resolved by the documented rule, bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("B,nc,A,md,q", [(16, 80, 8400, 300, 0), (4, 80, 33600, 300, 0), (3, 80, 33600, 300, 64), (2, 3, 5000, 4096, 16),
                                          (1, 80, 1, 300, 0), (2, 7, 999, 1, 0)])
def test_end2end_topk_equals_the_host_model(B, nc, A, md, q, dtype):
    """The sizes the engine serves (8 400 anchors at 640, 33 600 at 1280; 24 000 stage-2 candidates at nc = 80) and the edges
    (A = 1, max_det = 1, max_det at its bound of 4096), with and without ties, against the host model exactly."""
    from bs_yolo_amd import ops as O
    x = topk_input(B, nc, A, 1000 + A + nc + q, dtype, q)
    got = O.end2end_topk(x.to(DEV), md)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), host_topk(x.float().numpy(), md))


@pytest.mark.gpu
def test_end2end_topk_is_deterministic_and_replays_in_a_captured_graph():
    from bs_yolo_amd import ops as O
    x = topk_input(8, 80, 8400, 77, torch.float16, 128).to(DEV)
    eager = O.end2end_topk(x, 300)
    again = O.end2end_topk(x, 300)
    nbytes = L.lib.bsy_end2end_topk_workspace_bytes(8, 8400, 80, 300)
    out = torch.empty((8, 300, 6), dtype=torch.float32, device=DEV)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        O.end2end_topk(x, 300, out=out, workspace=ws)  # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        O.end2end_topk(x, 300, out=out, workspace=ws)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager, again) and torch.equal(out, eager)


@pytest.mark.gpu
def test_end2end_topk_wrapper_checks():
    from bs_yolo_amd import ops as O
    with pytest.raises(RuntimeError):
        O.end2end_topk(torch.zeros(1, 84, 100), 300)  # host tensor: no CPU fallback
    with pytest.raises(ValueError):
        O.end2end_topk(torch.zeros(1, 4, 100, device=DEV), 300)  # no class rows
    with pytest.raises(L.BsyError, match="max_det"):
        O.end2end_topk(torch.zeros(1, 84, 100, device=DEV), 5000)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_end2end_topk_rows_keep_the_stored_scores(dtype):
    """-0 ranks equal to +0 (ties go to the lower anchor, then class), and a row carries the stored score, sign included, as the
    reference's gather does."""
    from bs_yolo_amd import ops as O
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.rand(2, 4, 64, generator=g) * 640, torch.zeros(2, 3, 64)], 1)
    neg = torch.rand(2, 3, 64, generator=g) < 0.5
    x[:, 4:][neg] = -0.0
    x[:, 4:, 10:14] = 0.5
    x = x.to(dtype)
    got = O.end2end_topk(x.to(DEV), 40)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = host_topk(x.float().numpy(), 40)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))  # bit for bit: -0.0 stays -0.0
    assert np.signbit(got[..., 4]).any() and (got[..., 4] == 0.5).sum() == 2 * 12
