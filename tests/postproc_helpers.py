"""Shared pieces of the NMS / mask parity tests (test_gpu_parity.py, test_postprocess_edges.py): input builders and the
comparison of the device non_max_suppression with oracle.postproc_ref.  Not a test module."""
import torch

from oracle import postproc_ref as PP

DEV = "cuda:0"


def rand_pred(B, nc, A, nm, seed, dup=True):
    g = torch.Generator().manual_seed(seed)
    base = max(A // 6, 1)
    c = torch.rand(B, 2, base, generator=g) * 600 + 20
    wh = torch.rand(B, 2, base, generator=g) * 120 + 8
    rep = (A + base - 1) // base
    box = torch.cat((c, wh), 1).repeat(1, 1, rep)[:, :, :A] + torch.randn(B, 4, A, generator=g) * (3.0 if dup else 50.0)
    box[:, 2:] = box[:, 2:].abs() + 1
    cls = torch.rand(B, nc, A, generator=g) ** 4
    parts = [box, cls] + ([torch.randn(B, nm, A, generator=g)] if nm else [])
    return torch.cat(parts, 1)


def nms_compare(pred, kw):
    """fp32: same list length, shapes, rows (torch.equal) and the same in-place xywh -> xyxy mutation.  Returns (got, ref)."""
    from bs_yolo_amd import nms as HN
    ref_in = pred.clone()
    ref = PP.non_max_suppression(ref_in, **kw)
    dpred = pred.clone().to(DEV)
    got = HN.non_max_suppression(dpred, **kw)
    torch.cuda.synchronize()
    assert len(got) == len(ref)
    if kw.get("in_place", True):
        assert torch.equal(dpred[:, :4].cpu(), ref_in[:, :4])  # same in-place xywh->xyxy mutation
    else:
        assert torch.equal(dpred.cpu(), pred)
    for b, (g_, r_) in enumerate(zip(got, ref)):
        assert tuple(g_.shape) == tuple(r_.shape), (b, g_.shape, r_.shape)
        assert torch.equal(g_.cpu(), r_), f"image {b}"
    return got, ref


def misaligned_view(pred16):
    """The same fp16 values on the device, contiguous, at an address that is 2 modulo 8 (one element into an allocation)."""
    flat = torch.empty(pred16.numel() + 1, dtype=torch.float16, device=DEV)
    v = flat[1:].view(pred16.shape)
    v.copy_(pred16)
    assert v.is_contiguous() and v.data_ptr() % 8 == 2
    return v


def fp16_reference(pred16, kw):
    """The fp16 convention: boxes converted in fp16 on the CPU (as the reference's in-place op does), decisions in fp32.
    Returns (prediction after the in-place conversion, list of fp32 rows)."""
    ref_in = pred16.clone()
    tp = ref_in.transpose(-1, -2)
    tp[..., :4] = PP.xywh2xyxy(tp[..., :4])  # fp16 arithmetic on the CPU
    kwr = {k: v for k, v in kw.items() if k != "in_place"}
    return ref_in, PP.non_max_suppression(ref_in.float(), boxes_xyxy=True, **kwr)


def nms_compare_fp16(pred16, kw, misaligned=False, reference=None):
    """fp16 predictions against fp16_reference: rows compared after .half().  Returns (got, ref)."""
    from bs_yolo_amd import nms as HN
    assert pred16.dtype == torch.float16
    dpred = misaligned_view(pred16) if misaligned else pred16.clone().to(DEV)
    got = HN.non_max_suppression(dpred, **kw)
    torch.cuda.synchronize()
    ref_in, ref = reference if reference is not None else fp16_reference(pred16, kw)
    if kw.get("in_place", True):
        assert torch.equal(dpred[:, :4].cpu(), ref_in[:, :4])
        assert torch.equal(dpred[:, 4:].cpu(), pred16[:, 4:])
    else:
        assert torch.equal(dpred.cpu(), pred16)
    assert len(got) == len(ref)
    for b, (g_, r_) in enumerate(zip(got, ref)):
        assert tuple(g_.shape) == tuple(r_.shape), (b, g_.shape, r_.shape)
        if len(r_):
            assert g_.dtype == torch.float16
        assert torch.equal(g_.float().cpu(), r_.half().float()), f"image {b}"
    return got, ref
