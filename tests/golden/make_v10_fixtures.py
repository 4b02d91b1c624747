#!/usr/bin/env python3
"""Generate the YOLOv10 end-to-end top-k fixtures by RUNNING THE REFERENCE (build container only).

    python tests/golden/make_v10_fixtures.py

The reference is imported in-process with make_fixtures.py's stand-ins.  Nothing of the reference is modified or copied.
  v10_topk.npz  v10Detect.postprocess (nn/modules/head.py:151-172) -- Detect.postprocess(preds.permute(0, 2, 1), max_det, nc), as
           forward_end2end calls it (:96) -- on seeded synthetic (B, 4 + nc, A) predictions (CASES below).  The inputs regenerate
           from their seeds (topk_input; tests/test_v10_topk.py has the same function), so only their checksums and the output
           rows are stored.  f16 cases run the reference on the .half() tensor, as a half model does: it selects on the f16
           values and its rows come back f32 (torch.cat with the f32 class column).
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_fixtures as MF  # noqa: E402,F401  (stand-ins + the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ultralytics.nn.modules.head import v10Detect  # noqa: E402


def topk_input(B, nc, A, seed, dtype, tie_q=0):
    """Boxes in [0, 640), class scores spread over [0, 1) (cubed uniform); tie_q > 0 rounds the scores down to multiples of 1/tie_q,
    which makes exact ties everywhere, the K-th boundary included."""
    g = torch.Generator().manual_seed(seed)
    box = torch.rand(B, 4, A, generator=g) * 640
    sc = torch.rand(B, nc, A, generator=g) ** 3
    if tie_q:
        sc = torch.floor(sc * tie_q) / tie_q
    return torch.cat([box, sc], 1).to(dtype)


CASES = [  # tag, B, nc, A, max_det, seed, dtype, tie_q
    ("a_lt_maxdet", 2, 6, 150, 300, 1, "float32", 0),
    ("nc1", 2, 1, 700, 300, 2, "float32", 0),
    ("maxdet100", 2, 80, 2100, 100, 3, "float32", 0),
    ("a8400", 2, 80, 8400, 300, 4, "float32", 0),
    ("a8400_f16", 2, 80, 8400, 300, 5, "float16", 0),
    ("ties_f16", 2, 20, 1200, 64, 6, "float16", 32),
]


def topk_fixtures():
    out, meta = {}, []
    for tag, B, nc, A, md, seed, dt, q in CASES:
        x = topk_input(B, nc, A, seed, getattr(torch, dt), q)
        with torch.inference_mode():
            y = v10Detect.postprocess(x.permute(0, 2, 1), md, nc)
        assert y.dtype == torch.float32 and tuple(y.shape) == (B, min(md, A), 6)
        out[f"out_{tag}"] = y.numpy()
        meta.append({"tag": tag, "B": B, "nc": nc, "A": A, "max_det": md, "seed": seed, "dtype": dt, "tie_q": q,
                     "sum": float(x.double().sum()), "first": x.flatten()[:8].float().tolist()})
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(HERE / "v10_topk.npz", **out)


if __name__ == "__main__":
    topk_fixtures()
