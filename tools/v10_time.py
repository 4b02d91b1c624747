#!/usr/bin/env python3
"""YOLOv10s on one GPU, 640 x 640, batch 64 (default), fp16: ms per step from the image to the top-k rows, on the rows-only plan
(want_raw=False: no one2many branches) and on the plan with the one2many head (want_raw=True: both heads' raw maps come back too).
For scale, in the same process and the same alternating rounds: YOLOv8s forward + device NMS (bs_yolo_amd.nms.nms_batched, conf 0.25,
iou 0.7, max_det 300), the pipeline the NMS-free head replaces.  Weights are seeded synthetic ones (weights.synth_state_dict).

    python tools/v10_time.py [--batch 64] [--size 640] [--rounds 7] [--steps 20] [--warmup 5] [--out FILE.json]

Every round times each of the three once, `steps` calls between two device events after `warmup` calls; reported: the median of the
rounds with min .. max."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bs_yolo_amd.engine import YoloEngine  # noqa: E402
from bs_yolo_amd.graphs import stock_cfg  # noqa: E402
from bs_yolo_amd.nms import nms_batched  # noqa: E402
from bs_yolo_amd.plan import Plan  # noqa: E402
from bs_yolo_amd.weights import synth_state_dict  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def engine(family, scale, **kw):
    cfg = stock_cfg(family, scale)
    return YoloEngine(cfg, synth_state_dict(Plan(cfg, 1, 64, 64, one2many=True)), **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, S = a.batch, a.size
    v10, v8 = engine("yolov10", "s", max_det=300), engine("yolov8", "s")
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(0)).half().to("cuda:0")
    what = {
        "yolov10s_rows_only": lambda: v10(x, want_raw=False),
        "yolov10s_with_one2many": lambda: v10(x, want_raw=True),
        "yolov8s_forward_nms": lambda: nms_batched(v8(x, want_raw=False)[0], 0.25, 0.7, max_det=300),
    }
    for fn in what.values():  # autotune and first launches, before any round
        fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in what}
    for _ in range(a.rounds):
        for k, fn in what.items():
            rounds[k].append(timed(fn, a.steps, a.warmup))
    rows, _ = v10(x, want_raw=False)
    full, _ = v10(x, want_raw=True)
    torch.cuda.synchronize()
    res = {"workload": f"{S}x{S} bs={B} fp16", "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "same_rows_on_both_plans": bool(torch.equal(rows, full)),
           "ops": {"rows_only": len(v10.plan_for(B, S, S, x.dtype, x.dtype)[0].ops), "with_one2many": len(v10.plan_for(B, S, S, x.dtype, x.dtype, one2many=True)[0].ops)}}
    for k, v in rounds.items():
        res[k] = {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                  "images_per_s": round(B / statistics.median(v) * 1e3, 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    v10.close()
    v8.close()


if __name__ == "__main__":
    main()
