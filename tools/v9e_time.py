#!/usr/bin/env python3
"""YOLOv9e on one GPU, fp16, 640 x 640, nc = 80: ms per forward, and the five CBFUSE launches (layers 16, 18, 21, 24, 27) against their
algorithmic bytes -- the destination written once, the last input read once, every tap read once AT ITS OWN RESOLUTION (the 4^k
re-reads of a coarse tap's pixel are cache traffic) -- and against what the measured HBM copy rate (6.29 TB/s, a float4 copy) would give.
Per-op device times of one forward come from YoloEngine.profile (bsy_plan_profile: HIP events around every op, serial).  One warm-up
forward (it also tunes the conv configurations), then the median of --runs profiles and of --runs timed windows of --window forwards.
Synthetic weights (weights.synth_state_dict); prints a table and one JSON line.

    python tools/v9e_time.py [--batch 8] [--runs 7] [--window 10] [--out FILE.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bs_yolo_amd import lib as L  # noqa: E402
from bs_yolo_amd.engine import YoloEngine  # noqa: E402
from bs_yolo_amd.graphs import stock_cfg  # noqa: E402
from bs_yolo_amd.plan import Plan  # noqa: E402
from bs_yolo_amd.weights import synth_state_dict  # noqa: E402

DEV = "cuda:0"
NC, SIZE = 80, 640
HBM_TBS = 6.29  # measured copy rate of the part (a float4 copy), not the 8 TB/s of the data sheet


def wall_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def cbfuse_bytes(plan, o):
    """Algorithmic bytes of one CBFUSE op: dst written, last read, each tap read at its own resolution (fp16: 2 bytes an element)."""
    esz = 4 if plan.f32_mode else 2
    px = plan.B * o["H"] * o["W"]
    taps = list(o["box"]) + list(o.get("cls", []))
    return esz * o["dst"].C * (2 * px + sum(plan.B * t.H * t.W for t in taps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = stock_cfg("yolov9e", None, NC)
    sd = synth_state_dict(Plan(cfg, 1, 64, 64), 0)
    x = torch.rand(a.batch, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(0)).half().to(DEV)
    eng = YoloEngine(cfg, sd)
    eng(x)  # warm-up: builds the plan, tunes the convs
    torch.cuda.synchronize()
    profs = []
    for _ in range(a.runs):
        ops, plan = eng.profile(x)
        profs.append([t for _, _, t in ops])
    med = [statistics.median(p[i] for p in profs) for i in range(len(ops))]
    assert len(med) == len(plan.ops)

    def burst():
        for _ in range(a.window):
            eng(x)

    fwd = statistics.median(wall_ms(burst) for _ in range(a.runs)) / a.window
    arena = int(L.lib.bsy_engine_arena_bytes(eng._h))
    eng.close()
    rows = []
    print(f"yolov9e fp16 {SIZE} x {SIZE} batch {a.batch}: forward {fwd:.3f} ms ({a.batch / fwd * 1e3:.1f} images/s), {len(plan.ops)} ops, "
          f"sum of op times {sum(med):.3f} ms, arena {arena / 2 ** 20:.0f} MiB")
    print(f"{'op':10s} {'taps':>4s} {'map':>13s} {'MB':>8s} {'us':>8s} {'GB/s':>8s} {'us at %.2f TB/s' % HBM_TBS:>18s}")
    for o, t in zip(plan.ops, med):
        if o["kind"] != L.OP_CBFUSE:
            continue
        nbytes = cbfuse_bytes(plan, o)
        roof_us = nbytes / (HBM_TBS * 1e12) * 1e6
        rows.append({"op": o["name"], "taps": o["nl"], "H": o["H"], "W": o["W"], "C": o["dst"].C, "bytes": nbytes, "us": round(t * 1e3, 2),
                     "gb_per_s": round(nbytes / (t * 1e-3) / 1e9, 1), "roof_us": round(roof_us, 2)})
        r = rows[-1]
        print(f"{r['op']:10s} {r['taps']:4d} {'%dx%dx%d' % (r['H'], r['W'], r['C']):>13s} {nbytes / 1e6:8.2f} {r['us']:8.2f} {r['gb_per_s']:8.1f} {roof_us:18.2f}")
    res = {"workload": f"yolov9e, fp16, {SIZE} x {SIZE}, nc {NC}, batch {a.batch}, synthetic weights; per-op times from YoloEngine.profile, "
           f"forward_ms = a window of {a.window} forwards / {a.window}", "runs": a.runs, "forward_ms": round(fwd, 4),
           "images_per_s": round(a.batch / fwd * 1e3, 1), "ops": len(plan.ops), "sum_ops_ms": round(sum(med), 4), "arena_bytes": arena,
           "hbm_tb_per_s": HBM_TBS, "cbfuse": rows, "cbfuse_us": round(sum(r["us"] for r in rows), 2),
           "cbfuse_roof_us": round(sum(r["roof_us"] for r in rows), 2)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
