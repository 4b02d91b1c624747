#!/usr/bin/env python3
"""YOLOv6 on one GPU, fp16: what the conv kernels do once SiLU is gone.  Two engines of the same weights in one process: the graph as the
yaml has it (`activation: nn.ReLU()`: act = 2 on every activated conv, SPPF's two convs as --sppf-act says) and the same plan with every
act = 2 forced to 1 (the yaml without its `activation` key: the planner then emits the same ops, buffers and weight records with SiLU
everywhere).  csrc/common.h says the fp16 conv kernels' SIMDs are "~80 % busy issuing SiLU"; the difference of the two forwards is the
direct measurement of what that issue costs these kernels.  After a warm-up of both (which also tunes the conv configurations, each
engine its own: the activation is part of a conv's tuning signature) the forwards are timed in alternating rounds -- relu, silu, relu,
silu ... -- with device events around --reps forwards each, so both see the same box at the same time.  Per engine: the median and the
spread (min .. max) of the rounds, conv-family TFLOP/s from the plan's mfma_flops, the launch count, and the sum of the per-op device
times of the 3x3 chains, the other convs and the rest (YoloEngine.profile).  Synthetic weights (weights.synth_state_dict), nc = 80;
prints a table and one JSON line.

    python tools/v6_time.py [--scale s] [--size 640] [--batch 64] [--sppf-act silu] [--rounds 7] [--reps 10] [--out FILE.json]"""
import argparse
import json
import re
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


def wall_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def op_groups(eng, x, rounds):
    """Median device time per group of ops: the repeated 3x3 Convs (model.<i>.<j>), every other conv launch, everything else."""
    runs = []
    for _ in range(rounds):
        ops, plan = eng.profile(x)
        runs.append([t for _, _, t in ops])
    med = [statistics.median(r[i] for r in runs) for i in range(len(plan.ops))]
    out = {"chains_3x3": 0.0, "other_convs": 0.0, "rest": 0.0}
    for t, o in zip(med, plan.ops):
        if o["kind"] in (L.OP_CONV, L.OP_STEM, L.OP_CONV_FIRST):
            out["chains_3x3" if re.fullmatch(r"model\.\d+\.\d+", o["name"]) else "other_convs"] += t
        else:
            out["rest"] += t
    return {k: round(v, 4) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", default="s")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--sppf-act", default="silu")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "v6_time.py measures on the GPU"
    relu = stock_cfg("yolov6", a.scale, 80)
    silu = {k: v for k, v in relu.items() if k != "activation"}
    sd = synth_state_dict(Plan(relu, 1, 64, 64), 0)
    x = torch.rand(a.batch, 3, a.size, a.size, generator=torch.Generator().manual_seed(0)).half().to(DEV)
    engs = {"relu": YoloEngine(relu, sd, sppf_act=a.sppf_act), "silu": YoloEngine(silu, sd)}
    plans = {}
    for k, eng in engs.items():
        for _ in range(3):
            eng(x, want_raw=False)
        torch.cuda.synchronize()
        plans[k] = eng.plan_for(a.batch, a.size, a.size, x.dtype, x.dtype)[0]
    pr, ps = plans["relu"], plans["silu"]
    assert [(o["kind"], o["name"]) for o in pr.ops] == [(o["kind"], o["name"]) for o in ps.ops] and pr.buf_bytes == ps.buf_bytes
    assert all(p.get("act", 0) == (1 if r.get("act", 0) == 2 else r.get("act", 0)) for r, p in zip(pr.ops, ps.ops))
    ms = {k: [] for k in engs}
    for _ in range(a.rounds):
        for k, eng in engs.items():  # alternating
            ms[k].append(wall_ms(lambda: eng(x, want_raw=False), a.reps))
    res = {"workload": f"yolov6{a.scale} fp16, nc 80, synthetic weights, {a.batch} x {a.size} x {a.size}, sppf_act {a.sppf_act}", "rounds": a.rounds,
           "reps": a.reps, "device": torch.cuda.get_device_name(0), "engines": {}}
    for k, eng in engs.items():
        plan = plans[k]
        gf = sum(o.get("mfma_flops", 0) for o in plan.ops) / 1e9
        med = statistics.median(ms[k])
        acts = [o["act"] for o in plan.ops if o["kind"] in (L.OP_CONV, L.OP_STEM, L.OP_CONV_FIRST)]
        res["engines"][k] = {"median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4), "launches": len(plan.ops),
                             "conv_gflop": round(gf, 1), "tflops": round(gf / med, 1), "img_per_s": round(1e3 * a.batch / med, 1),
                             "convs_by_act": {str(i): acts.count(i) for i in sorted(set(acts))}, "op_time_ms": op_groups(eng, x, a.rounds)}
        r = res["engines"][k]
        print(f"{k}: {r['median_ms']} ms ({r['min_ms']} .. {r['max_ms']}), {r['launches']} launches, {r['conv_gflop']} conv GFLOP, {r['tflops']} TFLOP/s, "
              f"{r['img_per_s']} img/s; convs by act {r['convs_by_act']}; op times {r['op_time_ms']}", flush=True)
    d = res["engines"]["silu"]["median_ms"] - res["engines"]["relu"]["median_ms"]
    res["silu_minus_relu_ms"] = round(d, 4)
    print(f"SiLU costs {d:.4f} ms of {res['engines']['silu']['median_ms']} ms ({100 * d / res['engines']['silu']['median_ms']:.1f} %)")
    for eng in engs.values():
        eng.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
