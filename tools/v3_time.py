#!/usr/bin/env python3
"""YOLOv3 on one GPU, fp16.  (1) yolov3-tiny: the image conv with the max pool in its epilogue (BSY_OP_FIRST_POOL, csrc/conv_first.hip;
BSY_FUSE_FIRST_POOL=1) against the chain CONV_FIRST stride 1 -> MAXPOOL (BSY_FUSE_FIRST_POOL=0).  Two engines of the same model in one
process, one per setting; after a warm-up of both (which also tunes the conv configurations) the forwards are timed in alternating
rounds -- fused, chain, fused, chain ... -- with device events around --reps forwards each, so both see the same box at the same time.
Per batch: the median and the spread (min .. max) of the rounds, whether the outputs are the same bits, and the per-op device times of
the stem of both plans (YoloEngine.profile, median of the rounds) beside the bytes each form stores.  (2) One line per family of
--families at the first batch: the forward, its conv GFLOPs and TFLOP/s.  Synthetic weights (weights.synth_state_dict), nc = 80; prints
tables and one JSON line.

    python tools/v3_time.py [--size 640] [--batches 64,1] [--families yolov3] [--rounds 7] [--reps 20] [--out FILE.json]"""
import argparse
import json
import os
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
ENV = "BSY_FUSE_FIRST_POOL"


def wall_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def engines(cfg, sd, x):
    """{"fused": engine, "chain": engine}, each warmed up on x under its own BSY_FUSE_FIRST_POOL (a Plan reads it when it is built)."""
    out = {}
    for name, env in (("fused", "1"), ("chain", "0")):
        os.environ[ENV] = env
        eng = YoloEngine(cfg, sd)
        for _ in range(3):
            eng(x, want_raw=False)
        torch.cuda.synchronize()
        plan = eng.plan_for(x.shape[0], x.shape[2], x.shape[3], x.dtype, x.dtype)[0]
        assert any(o["kind"] == L.OP_FIRST_POOL for o in plan.ops) == (env == "1")
        out[name] = eng
    os.environ.pop(ENV)
    return out


def forward_times(engs, x, rounds, reps):
    ms = {k: [] for k in engs}
    for _ in range(rounds):
        for k, eng in engs.items():  # alternating
            ms[k].append(wall_ms(lambda: eng(x, want_raw=False), reps))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}


def stem_ops(engs, x, rounds):
    """Per plan: the ops in front of model.2 (FIRST_POOL, or CONV_FIRST + MAXPOOL) with their device time and the bytes they store."""
    out, sums = {}, {}
    for k, eng in engs.items():
        runs = []
        for _ in range(rounds):
            ops, plan = eng.profile(x)
            runs.append([t for _, _, t in ops])
        med = [statistics.median(r[i] for r in runs) for i in range(len(plan.ops))]
        n = next(i for i, o in enumerate(plan.ops) if o["name"] == "model.2")
        out[k] = [{"name": o["name"], "us": round(1e3 * t, 2), "stored_MB": round(x.shape[0] * o["OH"] * o["OW"] * o["dst"].ld * 2 / 1e6, 1)}
                  for t, o in zip(med[:n], plan.ops[:n])]
        sums[k] = round(sum(med), 4)
    return out, sums


def one_line(family, B, size, reps, rounds):
    cfg = stock_cfg(family, None, 80)
    eng = YoloEngine(cfg, synth_state_dict(Plan(cfg, 1, 64, 64), 0))
    x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(0)).half().to(DEV)
    for _ in range(3):
        eng(x, want_raw=False)
    torch.cuda.synchronize()
    ms = [wall_ms(lambda: eng(x, want_raw=False), reps) for _ in range(rounds)]
    plan = eng.plan_for(B, size, size, x.dtype, x.dtype)[0]
    gf = plan.flops / 1e9
    med = statistics.median(ms)
    eng.close()
    return {"family": family, "batch": B, "ops": len(plan.ops), "conv_gflop": round(gf, 1), "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "tflops": round(gf / med, 1), "img_per_s": round(1e3 * B / med, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--families", default="yolov3")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "v3_time.py measures on the GPU"
    cfg = stock_cfg("yolov3-tiny", None, 80)
    sd = synth_state_dict(Plan(cfg, 1, 64, 64), 0)
    batches = [int(b) for b in a.batches.split(",")]
    res = {"workload": f"yolov3-tiny fp16, nc 80, synthetic weights, {a.size} x {a.size}", "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "batches": [], "families": []}
    for B in batches:
        x = torch.rand(B, 3, a.size, a.size, generator=torch.Generator().manual_seed(0)).half().to(DEV)
        engs = engines(cfg, sd, x)
        same = torch.equal(engs["fused"](x, want_raw=False)[0], engs["chain"](x, want_raw=False)[0])
        reps = a.reps if B > 8 else 5 * a.reps
        fw = forward_times(engs, x, a.rounds, reps)
        stem, sums = stem_ops(engs, x, a.rounds)
        res["batches"].append({"batch": B, "same_bits": same, "reps": reps, "forward": fw, "sum_ops_ms": sums, "stem_ops": stem})
        print(f"batch {B}: same bits {same}; forward ms (median, min .. max of {a.rounds} alternating rounds of {reps})")
        for k in ("fused", "chain"):
            print(f"  {k:5s} {fw[k]['median_ms']:9.4f}  {fw[k]['min_ms']:9.4f} .. {fw[k]['max_ms']:9.4f}   sum of op times {sums[k]:.4f} ms; stem: "
                  + ", ".join(f"{o['name']} {o['us']} us ({o['stored_MB']} MB stored)" for o in stem[k]), flush=True)
        for eng in engs.values():
            eng.close()
    for fam in [f for f in a.families.split(",") if f]:
        r = one_line(fam, batches[0], a.size, a.reps, a.rounds)
        res["families"].append(r)
        print(f"{r['family']} batch {r['batch']}: {r['median_ms']} ms ({r['min_ms']} .. {r['max_ms']}), {r['ops']} ops, {r['conv_gflop']} conv GFLOP per image x batch, "
              f"{r['tflops']} TFLOP/s, {r['img_per_s']} img/s", flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
