#!/usr/bin/env python3
"""YOLOv8-ghost on one GPU, fp16: the one-launch GhostConv (BSY_OP_GHOST, csrc/ghost_fused.hip; BSY_FUSE_GHOST=1) against the plain chain
CONV 1x1 -> DWCONV_G 5x5 (-> ADD) (BSY_FUSE_GHOST=0).  Two engines of the same model in one process, one per setting; after a warm-up
of both (which also tunes the conv configurations) the forwards are timed in alternating rounds -- fused, chain, fused, chain ... --
with device events around --reps forwards each, so both see the same box at the same time.  Per batch: the median and the
spread (min .. max) of the rounds, and whether the outputs are the same bits.  Then the per-op device times of both plans
(YoloEngine.profile, median of the rounds): every OP_GHOST beside the ops of the chain it replaces, the widest and the narrowest
named.  Synthetic weights (weights.synth_state_dict), nc = 80; prints tables and one JSON line.

    python tools/ghost_time.py [--scale s] [--size 640] [--batches 64,1] [--rounds 7] [--reps 20] [--out FILE.json]"""
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


def wall_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def engines(cfg, sd, x):
    """{"fused": engine, "chain": engine}, each warmed up on x under its own BSY_FUSE_GHOST (a Plan reads it when it is built)."""
    out = {}
    for name, env in (("fused", "1"), ("chain", "0")):
        os.environ["BSY_FUSE_GHOST"] = env
        eng = YoloEngine(cfg, sd)
        for _ in range(3):
            eng(x, want_raw=False)
        torch.cuda.synchronize()
        plan = eng.plan_for(x.shape[0], x.shape[2], x.shape[3], x.dtype, x.dtype)[0]
        assert any(o["kind"] == L.OP_GHOST for o in plan.ops) == (env == "1")
        out[name] = eng
    os.environ.pop("BSY_FUSE_GHOST")
    return out


def forward_times(engs, x, rounds, reps):
    ms = {k: [] for k in engs}
    for _ in range(rounds):
        for k, eng in engs.items():  # alternating
            ms[k].append(wall_ms(lambda: eng(x, want_raw=False), reps))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}


def per_op(engs, x, rounds):
    """Per OP_GHOST of the fused plan: its device time and the summed time of the chain plan's ops of the same GhostConv."""
    med = {}
    for k, eng in engs.items():
        runs = []
        for _ in range(rounds):
            ops, plan = eng.profile(x)
            runs.append([t for _, _, t in ops])
        med[k] = ([statistics.median(r[i] for r in runs) for i in range(len(plan.ops))], plan)
    (tf, pf), (tc, pc) = med["fused"], med["chain"]
    rows = []
    for t, o in zip(tf, pf.ops):
        if o["kind"] != L.OP_GHOST:
            continue
        parts = [(u, c) for u, c in zip(tc, pc.ops) if c["name"].startswith(o["name"] + ".")]
        rows.append({"name": o["name"], "H": o["H"], "W": o["W"], "Cin": o["src0"].C, "CH": o["mid_c"], "res": o["res"] is not None,
                     "fused_us": round(1e3 * t, 2), "chain_us": round(1e3 * sum(u for u, _ in parts), 2), "chain_launches": len(parts)})
    return rows, round(sum(tf), 4), round(sum(tc), 4), len(pf.ops), len(pc.ops)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", default="s")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ghost_time.py measures on the GPU"
    cfg = stock_cfg("yolov8-ghost", a.scale, 80)
    sd = synth_state_dict(Plan(cfg, 1, 64, 64), 0)
    res = {"workload": f"yolov8{a.scale}-ghost fp16, nc 80, synthetic weights, {a.size} x {a.size}", "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "batches": []}
    for B in (int(b) for b in a.batches.split(",")):
        x = torch.rand(B, 3, a.size, a.size, generator=torch.Generator().manual_seed(0)).half().to(DEV)
        engs = engines(cfg, sd, x)
        same = torch.equal(engs["fused"](x, want_raw=False)[0], engs["chain"](x, want_raw=False)[0])
        reps = a.reps if B > 8 else 5 * a.reps
        fw = forward_times(engs, x, a.rounds, reps)
        rows, sum_f, sum_c, nf, nc_ = per_op(engs, x, a.rounds)
        r = {"batch": B, "same_bits": same, "reps": reps, "forward": fw, "ops": {"fused": nf, "chain": nc_},
             "sum_ops_ms": {"fused": sum_f, "chain": sum_c}, "ghost_ops": rows}
        res["batches"].append(r)
        print(f"batch {B}: same bits {same}; forward ms (median, min .. max of {a.rounds} alternating rounds of {reps})")
        for k in ("fused", "chain"):
            print(f"  {k:5s} {fw[k]['median_ms']:9.4f}  {fw[k]['min_ms']:9.4f} .. {fw[k]['max_ms']:9.4f}   {r['ops'][k]:3d} ops, sum of op times {r['sum_ops_ms'][k]:.4f} ms")
        print(f"  {'GhostConv':28s} {'map':>9s} {'Cin':>4s} {'CH':>4s} {'res':>4s} {'fused us':>9s} {'chain us':>9s} {'launches':>8s}")
        for g in rows:
            print(f"  {g['name']:28s} {g['H']:4d}x{g['W']:<4d} {g['Cin']:4d} {g['CH']:4d} {int(g['res']):4d} {g['fused_us']:9.2f} {g['chain_us']:9.2f} {g['chain_launches']:8d}")
        wide, narrow = max(rows, key=lambda g: g["Cin"] * g["CH"]), min(rows, key=lambda g: g["Cin"] * g["CH"])
        print(f"  widest {wide['name']}: {wide['fused_us']} vs {wide['chain_us']} us; narrowest {narrow['name']}: {narrow['fused_us']} vs {narrow['chain_us']} us;"
              f" all GhostConvs {sum(g['fused_us'] for g in rows):.1f} vs {sum(g['chain_us'] for g in rows):.1f} us", flush=True)
        for eng in engs.values():
            eng.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
