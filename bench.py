#!/usr/bin/env python3
"""Headline benchmark: images/sec of the YOLO11s 640x640 fp16 detection hot path (forward + NMS) on MI355X.

    python bench.py                                   # 1 GPU, defaults
    python bench.py --gpus N                          # N GPUs: starts the N ranks itself (a child torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W        # the same, launched by the caller: one rank per GPU (RCCL)
    python bench.py --imgsz 1280                      # the 1280 x 1280 line of the north-star
    python bench.py --gpus 8 --scaling strong --scale m --imgsz 1280 --batch 256   # BASELINE config 3: 256 images split 32 / GPU
    python bench.py --dump-outputs DIR                # also write the last timed step's outputs to DIR/*.npy (see dump_outputs)

One "step" = one pass of the hot path over one batch of synthetic images already resident in HBM:
engine forward (all HIP kernels) -> batched HIP NMS (conf 0.25, iou 0.7, max_det 300) -> (N > 1) RCCL all-gather of
the fixed-size detections over xGMI.  Images are independent units: by default each rank owns its own batch of 64 (weak
scaling); `--scaling strong` keeps the GLOBAL batch at --batch and gives every rank a contiguous share of it.  No
data-path collective besides the detection all-gather.

Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement" for how `roofline` and `cpu_baseline` are taken).
"""
import argparse
import json
import math
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

PEAK_MFMA_F16_TFLOPS = 2500.0  # MI355X dense fp16 MFMA (MI355X_MICROARCH.md, chip-level parameters)
PEAK_MFMA_F32_TFLOPS = 157.3   # fp32-input MFMA (v_mfma_f32_32x32x2_f32) = the fp32 vector rate (same table)
PEAK_MFMA_F32X_TFLOPS = 2500.0 / 3.0  # fp32x mode: three fp16 MFMAs (hi*hi, hi*lo, lo*hi) per useful product


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)   # ~1 s of GPU work at the default workload
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scale", default="s")
    ap.add_argument("--family", default="yolo11", choices=["yolo11", "yolov8", "bsyolo11"],
                    help="graph: stock YOLO11 (the headline config), YOLOv8, or the fork's own BS-YOLO graph (nc = 12)")
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--batch", type=int, default=64, help="images per GPU (weak scaling) or in all (strong scaling)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: --batch images per GPU; strong: --batch images in all, split contiguously over the ranks")
    ap.add_argument("--precision", default="fp16", choices=["fp16", "fp32", "fp32x"],
                    help="fp16: the product path (NHWC fp16 activations, the headline); fp32: the engine's exact fp32 mode -- fp32 storage and "
                         "arithmetic on the fp32 matrix pipe; fp32x: fp32 storage, dense convs on the fp16 matrix pipe with split-f16 operands "
                         "(~2^-21 operand error; what plugin.accelerate gives callers of predict(half=False))")
    ap.add_argument("--graph", default="off", choices=["on", "off"],
                    help="replay the forward as ONE captured hipGraph launch (engine graph mode).  Off by default: measured SLOWER than the "
                         "eager replay at every batch size on ROCm 7.2 (8 images: 1.17 vs 0.92 ms per forward + NMS; DESIGN.md section 6)")
    ap.add_argument("--serial-nms", action="store_true",
                    help="run NMS (and the detection all-gather) on the forward's stream; default: on a second stream, so that "
                         "NMS of step i runs beside the forward of step i + 1 (every step's work still lies inside the timed region)")
    ap.add_argument("--latency", default="auto", choices=["auto", "on", "off"],
                    help="the engine's latency mode (split-K by layer shape on the long thin conv layers: deterministic, shard-invariant; DESIGN.md "
                         "section 6).  auto: on when --scaling strong leaves this rank 16 images or fewer")
    ap.add_argument("--inflight", type=int, default=1, choices=[1, 2],
                    help="forwards in flight: 2 = a second engine (its own activation arena) on a second stream takes every other step, so that step "
                         "i + 1 runs beside step i (a pipelined server's two batches in flight); every step's work still lies inside the timed region")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=8)
    ap.add_argument("--cpu-runs", type=int, default=20, help="CPU baseline sample: runs of --cpu-batch images (~10 s in all)")
    ap.add_argument("--cpu-runs-1t", type=int, default=3, help="the same at ONE thread (the reference's default, ultralytics/__init__.py:7-8)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed to DIR/*.npy (rank 0; see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


NAMES = {"yolo11": "YOLO11", "yolov8": "YOLOv8", "bsyolo11": "BS-YOLO11"}


def cpu_baseline(args, cfg_sd):
    """The oracle (torch-CPU fp32 restatement of the reference path, oracle/) timed on this host: forward + NMS, at this
    job's core share AND at one thread (`import ultralytics` pins OMP_NUM_THREADS=1 by default)."""
    import torch
    from oracle import postproc_ref as PP
    from oracle import yolo_ref as R
    m = R.Model(args.family, args.scale, 12 if args.family == "bsyolo11" else 80, "detect")
    P = {k: v.float() for k, v in cfg_sd.items()}
    P[f"model.{len(m.layers) - 1}.dfl.conv.weight"] = torch.arange(16, dtype=torch.float32).view(1, 16, 1, 1)
    x = torch.rand(args.cpu_batch, 3, args.imgsz, args.imgsz, generator=torch.Generator().manual_seed(0))

    keep = {}

    def timed(threads, runs):
        torch.set_num_threads(threads)
        with torch.inference_mode():
            y, _ = m.forward(P, x)  # warm-up
            keep.setdefault("y", y.clone())
            t0 = time.perf_counter()
            for _ in range(runs):
                y, _ = m.forward(P, x)
                PP.non_max_suppression(y, 0.25, 0.7)
            return time.perf_counter() - t0

    if args.cpu_runs <= 0:
        return None
    # the GPU box shares its host: use this job's CPU share (16 threads per GPU), not every visible core
    cores = min(16, os.cpu_count() or 1)
    what = f"batch {args.cpu_batch} {NAMES[args.family]}{args.scale} {args.imgsz}x{args.imgsz} fp32 forward + NMS, torch CPU"
    dt = timed(cores, args.cpu_runs)
    out = {"value": round(args.cpu_batch * args.cpu_runs / dt, 3), "unit": "images/sec", "cores": cores, "kind": "port",
           "sample": f"{args.cpu_runs} x {what} {cores} threads, after 1 warm-up ({dt:.1f} s)"}
    if args.cpu_runs_1t > 0:
        dt1 = timed(1, args.cpu_runs_1t)
        out["single_thread"] = {"value": round(args.cpu_batch * args.cpu_runs_1t / dt1, 3), "unit": "images/sec", "cores": 1,
                                "sample": f"{args.cpu_runs_1t} x {what} 1 thread, after 1 warm-up ({dt1:.1f} s)"}
    out["_sample"] = (x, keep["y"])  # the oracle's prediction tensor for its sample: main() states the GPU path's parity against it
    return out


def parity_stats(y, y_ref):
    """max / p99.9 / mean of |dscore| and |dbox| (pixels) between two (B, 4 + nc, A) prediction tensors."""
    import torch
    ds, db = (y[:, 4:] - y_ref[:, 4:]).abs().flatten().float(), (y[:, :4] - y_ref[:, :4]).abs().flatten().float()
    step = max(1, ds.numel() // 8_000_000)  # torch.quantile caps its input size
    return {"score_max": float(f"{float(ds.max()):.3g}"), "score_p999": float(f"{float(torch.quantile(ds[::step], 0.999)):.3g}"), "score_mean": float(f"{float(ds.mean()):.3g}"),
            "box_max_px": float(f"{float(db.max()):.3g}"), "box_p999_px": float(f"{float(torch.quantile(db, 0.999)):.3g}"), "box_mean_px": float(f"{float(db.mean()):.3g}")}


DUMP_BUDGET = 48 << 20  # bytes of detections written by --dump-outputs; the prediction sample adds 12 MB
DUMP_PRED_SAMPLE = 1 << 20  # elements of the prediction tensor written by --dump-outputs


def dump_outputs(out_dir, det, counts, y):
    """--dump-outputs: the last timed step's results as float .npy files, identical inputs from run to run (seeded weights and images):
    detections.npy  (N, max_det, 6) float32: what NMS returned per image (x1, y1, x2, y2, conf, cls); rows past counts[i] are padding
                    and written as zeros.  N = every image of the step (all ranks' after the all-gather), or its first images that fit
                    DUMP_BUDGET.
    counts.npy      (N,) float64: detections per image.
    predictions_sample.npy / predictions_sample_index.npy  (DUMP_PRED_SAMPLE,) float32 / float64: a fixed seeded sample of this rank's
                    prediction tensor (B, 4 + nc, A) that NMS read, and the flat indices it was taken at (sorted; may repeat).
    Host copies only (no kernel launch), after the timed region."""
    import numpy as np
    import torch
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    n = max(1, min(det.shape[0], DUMP_BUDGET // (det[0].numel() * 4)))
    d, c = det[:n].cpu().float(), counts[:n].cpu().to(torch.int64)
    d[torch.arange(d.shape[1]).view(1, -1) >= c.view(-1, 1)] = 0.0
    yh = y.detach().flatten().cpu()
    idx = torch.randint(0, yh.numel(), (DUMP_PRED_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
    np.save(out / "detections.npy", d.numpy())
    np.save(out / "counts.npy", c.numpy().astype(np.float64))
    np.save(out / "predictions_sample.npy", yh[idx].float().numpy())
    np.save(out / "predictions_sample_index.npy", idx.numpy().astype(np.float64))


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a CHILD `torch.distributed.run` and relay its
    output and exit code.  Decided before this process has imported torch or touched the GPU (never an exec of a process
    that initialised HIP)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve()), *sys.argv[1:]]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.run(cmd, env=env).returncode


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    args.gpus = world
    if not torch.cuda.is_available():
        sys.exit(f"bench.py needs a ROCm GPU: the product path has no CPU fallback (rank {rank} of {world})")
    # BSY_BENCH_BACKEND=gloo: rehearsal of the N > 1 control flow with several ranks on ONE GPU (RCCL refuses two ranks on
    # one device); never a measurement
    backend = os.environ.get("BSY_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local %= torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    use_dist = world > 1 or os.environ.get("BSY_BENCH_FORCE_DIST") == "1"  # the latter: 1-rank rehearsal of the RCCL path
    saved_stdout = None
    if use_dist:
        # RCCL prints a version banner on STDOUT when the first communicator is created; the contract is ONE JSON line there:
        # everything up to the result goes to stderr (file descriptor level: the banner comes from C code)
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))

    from bs_yolo_amd import lib as L
    from bs_yolo_amd import nms as HN
    from bs_yolo_amd.engine import YoloEngine
    from bs_yolo_amd.graphs import stock_cfg
    from bs_yolo_amd.plan import Plan
    from bs_yolo_amd.weights import synth_state_dict

    cfg = stock_cfg(args.family, args.scale, 12 if args.family == "bsyolo11" else 80, "detect")
    sd = synth_state_dict(Plan(cfg, 1, 64, 64), seed=0)
    S = args.imgsz
    f32 = args.precision in ("fp32", "fp32x")
    f32x = args.precision == "fp32x"
    peak = PEAK_MFMA_F32X_TFLOPS if f32x else (PEAK_MFMA_F32_TFLOPS if f32 else PEAK_MFMA_F16_TFLOPS)
    if args.scaling == "strong":  # the global batch is fixed: this rank's contiguous share of it (parallel.shard_bounds)
        from bs_yolo_amd.parallel import shard_bounds
        lo, hi = shard_bounds(args.batch, world)[rank]
        B, global_batch = hi - lo, args.batch
        if B == 0:
            sys.exit(f"--scaling strong: batch {args.batch} leaves rank {rank} of {world} without images")
    else:
        B, global_batch = args.batch, world * args.batch
    use_graph = args.graph == "on"
    use_latency = args.precision == "fp16" and (args.latency == "on" or (args.latency == "auto" and args.scaling == "strong" and B <= 16))
    eng = YoloEngine(cfg, sd, device=local, precision=args.precision, graph=use_graph, latency=use_latency)
    g = torch.Generator().manual_seed(1234 + rank)
    x = torch.rand(B, 3, S, S, generator=g).to(torch.float32 if f32 else torch.float16).to(dev)
    if not (args.family == "yolo11" and args.scale == "s"):
        # The class head of synth_state_dict is calibrated for the headline graph (1.5 % of the anchors above conf 0.25).
        # Other graphs: rescale and shift it from the raw class logits of one probe forward (8 images) so that the same
        # share passes (1-2 %) -- else NMS sees either nothing or max_det-saturated images.
        _, raws = eng(x[:min(8, B)], want_raw=True)
        bias0 = float(next(v for k, v in sd.items() if ".cv3." in k and k.endswith(".2.bias")).flatten()[0])
        lc = torch.cat([r[:, 64:].float().flatten(2) for r in raws], 2) - bias0          # centred logits (8, nc, A)
        gain = 1.0 / max(float(lc.std()), 1e-6)
        q = float(torch.quantile((lc * gain).amax(1).flatten().cpu(), 1.0 - 0.015))
        for k in list(sd):
            if ".cv3." in k and k.endswith(".2.weight"):
                sd[k] = sd[k] * gain
            elif ".cv3." in k and k.endswith(".2.bias"):
                sd[k] = torch.full_like(sd[k], math.log(0.25 / 0.75) - q)
        eng.close()
        eng = YoloEngine(cfg, sd, device=local, precision=args.precision, graph=use_graph, latency=use_latency)
    from bs_yolo_amd.parallel import gather_detections_async
    pending = None   # the previous step's detection all-gather, in flight on RCCL's stream
    gathered = None
    last_y = None    # --dump-outputs: the prediction tensor of the latest step

    # Post-processing stream: NMS reads a prediction tensor of its own (the engine allocates `y` per call), so NMS of step i may run
    # beside the forward of step i + 1 -- 64 one-workgroup-per-image kernels next to 256-CU conv launches.  The forward's stream
    # never waits for it; torch.cuda.synchronize() at the end of the timed region does.
    if use_graph:  # the legacy default stream cannot be captured: the forward gets a stream of its own
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    main = torch.cuda.current_stream(dev)
    # graph mode returns outputs from a ring of preallocated tensors that a later replay overwrites: a consumer on another stream
    # could still be reading them -- NMS stays on the forward's stream there
    post = main if (args.serial_nms or use_graph) else torch.cuda.Stream(device=dev)
    # --inflight 2: engines[1] is a second engine (same weights, its own arena and plans) on a stream of its own; steps alternate
    engines, fstreams, nstep = [eng], [main], 0
    if args.inflight == 2:
        if use_graph or args.serial_nms:
            sys.exit("--inflight 2 needs the eager forward and the NMS stream")
        engines.append(YoloEngine(cfg, sd, device=local, precision=args.precision, latency=use_latency))
        fstreams.append(torch.cuda.Stream(device=dev))

    def step():
        nonlocal pending, gathered, nstep, last_y
        k = nstep % len(engines)
        nstep += 1
        if k:
            with torch.cuda.stream(fstreams[k]):
                y, _ = engines[k](x, want_raw=False)
            y.record_stream(fstreams[k])
            post.wait_stream(fstreams[k])
        else:
            y, _ = eng(x, want_raw=False)
        if args.dump_outputs:
            last_y = y
        if post is not main and not k:
            post.wait_stream(main)
        with torch.cuda.stream(post):
            det, counts = HN.nms_batched(y, 0.25, 0.7, max_det=300)
            if post is not main:
                y.record_stream(post)
            if use_dist:
                # ONE collective per step (counts packed behind the detections), overlapped with the NEXT step's forward:
                # this step's kernels are already enqueued when the stream is ordered after the previous gather
                if pending is not None:
                    gathered = pending.wait()
                pending = gather_detections_async(det, counts)
        return det, counts

    def drain():
        nonlocal pending, gathered
        if pending is not None:
            with torch.cuda.stream(post):
                gathered = pending.wait()
            pending = None

    # Parity of the benchmarked path and the CPU leg run HERE, before the warm-up: the W warm-up steps lead straight into the K timed steps
    # (no idle gap in front of the timed region: the CPU leg takes ~10 s), and the timed steps and the three serial profile passes are the
    # last GPU work of the process (tools/prof_summary.py and the PMC scripts window the trace by launch count)
    cpu_base, parity = None, None
    if rank == 0:
        # Parity of the benchmarked path, so that the headline number travels with its tolerance (north-star: 1e-3 on scores, 1e-3 * imgsz on
        # boxes against the CPU reference).  With the cpu_baseline leg: against the oracle's own outputs on that leg's sample; always:
        # against the engine's exact fp32 mode on 8 of the benchmark's images (that mode is pinned to the reference at ~1e-5 by the tests).
        parity = {"tolerance_claimed": "1e-3 scores, 1e-3 * imgsz boxes" if f32 else
                  ("fp16 storage, BS-YOLO graph with synthetic weights: mean score error < 1e-3, mean box error < 0.2 px; no max / p99.9 bound "
                   "(the graph amplifies f16 storage rounding on flat DFL distributions: the CPU oracle with f16 storage emulation shows the same "
                   "tails, tests/test_gpu_parity.py test_engine_bsyolo_large_input_matches_oracle)") if args.family == "bsyolo11" else
                  "fp16 storage: score max < 1e-2 / p99.9 < 5e-3, box max < 16 px / p99.9 < 4 px (NOT 1e-3)"}
        nb = min(8, B)
        xs = x[:nb]
        y_path = eng(xs, want_raw=False)[0].float()
        if args.precision != "fp32":
            e32 = YoloEngine(cfg, sd, device=local, precision="fp32")
            y32 = e32(xs.float(), want_raw=False)[0]
            torch.cuda.synchronize()
            parity["vs_engine_fp32_mode"] = dict(parity_stats(y_path, y32), images=nb)
            e32.close()
        if not args.no_cpu_baseline and world == 1:  # reported at N = 1 only
            cpu_base = cpu_baseline(args, sd)
            if cpu_base:
                xc, yc = cpu_base.pop("_sample")
                yg = eng(xc.to(dev).to(x.dtype), want_raw=False)[0].float().cpu()
                parity["vs_cpu_reference"] = dict(parity_stats(yg, yc), images=int(xc.shape[0]),
                                                  against="the cpu_baseline leg's oracle forward (torch fp32 restatement of the reference) on its own sample")
    for _ in range(args.warmup):
        det, counts = step()
    drain()
    torch.cuda.synchronize()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        det, counts = step()
    drain()  # the last step's gather completes inside the timed region
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_step = dt / args.steps * 1e3
    value = global_batch * args.steps / dt
    if args.dump_outputs and rank == 0:  # before the profile passes: graph mode's outputs live in a ring that a replay overwrites
        dump_outputs(args.dump_outputs, *(gathered if use_dist else (det, counts)), last_y)

    if rank == 0:
        # ---- roofline of the dominant kernel family: EVERY launch that does dense-conv MFMA work -- the plan's OP_CONV ops
        #      (conv_mfma_kernel / conv3x3_patch_kernel / conv1x1_persist_kernel) and the fused conv kernels (stem, Bottleneck,
        #      C3k2 tail, DWConv+1x1, ...).  Round 1 priced the OP_CONV launches alone; since convs keep moving into fused
        #      kernels that subset is no longer a stable family, so both are reported.  HIP events around every op on the
        #      launch stream, three serial passes after the timed region.  They come LAST in the process: the
        #      PMC scripts under tools/ window "the last forward" by launch count.
        prof = None
        for _ in range(3):
            prof, plan = eng.profile(x)
        fam = [(o, t) for o, (_, _, t) in zip(plan.ops, prof) if o.get("mfma_flops")]
        fam_ms = sum(t for _, t in fam)
        fam_flops = sum(o["mfma_flops"] for o, _ in fam)
        n_fam = len(fam)
        conv_ms = sum(t for o, t in fam if o["kind"] == L.OP_CONV)
        conv_flops = sum(o["mfma_flops"] for o, _ in fam if o["kind"] == L.OP_CONV)
        n_conv = sum(1 for o, _ in fam if o["kind"] == L.OP_CONV)
        # algorithmic bytes of the family: every operand read once, every result written once (fused ops: their external
        # inputs and outputs only)
        fam_bytes = 0
        for o, _ in fam:
            for key in ("src0", "src1", "res"):
                t = o.get(key)
                if t is None:
                    continue
                if o["kind"] in (L.OP_CONV_FIRST, L.OP_STEM) and key == "src0":
                    fam_bytes += B * 3 * o["H"] * o["W"] * (4 if f32 else 2)
                else:
                    fam_bytes += B * o["H"] * o["W"] * t.C * (4 if t.f32 else 2) // (4 if t.up else 1)
            if o["kind"] == L.OP_CHAIN:  # first conv's output where it is written, second conv's HBM K part, first conv's shortcut operand
                fam_bytes += sum(B * o["H"] * o["W"] * t.C * 2 for t in o["box"] if t is not None)
            mode = o.get("out_f32", 0)  # 0 f16 map, 1 f32 map, 2 / 3 fused decoder: class rows / 4 box rows of y (f16)
            fam_bytes += B * o["OH"] * o["OW"] * ({2: o.get("cout", 0), 3: 4}.get(mode, o["dst"].C)) * (4 if (mode == 1 or f32) else 2)
        achieved = fam_flops / (fam_ms * 1e-3) / 1e12
        # HBM traffic of the same kernel family cannot be sampled from inside the process: it is the PMC measurement
        # committed under profiles/ (tools/pmc_bench_traffic.sh: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate
        # passes, gfx950 correction), per launch like `achieved`; only valid for the default workload
        # passes, gfx950 correction), per launch like `achieved`; only valid for the default workload AND for the plan it was
        # taken on: the file records the family's launch count, a different count here means the plan has changed since
        traffic, tsrc, tnote = None, None, None
        for name in ("r04_traffic.json", "r03_traffic.json", "r02_traffic.json"):
            tfile = ROOT / "profiles" / name
            if tfile.exists() and args.family == "yolo11" and args.scale == "s" and S == 640 and B == 64 and not f32:
                tj = json.load(open(tfile))
                if tj.get("conv_launches_per_step", n_fam) != n_fam:
                    tnote = f"profiles/{name} was measured on a plan with {tj.get('conv_launches_per_step')} family launches per step, this one has {n_fam}: not reported"
                    continue
                traffic = round(tj["conv_mfma_hbm_bytes_per_launch_avg"])
                tsrc = name
                break
        fwd_ms = sum(t for (_, _, t) in prof)
        out = {
            "metric": f"images/sec {NAMES[args.family]}{args.scale} {S}x{S} bs={B if args.scaling == 'weak' else global_batch} (forward + NMS)"
                      + (", fp32x engine mode" if f32x else (", fp32 engine mode" if f32 else "")),
            "value": round(value, 1), "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step, 4),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "f32" if f32 else "f16", "data": "synthetic",
            "config": {"workload": f"{NAMES[args.family]}{args.scale} detect {S}x{S} {args.precision}, "
                                   + (f"batch {B} per GPU" if args.scaling == "weak" else f"global batch {global_batch} split over {world} GPU(s)")
                                   + ", seeded random weights, engine forward + HIP NMS (conf 0.25, iou 0.7, max_det 300)"
                                   + ((" + RCCL all-gather of detections" if backend == "nccl" else f" + {backend} all-gather of detections (rehearsal backend, not RCCL)") if use_dist else ""),
                       "global_batch": global_batch, "imgsz": S, "parallelism": f"images sharded over {world} GPU(s)",
                       "pipeline": ("NMS on the forward's stream" if args.serial_nms else "NMS of step i on a second stream beside the forward of step i + 1")
                                   + (", two forwards in flight (two engines with their own activation arenas on two streams take alternate steps)" if args.inflight == 2 else ""),
                       "latency_mode": bool(use_latency),
                       "forward_launch": ("one captured hipGraph launch per forward (%d captured, %d replayed)" % (eng.graph_stats["captures"], eng.graph_stats["replays"]))
                                         if use_graph else "eager: one launch per op",
                       "mean_detections_per_image": round(float(counts.float().mean().item()), 1),
                       "model_gflop_per_image": round(plan.flops / B / 1e9, 2),
                       "whole_path_tflops": round(plan.flops / B * global_batch / (ms_step * 1e-3) / 1e12, 1)},
            "roofline": {"bound": "mfma", "achieved": round(achieved, 1), "peak": peak, "unit": "TFLOP/s",
                         "frac": round(achieved / peak, 4), "traffic": traffic,
                         "traffic_unit": f"HBM bytes per launch (PMC, profiles/{tsrc})" if tsrc else tnote,
                         "algorithmic_bytes_per_launch_avg": round(fam_bytes / n_fam),
                         "kernel": ("dense-conv family of the fp32x mode: every conv launch of one forward (conv32x_mfma_kernel: fp32 storage, operands "
                                    "split into f16 pairs, three v_mfma_f32_32x32x16_f16 per product; peak = the fp16 matrix rate / 3; the image "
                                    "conv stays on the exact fp32 kernel)") if f32x else
                                   ("dense-conv family of the fp32 mode: every conv launch of one forward (conv32_mfma_kernel, v_mfma_f32_32x32x2_f32; "
                                    "peak = the fp32 matrix rate)") if f32 else
                                   ("dense-conv family: every MFMA conv launch of one forward (conv_mfma_kernel, conv3x3_patch_kernel, "
                                    "conv1x1_persist_kernel, the fused stem / Bottleneck / C3k2 / DWConv+1x1 kernels and the chained 1x1 pairs of chain1x1_kernel)"),
                         "launches_per_step": n_fam,
                         "flops_per_launch_avg": round(fam_flops / n_fam), "avg_launch_ms": round(fam_ms / n_fam, 5),
                         "family_ms_per_step": round(fam_ms, 4), "forward_ms_per_step_by_events": round(fwd_ms, 4),
                         "op_conv_only": {"launches_per_step": n_conv, "ms_per_step": round(conv_ms, 4),
                                          "achieved": round(conv_flops / (conv_ms * 1e-3) / 1e12, 1),
                                          "frac": round(conv_flops / (conv_ms * 1e-3) / 1e12 / peak, 4),
                                          "note": "the round-1 definition (plan ops of kind OP_CONV only), for continuity"}},
        }
        out["config"]["parity"] = parity
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
        if saved_stdout is not None:
            sys.stdout.flush()
            os.dup2(saved_stdout, 1)
            os.close(saved_stdout)
            saved_stdout = None
        print(json.dumps(out), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    for e in engines[1:]:
        e.close()
    eng.close()


if __name__ == "__main__":
    main()
