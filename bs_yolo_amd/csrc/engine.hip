// Engine / plan objects behind the C ABI (include/bsyolo.h): lifecycle, arena, guards, plan replay, graph capture, tuning, profile.
// What an op record means is op_args.h, which launcher it goes to plan_ops.hip; the stand-alone operators are ops_api.hip.
//
// The host side (bs_yolo_amd/plan.py) flattens the model graph -- the work of BaseModel._predict_once
// (nn/tasks.py:138-165) and of every module forward on the path -- into a list of bsy_op records that reference
// workspace buffers by index.  A plan owns that workspace in HBM (one allocation, 256-byte aligned slices) and replays
// the op list on the caller's stream; nothing here synchronises or allocates per call.
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "engine.h"

extern "C" int bsy_sizeof_op(void) { return (int)sizeof(bsy_op); }  // the host mirrors the record with ctypes: checked at load

extern "C" int bsy_engine_create(int device, bsy_engine** out) {
    if (!out) BSY_FAIL(BSY_ERR_ARG, "engine_create: null out");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) BSY_FAIL(BSY_ERR_ARG, "engine_create: device %d of %d", device, ndev);
    bsy_engine* e = new bsy_engine();
    e->device = device;
    *out = e;
    return BSY_OK;
}

extern "C" void bsy_engine_destroy(bsy_engine* e) {
    if (!e) return;
    if (e->weights) (void)hipFree(e->weights);
    if (e->arena) (void)hipFree(e->arena);
    delete e;
}

extern "C" int bsy_engine_load_weights(bsy_engine* e, const void* host_blob, size_t bytes) {
    if (!e || !host_blob || !bytes) BSY_FAIL(BSY_ERR_ARG, "load_weights: bad argument");
    HIP_TRY(hipSetDevice(e->device));
    if (e->weights) {
        // a reload on an engine that has run: nothing may still be reading the old blob (plans resolve `weights + w_off` when they
        // are enqueued), and graphs captured so far hold its addresses -- weights_gen below makes bsy_plan_graph_launch drop them
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipFree(e->weights));
        e->weights = nullptr;
    }
    ++e->weights_gen;
    // BSY_WEIGHT_GUARD=<bytes> (test aid): that many bytes of 0x7C behind the blob -- as f16 every pair is a NaN (0x7C7C), as
    // f32 a huge finite number -- so a kernel that reads past the packed weights AND uses what it read changes the outputs
    // (tests compare a poisoned engine with a plain one; round 1 found such a read in the flat-DMA path by accident, 8ab4d40).
    // Reads past the blob whose values are discarded (padding rows of a cout tile) stay invisible by design.
    const char* g = getenv("BSY_WEIGHT_GUARD");
    const size_t guard = g ? align256((size_t)atoll(g)) : 0;
    if (hipMalloc(&e->weights, bytes + 256 + guard) != hipSuccess) BSY_FAIL(BSY_ERR_ALLOC, "load_weights: hipMalloc(%zu) failed", bytes);
    HIP_TRY(hipMemcpy(e->weights, host_blob, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset((char*)e->weights + bytes, guard ? 0x7C : 0, 256 + guard));
    e->weight_bytes = bytes;
    return BSY_OK;
}

static int plan_make_lanes(bsy_plan* p) {
    int max_lane = 0;
    for (const auto& o : p->ops) max_lane = o.lane > max_lane ? o.lane : max_lane;
    if (max_lane > 31) BSY_FAIL(BSY_ERR_ARG, "plan_create: too many lanes");
    p->lanes.assign(max_lane + 1, nullptr);
    p->lane_done.assign(max_lane + 1, nullptr);
    p->lane_fork.assign(max_lane + 1, nullptr);
    bool ok = true;
    for (int l = 1; l <= max_lane && ok; ++l)
        ok = hipStreamCreateWithFlags(&p->lanes[l], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&p->lane_done[l], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&p->lane_fork[l], hipEventDisableTiming) == hipSuccess;
    if (!ok) BSY_FAIL(BSY_ERR_HIP, "plan_create: stream/event creation failed");
    return BSY_OK;
}

// bsy_op.act per kind (include/bsyolo.h): an activation id 0 / 1 / 2 (identity, SiLU, ReLU) for the four kinds whose kernels take one; a
// field of its own meaning for DWCONV_G (a channel count), DECODE (bits) and ATTN (the pe flag); a 0 / 1 SiLU switch for every other
// kind, whose kernels test it for truth -- an id above 1 there would run SiLU and say nothing, so it is refused here, by name.
static int plan_check_acts(const bsy_op* ops, int n_ops, const char* who) {
    static const char* const names[] = {"CONV_FIRST", "CONV", "DWCONV", "SPPF_POOL", "ATTN", "DECODE", "RAW_NCHW", "NHWC2NCHW", "STEM", "BNECK",
                                        "DWCONV_G", "COPY", "GAP", "MSCA_MIX", "MUL", "ELA", "DWPW", "MSCA_SPATIAL", "C3K2", "S2D", "PMSFA_TAIL",
                                        "CHAIN", "POOL_DOWN", "CLASSIFY_TAIL", "GHOST", "ADD", "E2E_TOPK", "MAXPOOL", "FIRST_POOL", "MAXSIG", "CBFUSE"};
    static_assert(sizeof(names) / sizeof(names[0]) == BSY_OP_KIND_COUNT && BSY_OP_CBFUSE == BSY_OP_KIND_COUNT - 1 && BSY_OP_MAXSIG == 29 && BSY_OP_ELA == 15 &&
                  BSY_OP_DWPW == 16 && BSY_OP_GHOST == 24, "names[] is indexed by bsy_op_kind: a new kind adds its name here, in the enum's order");
    for (int i = 0; i < n_ops; ++i) {
        const int kind = ops[i].kind, act = ops[i].act;
        // MAXSIG: what its record says without a pointer -- absent views, nc < 1, a head width the fp16 kernel does not take, a destination
        // over the embedding -- is refused here, by name, not at the first launch
        if (kind == BSY_OP_MAXSIG && !maxsig_record_ok(ops[i])) {
            const std::string why = bsy_last_error();
            BSY_FAIL(BSY_ERR_ARG, "%s: op %d (MAXSIG): %s", who, i, why.c_str());
        }
        // CBFUSE: a tap count or shift out of range, a size a shift does not divide, a tap narrower than dst, a dst over a tap's channels
        if (kind == BSY_OP_CBFUSE && !cbfuse_record_ok(ops[i])) {
            const std::string why = bsy_last_error();
            BSY_FAIL(BSY_ERR_ARG, "%s: op %d (CBFUSE): %s", who, i, why.c_str());
        }
        if (kind == BSY_OP_DWCONV_G || kind == BSY_OP_DECODE || kind == BSY_OP_ATTN) continue;
        const bool ids = kind == BSY_OP_CONV_FIRST || kind == BSY_OP_FIRST_POOL || kind == BSY_OP_STEM || kind == BSY_OP_CONV;
        if (act < 0 || act > (ids ? 2 : 1))
            BSY_FAIL(BSY_ERR_ARG, "%s: op %d (%s) has act = %d: %s", who, i, kind >= 0 && kind < (int)(sizeof(names) / sizeof(names[0])) ? names[kind] : "?",
                     act, ids ? "0 identity, 1 SiLU, 2 ReLU" : "this kind takes 0 or 1 (SiLU); ReLU (2) exists in CONV_FIRST, FIRST_POOL, STEM and CONV");
    }
    return BSY_OK;
}

extern "C" int bsy_plan_create(bsy_engine* e, const bsy_op* ops, int n_ops, const int64_t* buf_bytes, int n_bufs,
                               bsy_plan** out) {
    if (!e || !ops || n_ops <= 0 || !out || n_bufs < 0 || (n_bufs && !buf_bytes)) BSY_FAIL(BSY_ERR_ARG, "plan_create: bad argument");
    if (const int rc = plan_check_acts(ops, n_ops, "plan_create")) return rc;
    if (!e->weights) BSY_FAIL(BSY_ERR_STATE, "plan_create: load weights first");
    HIP_TRY(hipSetDevice(e->device));
    bsy_plan* p = new bsy_plan();
    p->eng = e;
    p->ops.assign(ops, ops + n_ops);
    // BSY_PLAN_GUARD=<bytes> (test aid): a guard band of that many bytes, filled with 0xA5, behind every buffer;
    // bsy_plan_check_guards reports the first band a kernel wrote into (an out-of-bounds store).
    {
        const char* g = getenv("BSY_PLAN_GUARD");
        p->guard = g ? align256((size_t)atoll(g)) : 0;
    }
    size_t off = 0;
    for (int i = 0; i < n_bufs; ++i) {
        if (buf_bytes[i] < 0) { delete p; BSY_FAIL(BSY_ERR_ARG, "plan_create: negative buffer size"); }
        p->buf_off.push_back(off);
        p->buf_size.push_back((size_t)buf_bytes[i]);
        off += align256((size_t)buf_bytes[i]) + p->guard;
    }
    p->workspace_bytes = off + 256;
    if (hipMalloc((void**)&p->workspace, p->workspace_bytes) != hipSuccess) {
        delete p;
        BSY_FAIL(BSY_ERR_ALLOC, "plan_create: hipMalloc(%zu) failed", off + 256);
    }
    // zero once so that padding channels nobody writes are finite
    if (hipMemset(p->workspace, 0, p->workspace_bytes) != hipSuccess) {
        (void)hipFree(p->workspace);
        delete p;
        BSY_FAIL(BSY_ERR_HIP, "plan_create: hipMemset failed");
    }
    for (int i = 0; i < n_bufs && p->guard; ++i)
        if (hipMemset(p->workspace + p->buf_off[i] + align256(p->buf_size[i]), 0xA5, p->guard) != hipSuccess) {
            (void)hipFree(p->workspace);
            delete p;
            BSY_FAIL(BSY_ERR_HIP, "plan_create: guard memset failed");
        }
    const int rc = plan_make_lanes(p);
    if (rc != BSY_OK) { bsy_plan_destroy(p); return rc; }
    *out = p;
    return BSY_OK;
}

// The activation buffers of this plan live at HOST-assigned byte offsets (multiples of 256; they may overlap where
// bs_yolo_amd/plan.py found the buffers' lifetimes disjoint) inside the engine's shared arena of at least `arena_bytes`.
// The arena is (re)allocated here when it is too small -- after a device synchronisation, so no earlier plan can still be
// running in the old one.  Plans of one engine share the arena: run them on one stream at a time (the reference serialises
// predict() the same way, engine/predictor.py:113,229).
extern "C" int bsy_plan_create_arena(bsy_engine* e, const bsy_op* ops, int n_ops, const int64_t* buf_bytes, const int64_t* buf_off,
                                     int n_bufs, int64_t arena_bytes, bsy_plan** out) {
    if (!e || !ops || n_ops <= 0 || !out || n_bufs < 0 || (n_bufs && (!buf_bytes || !buf_off)) || arena_bytes < 0)
        BSY_FAIL(BSY_ERR_ARG, "plan_create_arena: bad argument");
    if (const int rc = plan_check_acts(ops, n_ops, "plan_create_arena")) return rc;
    if (!e->weights) BSY_FAIL(BSY_ERR_STATE, "plan_create_arena: load weights first");
    for (int i = 0; i < n_bufs; ++i)
        if (buf_bytes[i] < 0 || buf_off[i] < 0 || (buf_off[i] & 255) || buf_off[i] + buf_bytes[i] > arena_bytes)
            BSY_FAIL(BSY_ERR_ARG, "plan_create_arena: buffer %d (offset %lld, %lld bytes) outside the arena of %lld bytes", i,
                     (long long)buf_off[i], (long long)buf_bytes[i], (long long)arena_bytes);
    HIP_TRY(hipSetDevice(e->device));
    const size_t need = (size_t)arena_bytes + 256;
    if (need > e->arena_bytes) {
        HIP_TRY(hipDeviceSynchronize());
        if (e->arena) { HIP_TRY(hipFree(e->arena)); e->arena = nullptr; e->arena_bytes = 0; }
        if (hipMalloc((void**)&e->arena, need) != hipSuccess) BSY_FAIL(BSY_ERR_ALLOC, "plan_create_arena: hipMalloc(%zu) failed", need);
        e->arena_bytes = need;
        ++e->arena_gen;
        // zero once so that padding channels nobody writes start finite (later tenants of a region leave ordinary f16 / f32
        // activations behind; no kernel consumes padding channels)
        HIP_TRY(hipMemset(e->arena, 0, need));
    }
    bsy_plan* p = new bsy_plan();
    p->eng = e;
    p->use_arena = true;
    p->ops.assign(ops, ops + n_ops);
    for (int i = 0; i < n_bufs; ++i) {
        p->buf_off.push_back((size_t)buf_off[i]);
        p->buf_size.push_back((size_t)buf_bytes[i]);
    }
    const int rc = plan_make_lanes(p);
    if (rc != BSY_OK) { bsy_plan_destroy(p); return rc; }
    *out = p;
    return BSY_OK;
}

extern "C" size_t bsy_engine_arena_bytes(const bsy_engine* e) { return e ? e->arena_bytes : 0; }

// Test aid: synchronises the device and checks the guard bands (plans created under BSY_PLAN_GUARD).  Returns BSY_OK and
// *bad_buf = -1 when every band is intact, else the index of the first buffer whose band was written and the byte offset
// of the first damaged byte inside the band.
extern "C" int bsy_plan_check_guards(bsy_plan* p, int32_t* bad_buf, int64_t* bad_off) {
    if (!p || !bad_buf) BSY_FAIL(BSY_ERR_ARG, "plan_check_guards: bad argument");
    *bad_buf = -1;
    if (bad_off) *bad_off = 0;
    if (!p->guard || p->use_arena) return BSY_OK;  // arena plans carry no guard bands (buffers alias by design)
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned char> host(p->guard);
    for (size_t i = 0; i < p->buf_off.size(); ++i) {
        HIP_TRY(hipMemcpy(host.data(), p->workspace + p->buf_off[i] + align256(p->buf_size[i]), p->guard, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < p->guard; ++k)
            if (host[k] != 0xA5) {
                *bad_buf = (int32_t)i;
                if (bad_off) *bad_off = (int64_t)k;
                return BSY_OK;
            }
    }
    return BSY_OK;
}

extern "C" void bsy_plan_destroy(bsy_plan* p) {
    if (!p) return;
    p->drop_graphs();
    for (auto ev : p->events) (void)hipEventDestroy(ev);
    for (auto ev : p->lane_done) if (ev) (void)hipEventDestroy(ev);
    for (auto st : p->lanes) if (st) (void)hipStreamDestroy(st);
    for (auto ev : p->lane_fork) if (ev) (void)hipEventDestroy(ev);
    if (p->workspace) (void)hipFree(p->workspace);
    delete p;
}

// Ops are listed in a valid serial order.  An op on lane k > 0 runs on the plan's side stream k, which is forked from
// the caller's stream (event wait) the first time it is used after a join; an op flagged `join` first waits for every
// active side stream.  Chains on different lanes must not depend on each other between a fork and the next join
// (plan.py guarantees it: per-level Detect / Segment branches).
extern "C" int bsy_plan_run(bsy_plan* p, void* const* ext, int n_ext, bsy_stream stream) {
    if (!p || (n_ext && !ext)) BSY_FAIL(BSY_ERR_ARG, "plan_run: bad argument");
    hipStream_t main = (hipStream_t)stream;
    Resolver R = p->resolver(ext, n_ext);
    unsigned active = 0;  // bit k: side stream k has work since the last join
    int rc = BSY_OK;
    for (size_t i = 0; i < p->ops.size() && rc == BSY_OK; ++i) {
        const bsy_op& op = p->ops[i];
        // no early return inside this loop: every exit goes through the tail join below
        if (op.join && active) {
            for (size_t l = 1; l < p->lanes.size() && rc == BSY_OK; ++l)
                if (active & (1u << l)) {
                    if (hipEventRecord(p->lane_done[l], p->lanes[l]) != hipSuccess ||
                        hipStreamWaitEvent(main, p->lane_done[l], 0) != hipSuccess) {
                        bsy_set_error("plan_run: joining lane %zu failed", l);
                        rc = BSY_ERR_HIP;
                    } else {
                        active &= ~(1u << l);
                    }
                }
            if (rc != BSY_OK) break;
        }
        hipStream_t s = main;
        if (op.lane > 0) {
            s = p->lanes[op.lane];
            if (!(active & (1u << op.lane))) {
                if (hipEventRecord(p->lane_fork[op.lane], main) != hipSuccess ||
                    hipStreamWaitEvent(s, p->lane_fork[op.lane], 0) != hipSuccess) {
                    bsy_set_error("plan_run: forking lane %d failed", op.lane);
                    rc = BSY_ERR_HIP;
                    break;
                }
                active |= 1u << op.lane;
            }
        }
        rc = run_op(op, R, p->weights(), s);
    }
    // never leave side streams un-joined (error paths included): the caller only synchronises its own stream.  After an
    // error the lanes are drained on the host as well, so that nothing of this forward can still be writing the workspace
    // or the caller's outputs when the error is reported (the last-error text of the failing call is kept).
    for (size_t l = 1; l < p->lanes.size(); ++l)
        if (active & (1u << l)) {
            if (rc != BSY_OK) (void)hipStreamSynchronize(p->lanes[l]);
            (void)hipEventRecord(p->lane_done[l], p->lanes[l]);
            (void)hipStreamWaitEvent(main, p->lane_done[l], 0);
        }
    return rc;
}

// The forward as ONE graph launch.  At a rank's share of a strong-scaled batch (8 or 16 images: 70-odd launches of 4-15 us) the
// eager replay is bound by the host's launch rate and by the fork / join events of the head lanes; a captured graph hands the
// whole dependency structure -- lanes included, they become edges -- to the GPU's command processor in one submission.
// The graph bakes in every address: it is cached per set of external pointers (callers that cycle through a few input / output
// buffers hit the cache; at most BSY_GRAPH_MAX = 8 graphs per plan, least recently used dropped), and dropped when the arena
// moves, the weight blob is replaced (bsy_engine_load_weights) or the tuning changes.  Captures on `stream` in thread-local mode (bsy_plan_run issues nothing but kernel launches and event
// record / wait pairs); if a capture fails the plan runs eagerly, now and later.  *captured (may be null): 1 when this call
// had to capture, 0 when it replayed a cached graph, -1 when it ran eagerly.
#define BSY_GRAPH_MAX 8
extern "C" int bsy_plan_graph_launch(bsy_plan* p, void* const* ext, int n_ext, bsy_stream stream, int* captured) {
    if (!p || (n_ext && !ext)) BSY_FAIL(BSY_ERR_ARG, "plan_graph_launch: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (captured) *captured = -1;
    if (p->graph_unavailable || !s) return bsy_plan_run(p, ext, n_ext, stream);  // (the null stream cannot be captured)
    const unsigned gen = p->use_arena ? p->eng->arena_gen : 0u, wgen = p->eng->weights_gen;
    std::vector<void*> key(ext, ext + n_ext);
    for (size_t i = 0; i < p->graphs.size(); ++i)
        if (p->graphs[i].arena_gen == gen && p->graphs[i].weights_gen == wgen && p->graphs[i].ext == key) {
            if (captured) *captured = 0;
            if (i + 1 != p->graphs.size()) std::rotate(p->graphs.begin() + i, p->graphs.begin() + i + 1, p->graphs.end());  // most recently used last
            HIP_TRY(hipGraphLaunch(p->graphs.back().exec, s));
            return BSY_OK;
        }
    for (size_t i = 0; i < p->graphs.size();)  // graphs of an arena that has moved, or of a weight blob that has been replaced since
        if (p->graphs[i].arena_gen != gen || p->graphs[i].weights_gen != wgen) { (void)hipGraphExecDestroy(p->graphs[i].exec); p->graphs.erase(p->graphs.begin() + i); } else ++i;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        p->graph_unavailable = true;
        return bsy_plan_run(p, ext, n_ext, stream);
    }
    const int rc = bsy_plan_run(p, ext, n_ext, stream);
    const hipError_t ec = hipStreamEndCapture(s, &graph);
    if (rc != BSY_OK || ec != hipSuccess || !graph || hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        p->graph_unavailable = true;
        if (rc != BSY_OK) return rc;  // the plan itself is at fault: report it
        return bsy_plan_run(p, ext, n_ext, stream);
    }
    (void)hipGraphDestroy(graph);
    if (p->graphs.size() >= BSY_GRAPH_MAX) { (void)hipGraphExecDestroy(p->graphs.front().exec); p->graphs.erase(p->graphs.begin()); }
    p->graphs.push_back(bsy_plan::Captured{key, gen, wgen, exec});
    if (captured) *captured = 1;
    HIP_TRY(hipGraphLaunch(exec, s));
    return BSY_OK;
}

// Per-op autotuning of the conv kernel configuration (tile shape / K-step / ring depth): runs the plan once, timing
// every valid configuration of every conv op with HIP events on `stream` (1 warm-up + 3 timed launches each) and
// records the fastest in the plan.  All configurations of a layer are bit-identical in their results: the K walk is a function of the
// layer's shape (conv_select.hip conv_korder), never of the configuration.
extern "C" int bsy_plan_autotune(bsy_plan* p, void* const* ext, int n_ext, bsy_stream stream) {
    if (!p || (n_ext && !ext)) BSY_FAIL(BSY_ERR_ARG, "plan_autotune: bad argument");
    p->drop_graphs();
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    Resolver R = p->resolver(ext, n_ext);
    int rc = BSY_OK;
    for (size_t i = 0; i < p->ops.size() && rc == BSY_OK; ++i) {
        bsy_op& op = p->ops[i];
        if (op.kind != BSY_OP_CONV || op.tuned_cfg > 0 || op.prec != 0) { rc = run_op(op, R, p->weights(), s); continue; }  // preset (bsy_plan_set_tuning): kept
        ConvArgs a;
        if (!build_conv(a, op, R, p->weights())) { rc = BSY_ERR_ARG; break; }
        int cand[BSY_CONV_MAX_CFG];
        const int nc = conv_candidates(a, cand, BSY_CONV_MAX_CFG);
        // Candidates are timed ROUND-ROBIN (three rounds; per round one warm-up + a burst of five launches each) and ranked by
        // their best burst: clock ramps and neighbours' activity drift over a sweep, and timing every candidate in every phase
        // of it keeps near-ties from going to whichever kernel happened to run in a quiet moment (r02: the same layer flipped
        // between a 0.045 ms and a 0.056 ms configuration from box to box).
        float best_of[BSY_CONV_MAX_CFG];
        for (int c = 0; c < nc; ++c) best_of[c] = 1e30f;
        for (int round = 0; round < 3 && rc == BSY_OK; ++round)
            for (int c = 0; c < nc && rc == BSY_OK; ++c) {
                a.cfg = cand[c];
                rc = launch_conv(a, s);  // warm-up
                if (rc != BSY_OK) break;
                if (hipEventRecord(e0, s) != hipSuccess) { rc = BSY_ERR_HIP; break; }
                for (int r = 0; r < 5 && rc == BSY_OK; ++r) rc = launch_conv(a, s);
                if (rc != BSY_OK) break;
                float ms = 0.f;
                if (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                    hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { rc = BSY_ERR_HIP; bsy_set_error("plan_autotune: event timing failed"); break; }
                if (ms < best_of[c]) best_of[c] = ms;
            }
        float best = 1e30f;
        int best_cfg = cand[0];
        for (int c = 0; c < nc; ++c)
            if (best_of[c] < best) { best = best_of[c]; best_cfg = cand[c]; }
        if (rc != BSY_OK) break;
        op.tuned_cfg = best_cfg + 1;
        a.cfg = best_cfg;
        rc = launch_conv(a, s);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

// HOST array out[n_ops]: the configuration id chosen for each op (-1 = not a conv / not tuned).
extern "C" int bsy_plan_get_tuning(bsy_plan* p, int32_t* out, int n) {
    if (!p || !out || n != (int)p->ops.size()) BSY_FAIL(BSY_ERR_ARG, "plan_get_tuning: bad argument");
    for (int i = 0; i < n; ++i) out[i] = p->ops[i].kind == BSY_OP_CONV ? p->ops[i].tuned_cfg - 1 : -1;
    return BSY_OK;
}

// HOST array cfg[n_ops]: >= 0 presets that configuration for op i (a later bsy_plan_autotune leaves the op alone), -1 keeps
// the op as it is, -2 clears it (heuristic / to be tuned).  A preset that is not valid for the op's shape is ignored at launch.
extern "C" int bsy_plan_set_tuning(bsy_plan* p, const int32_t* cfg, int n) {
    if (!p || !cfg || n != (int)p->ops.size()) BSY_FAIL(BSY_ERR_ARG, "plan_set_tuning: bad argument");
    p->drop_graphs();  // captured forwards hold the old configurations' launches
    for (int i = 0; i < n; ++i) {
        if (p->ops[i].kind != BSY_OP_CONV || cfg[i] == -1) continue;
        p->ops[i].tuned_cfg = cfg[i] >= 0 ? cfg[i] + 1 : 0;
    }
    return BSY_OK;
}

// HOST array valid[n_ops]: 1 = the configuration preset for op i (bsy_plan_set_tuning) can run the op's shape, 0 = it cannot (a launch
// would fall back to the heuristic configuration: a stale or foreign tune cache), -1 = not a conv op or not preset.  Launches nothing.
extern "C" int bsy_plan_check_tuning(bsy_plan* p, void* const* ext, int n_ext, int32_t* valid, int n) {
    if (!p || !valid || (n_ext && !ext) || n != (int)p->ops.size()) BSY_FAIL(BSY_ERR_ARG, "plan_check_tuning: bad argument");
    Resolver R = p->resolver(ext, n_ext);
    for (int i = 0; i < n; ++i) {
        const bsy_op& op = p->ops[i];
        valid[i] = -1;
        if (op.kind != BSY_OP_CONV || op.tuned_cfg <= 0 || op.prec != 0) continue;
        ConvArgs a;
        if (!build_conv(a, op, R, p->weights())) return BSY_ERR_ARG;
        valid[i] = conv_cfg_valid(a, op.tuned_cfg - 1) ? 1 : 0;
    }
    return BSY_OK;
}

extern "C" int bsy_plan_copy_buffer(bsy_plan* p, int buf, void* host_dst, size_t bytes) {
    if (!p || !host_dst || buf < 0 || (size_t)buf >= p->buf_off.size()) BSY_FAIL(BSY_ERR_ARG, "copy_buffer: bad argument");
    if (bytes > p->buf_size[buf]) BSY_FAIL(BSY_ERR_ARG, "copy_buffer: %zu > buffer size %zu", bytes, p->buf_size[buf]);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_dst, p->base() + p->buf_off[buf], bytes, hipMemcpyDeviceToHost));
    return BSY_OK;
}

extern "C" int bsy_plan_profile(bsy_plan* p, void* const* ext, int n_ext, bsy_stream stream, float* ms_per_op) {
    if (!p || !ms_per_op || (n_ext && !ext)) BSY_FAIL(BSY_ERR_ARG, "plan_profile: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t n = p->ops.size();
    constexpr size_t NCAL = 16;  // empty event intervals recorded after the ops: the cost of the event pair itself
    while (p->events.size() < n + 1 + NCAL) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreate(&ev));
        p->events.push_back(ev);
    }
    Resolver R = p->resolver(ext, n_ext);
    HIP_TRY(hipEventRecord(p->events[0], s));
    for (size_t i = 0; i < n; ++i) {
        const int rc = run_op(p->ops[i], R, p->weights(), s);
        if (rc != BSY_OK) return rc;
        HIP_TRY(hipEventRecord(p->events[i + 1], s));
    }
    for (size_t i = 0; i < NCAL; ++i) HIP_TRY(hipEventRecord(p->events[n + 1 + i], s));
    HIP_TRY(hipEventSynchronize(p->events[n + NCAL]));
    // An interval between two recorded events holds the kernel AND the event packet between it and its neighbour (a few
    // microseconds that a normal run, which records no events between kernels, does not pay: rocprofv3's kernel
    // durations are that much shorter).  The median empty interval measures it; it is subtracted from every op.
    float cal[NCAL];
    for (size_t i = 0; i < NCAL; ++i) HIP_TRY(hipEventElapsedTime(&cal[i], p->events[n + i], p->events[n + 1 + i]));
    std::sort(cal, cal + NCAL);
    const float ev_ms = cal[NCAL / 2];
    for (size_t i = 0; i < n; ++i) {
        HIP_TRY(hipEventElapsedTime(&ms_per_op[i], p->events[i], p->events[i + 1]));
        ms_per_op[i] = ms_per_op[i] > ev_ms ? ms_per_op[i] - ev_ms : 0.f;
    }
    p->last_event_overhead_ms = ev_ms;
    return BSY_OK;
}

// In-place autotune: every candidate configuration of every untuned conv op is timed WHERE IT RUNS -- serial profile passes of the
// whole forward (bsy_plan_profile's event scheme), pass k running candidate k of every op at once, `rounds` passes per candidate index,
// best time kept -- instead of back-to-back launches of one layer, which see their operands in L2 / Infinity Cache and ranked near-ties
// differently from the forward (round 2: re-timing just the top three in place already moved the forward by 0.6-2.4 %).  Ops with a
// preset (bsy_plan_set_tuning) are left alone.  Costs max_i(#candidates) x rounds forwards (~0.4 s for YOLO11s at 64 x 640 x 640).
extern "C" int bsy_plan_autotune_in_place(bsy_plan* p, void* const* ext, int n_ext, bsy_stream stream, int rounds) {
    if (!p || (n_ext && !ext) || rounds < 1 || rounds > 16) BSY_FAIL(BSY_ERR_ARG, "plan_autotune_in_place: bad argument");
    p->drop_graphs();
    hipStream_t s = (hipStream_t)stream;
    const size_t n = p->ops.size();
    Resolver R = p->resolver(ext, n_ext);
    std::vector<std::vector<int>> cand(n);
    size_t K = 0;
    for (size_t i = 0; i < n; ++i) {  // one plain pass: the operands of every op exist, and the conv ops yield their arguments
        bsy_op& op = p->ops[i];
        if (op.kind == BSY_OP_CONV && op.tuned_cfg <= 0 && op.prec == 0) {
            ConvArgs a;
            if (!build_conv(a, op, R, p->weights())) return BSY_ERR_ARG;
            int list[BSY_CONV_MAX_CFG];
            const int nc = conv_candidates(a, list, BSY_CONV_MAX_CFG);
            cand[i].assign(list, list + (nc > 0 ? nc : 0));
            K = cand[i].size() > K ? cand[i].size() : K;
        }
        const int rc = run_op(op, R, p->weights(), s);
        if (rc != BSY_OK) return rc;
    }
    if (K == 0) return BSY_OK;
    std::vector<float> best(n, 1e30f), ms(n);
    std::vector<std::vector<float>> tk(n);  // best time of every candidate
    for (size_t i = 0; i < n; ++i) tk[i].assign(cand[i].size(), 1e30f);
    std::vector<int> best_c(n, -1);
    for (size_t i = 0; i < n; ++i)
        if (!cand[i].empty()) best_c[i] = cand[i][0];
    for (size_t k = 0; k < K; ++k) {
        for (size_t i = 0; i < n; ++i)
            if (!cand[i].empty()) p->ops[i].tuned_cfg = (k < cand[i].size() ? cand[i][k] : best_c[i]) + 1;
        for (int r = 0; r < rounds; ++r) {
            const int rc = bsy_plan_profile(p, ext, n_ext, stream, ms.data());
            if (rc != BSY_OK) {
                for (size_t i = 0; i < n; ++i)
                    if (!cand[i].empty()) p->ops[i].tuned_cfg = 0;
                return rc;
            }
            for (size_t i = 0; i < n; ++i)
                if (k < cand[i].size()) {
                    if (ms[i] < tk[i][k]) tk[i][k] = ms[i];
                    if (ms[i] < best[i]) { best[i] = ms[i]; best_c[i] = cand[i][k]; }
                }
        }
    }
    for (size_t i = 0; i < n; ++i)
        if (!cand[i].empty()) p->ops[i].tuned_cfg = best_c[i] + 1;
    return BSY_OK;
}
