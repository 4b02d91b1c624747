// The engine and plan objects behind the C ABI (include/bsyolo.h), shared by engine.hip (their lifecycle) and plan_ops.hip (run_op).
#pragma once
#include <vector>

#include "op_args.h"

struct bsy_engine {
    int device = 0;
    void* weights = nullptr;
    size_t weight_bytes = 0;
    // ONE activation arena shared by every plan created with bsy_plan_create_arena (sized for the largest of them; a plan
    // addresses it through host-assigned offsets).  Grows, never shrinks; plans resolve the base at run time.
    char* arena = nullptr;
    size_t arena_bytes = 0;
    unsigned arena_gen = 0;  // bumped whenever the arena moves: captured graphs hold its addresses
    unsigned weights_gen = 0;  // bumped by every bsy_engine_load_weights: captured graphs hold addresses inside the weight blob too
};

struct bsy_plan {
    bsy_engine* eng = nullptr;
    std::vector<bsy_op> ops;
    std::vector<size_t> buf_off;
    std::vector<size_t> buf_size;
    char* workspace = nullptr;     // plan-owned workspace (bsy_plan_create) ...
    size_t workspace_bytes = 0;
    bool use_arena = false;        // ... or the engine's shared arena (bsy_plan_create_arena): base = eng->arena
    char* base() const { return use_arena ? eng->arena : workspace; }
    const char* weights() const { return (const char*)eng->weights; }
    // the views of one call (bsy_plan_run and its kin): bases and external slots are looked up when the call starts
    Resolver resolver(void* const* ext, int n_ext) const { return Resolver{base(), buf_off.data(), buf_off.size(), ext, n_ext}; }
    std::vector<hipEvent_t> events;
    // side streams ("lanes") for independent op chains + the events that fork / join them
    std::vector<hipStream_t> lanes;      // index 0 unused (lane 0 = caller's stream)
    std::vector<hipEvent_t> lane_done;   // per lane: recorded at its tail before a join
    std::vector<hipEvent_t> lane_fork;   // per lane: recorded on the caller's stream where the lane forks (one event per lane:
                                         // an event that still has a waiter pending is never re-recorded)
    float last_event_overhead_ms = 0.f;  // bsy_plan_profile: median empty event interval of the last call
    size_t guard = 0;                    // bytes of guard band behind every buffer (BSY_PLAN_GUARD)
    // captured forwards (bsy_plan_graph_launch): one executable graph per set of external pointers, oldest first
    struct Captured {
        std::vector<void*> ext;
        unsigned arena_gen, weights_gen;
        hipGraphExec_t exec;
    };
    std::vector<Captured> graphs;
    bool graph_unavailable = false;      // a capture failed once: this plan runs eagerly from then on
    void drop_graphs() {
        for (auto& g : graphs) (void)hipGraphExecDestroy(g.exec);
        graphs.clear();
    }
};

// plan_ops.hip: one op record -> its launch on `s` (wb = the engine's weight blob)
int run_op(const bsy_op& op, Resolver& R, const char* wb, hipStream_t s);
