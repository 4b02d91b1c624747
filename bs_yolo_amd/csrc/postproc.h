// Building blocks shared by the postprocess units nms.hip, obb.hip, sahi.hip, topk.hip and classify.hip (val_ap.hip takes the
// size helpers only; align256 itself is common.h's, for engine.hip and op_args.h).  Everything here is inline: a __global__ lives in exactly one unit (the key sort: nms.hip) and is reached
// from the others through the host launchers declared at the end.
//   host:   pow2_at_least, align256, Carver (workspace layout, measured and carved by the same calls), dispatch_dtype
//   device: block_bitonic_desc, greedy_resolve_256, kept_rank / block_kept_rank, first_max_class, score_key / decode_score_key, ord_key
// What is NOT shared, on purpose: the overlap tests (iou_gt, nmm_matched, has_match64) round differently because each mirrors
// its own reference; they stay with their units.
#pragma once
#include "common.h"

typedef unsigned long long u64;

#define NMS_MAX_DET 4096      // bsy_nms / bsy_nms_rotated: the greedy kernel keeps its kept boxes in LDS, 20 bytes each
#define SORT_LDS_KEYS 8192    // key_sort_kernel: segments up to this many keys are sorted in LDS, longer ones in global memory

// ---- host helpers -------------------------------------------------------------------------------------------------------
// The power of two >= n, at least 2 (the bitonic networks need a pair).
template <typename I>
__host__ __device__ inline I pow2_at_least(I n) {
    I p = 2;
    while (p < n) p <<= 1;
    return p;
}

// Bump allocator over a caller's workspace.  Each unit describes its layout ONCE, as a function that runs the same align() /
// take() calls with the real base pointer (the pointers are used) or with nullptr (only `need` is used: the *_workspace_bytes
// entry point).  `need` is a bound that holds for any alignment of the base, which is why align() costs a full 256 there.
struct Carver {
    uintptr_t at;
    size_t need = 0;
    explicit Carver(void* base) : at((uintptr_t)base) {}
    void align() {
        at = (uintptr_t)align256((size_t)at);
        need += 256;
    }
    template <typename T>
    T* take(size_t count, bool padded = false) {  // padded: the block's size is rounded up to 256, so the next one stays aligned
        const size_t bytes = padded ? align256(count * sizeof(T)) : count * sizeof(T);
        T* r = (T*)at;
        at += bytes;
        need += bytes;
        return r;
    }
};

// f(T{}) with T = half_t or float: one launch sequence written once for both prediction dtypes (the caller has checked the code).
template <typename F>
static inline void dispatch_dtype(int dtype, F f) {
    if (dtype == BSY_F16) f(half_t{});
    else f(float{});
}

// ---- sort ---------------------------------------------------------------------------------------------------------------
// Block-wide bitonic network, descending, over a[0 .. np2), np2 a power of two (1: nothing to do); the caller has published a[]
// with a barrier, every step ends with one.  Called once per address space: after inlining the compiler knows whether `a` is LDS
// or global memory and emits ds_* / global_* accesses, never flat ones -- do not fold two call sites into one over a selected pointer.
template <typename P>
__device__ __forceinline__ void block_bitonic_desc(P a, int np2) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += nt) {
                const int l = i ^ j;
                if (l > i) {
                    const u64 x = a[i], y = a[l];
                    const bool desc = (i & k) == 0;  // descending overall
                    if (desc ? (x < y) : (x > y)) { a[i] = y; a[l] = x; }
                }
            }
            __syncthreads();
        }
}

// ---- ordered compaction -------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_kept(int count) { return count; }
__device__ __forceinline__ int wave_kept(u64 mask) { return __popcll(mask); }

// Rank, in thread order, of lane `lane` of wave `wave` among a block's kept lanes: the kept lanes of the waves before it plus
// those below it in its own wave's mask.  per_wave[NW]: every wave's keep mask (u64) or kept count (int), registers or LDS.
template <int NW, typename W>
__device__ __forceinline__ int kept_rank(const W* per_wave, int wave, u64 own_mask, int lane) {
    int before = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) before += w < wave ? wave_kept(per_wave[w]) : 0;
    return before + __popcll(own_mask & ((1ull << lane) - 1ull));
}

// The same for a flag per thread of a block of NW waves: cnt is LDS, [NW].  One barrier inside; the caller puts another before
// the next call rewrites cnt.  total = the block's kept lanes (the same value in every thread).
template <int NW>
__device__ __forceinline__ int block_kept_rank(bool kept, int* cnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 m = __ballot(kept);
    if (lane == 0) cnt[wave] = __popcll(m);
    __syncthreads();
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) total += cnt[w];
    return kept_rank<NW>(cnt, wave, m, lane);
}

// ---- greedy resolve -----------------------------------------------------------------------------------------------------
struct GreedyLds {  // the caller's LDS (a dynamic layout or static arrays)
    u64 *keepw, *supw, *alw;  // [4] each: keep / suppressed / alive bit per candidate of the chunk
    int* undecided;           // [1]
};

// Greedy suppression inside a chunk of 256 candidates in priority order (thread = candidate, 256 threads), WITHOUT 256 serial
// steps.  `alive`: the candidate exists and survived the test against everything kept before the chunk.  pair_matches(j): does
// this candidate overlap candidate j < tid of the chunk (staged by the caller, published by the first barrier here).
// Fixed point on the 256x256 overlap bitmask: keep = every overlapping earlier candidate is suppressed; suppressed = some
// overlapping earlier candidate is kept -- the sequential greedy order exactly.  Candidate 0 decides in the first round and each
// round decides at least the first undecided one, hence the bound of 257.
// Returns this candidate's state, 1 = keep or 2 = suppressed (or not alive); mrow = the earlier alive candidates of the chunk it
// overlaps, keep = the chunk's keep bits (plain arrays, not a struct: they are indexed by wave and must stay in registers).
// The caller puts a barrier before the next call, which clears the words.
template <typename F>
__device__ __forceinline__ int greedy_resolve_256(bool alive, F pair_matches, const GreedyLds& sh, u64 (&mrow)[4], u64 (&keep)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 4) { sh.keepw[tid] = 0ull; sh.supw[tid] = 0ull; }
    const u64 aliveb = __ballot(alive);
    if (lane == 0) sh.alw[wave] = aliveb;
    __syncthreads();
    u64 alivew[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) { alivew[w] = sh.alw[w]; mrow[w] = 0ull; }
    if (alive)
        for (int j = 0; j < tid; ++j) {
            if (!((alivew[j >> 6] >> (j & 63)) & 1ull)) continue;
            if (pair_matches(j)) mrow[j >> 6] |= 1ull << (j & 63);
        }
    int state = alive ? 0 : 2;  // 0 = undecided
    if (!alive) atomicOr(&sh.supw[wave], 1ull << lane);
    for (int it = 0; it < 257; ++it) {
        if (tid == 0) *sh.undecided = 0;
        __syncthreads();  // the words of the previous round (and the clear above) are complete
        u64 kw[4], sw[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) { kw[w] = sh.keepw[w]; sw[w] = sh.supw[w]; }
        int ns = state;
        if (state == 0) {
            bool hit = false, pending = false;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                hit |= (mrow[w] & kw[w]) != 0ull;
                pending |= (mrow[w] & ~(kw[w] | sw[w])) != 0ull;
            }
            if (hit) ns = 2;
            else if (!pending) ns = 1;
        }
        __syncthreads();  // everyone has read keepw / supw
        if (ns != state) {
            if (ns == 1) atomicOr(&sh.keepw[wave], 1ull << lane);
            else atomicOr(&sh.supw[wave], 1ull << lane);
            state = ns;
        }
        if (state == 0) atomicAdd(sh.undecided, 1);
        __syncthreads();
        if (*sh.undecided == 0) break;
        __syncthreads();  // everyone has read the counter before the next round clears it
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) keep[w] = sh.keepw[w];
    return state;
}

// ---- score keys and the best class --------------------------------------------------------------------------------------
// Best class of one anchor = FIRST maximum (utils/ops.py:274 cls.max(1)); cp = the anchor's score of class 0, rows A apart.
template <typename T>
__device__ __forceinline__ int first_max_class(const T* cp, int A, int nc, float& best) {
    best = (float)cp[0];
    int bc = 0;
    for (int c = 1; c < nc; ++c) {
        const float s = (float)cp[(size_t)c * A];
        if (s > best) { best = s; bc = c; }
    }
    return bc;
}

// fp32 score bits << 32 | ~candidate index: ONE descending sort gives "score descending, ties by ascending index".
__device__ __forceinline__ u64 score_key(float score, unsigned idx) { return ((u64)__float_as_uint(score) << 32) | (u64)(~idx); }

// float -> unsigned with the same order (NaN above +inf, as torch's topk ranks it; -0 == +0).  Used for ranking only: the rows
// carry the scores as stored
__device__ __forceinline__ unsigned ord_key(float f) {
    unsigned u = __float_as_uint(f);
    if (f != f) u = 0x7fc00000u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The inverse.  The index is anchor * nc + class with multi_label, else the anchor, whose class is looked up again;
// pb = the image's prediction (4 + nc + .. rows of A).
template <typename T>
__device__ __forceinline__ void decode_score_key(u64 k, int nc, int multi_label, const T* pb, int A, float& score, int& anchor, int& cls) {
    score = __uint_as_float((unsigned)(k >> 32));
    const unsigned idx = ~(unsigned)(k & 0xffffffffull);
    if (multi_label) {
        anchor = (int)(idx / (unsigned)nc);
        cls = (int)(idx - (unsigned)anchor * nc);
    } else {
        anchor = (int)idx;
        float best;
        cls = first_max_class(pb + (size_t)4 * A + anchor, A, nc, best);
    }
}

// ---- host launchers owned by nms.hip ------------------------------------------------------------------------------------
// Sorts `segments` key lists descending in place, one workgroup each: segment b is keys[b * stride ..) with counts[b] keys.
// stride is a power of two >= the longest count (the sort pads a long segment with zero keys up to a power of two).
int launch_key_sort(u64* keys, int stride, const int32_t* counts, int segments, hipStream_t s);
// bsy_nms's candidate keys: confidence / class filter + sort (nms.hip steps 1-2), for bsy_nms itself and for bsy_nms_rotated.
// in_place: the filter also rewrites the boxes xywh -> xyxy.  multi_label is already reduced (nc > 1).
int nms_candidates(void* pred, int pred_dtype, int B, int nc, int C, int A, float conf_thres, const int32_t* classes, int n_classes,
                   int multi_label, int in_place, int cap, u64* keys, int32_t* cand_count, hipStream_t s);
// The argument checks the two NMS entry points share, with their messages; op = "nms" / "nms_rotated", extra = "nm" / "ne".
int nms_check_args(const char* op, const char* extra, const void* pred, const void* out, const void* counts, const void* workspace,
                   int pred_dtype, int B, int nc, int n_extra, int A, float conf_thres, float iou_thres, int max_det, int max_nms);
