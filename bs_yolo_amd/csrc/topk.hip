// End-to-end (NMS-free) detection postprocess for gfx950: v10Detect.postprocess (nn/modules/head.py:151-172), whole batch,
// no host synchronisation, no allocation.  Two kernels per call:
//   1. topk_amax_kernel   (thread = anchor; four anchors for f16 with A % 4 == 0): the best class score of every anchor in the prediction's own dtype, stored as an
//      order-preserving 32-bit key (scores.amax(dim=-1), :167).
//   2. topk_select_kernel (block = image, 1024 threads):
//        stage 1 -- the K = min(max_det, A) anchors with the highest best-class score (topk of the amax, :167): a radix select
//                   on 64-bit keys (score key << 32 | ~anchor) finds the K-th key, one pass collects the K anchors (LDS);
//        stage 2 -- the K highest of the K x nc gathered class scores (:170): the gathered keys (score key << 32 |
//                   ~(anchor * nc + class)) go to the workspace, a second radix select finds the K-th, the K winners are
//                   collected into LDS and sorted descending (postproc.h block_bitonic_desc); row j = [box of the anchor, score,
//                   class] (:172).
// Keys are unique (the anchor / anchor-class index is in the low word), so "key >= K-th key" selects exactly K, and the order
// is total: higher score first, then lower anchor index, then lower class -- torch's topk leaves equal values in an unspecified
// order.  The selection compares the stored scores (f16 predictions: the f16 values, as the reference's half model does).
// The radix select walks 8-bit digits from the top; a digit whose bin holds exactly the keys still needed ends it early.
#include "postproc.h"

#define TOPK_MAX_K 4096  // max_det bound: the stage-2 winners are sorted in LDS
#define TOPK_THREADS 1024
#define TOPK_MAX_AN (1LL << 30)  // bound on A * nc
#define TOPK_U 8  // keys a thread loads before it uses the first: the passes are bound by L2 latency, not bandwidth

struct TopkK {
    const void* pred;  // (B, 4 + nc, A)
    int B, nc, A, K;
    unsigned* amax;    // workspace: B x A score keys
    u64* gath;         // workspace: B x K x nc stage-2 keys
    float* out;        // (B, K, 6)
};

template <typename T>
__global__ __launch_bounds__(256) void topk_amax_kernel(const TopkK p) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (a >= p.A) return;
    const T* cp = reinterpret_cast<const T*>(p.pred) + ((size_t)b * (4 + p.nc) + 4) * p.A + a;
    float m = (float)cp[0];
    for (int c = 1; c < p.nc; ++c) {
        const float s = (float)cp[(size_t)c * p.A];
        if (s > m || s != s) m = (m != m) ? m : s;  // amax propagates NaN
    }
    p.amax[(size_t)b * p.A + a] = ord_key(m);
}

// f16 predictions with A % 4 == 0: four anchors per thread, every class row read as 8-byte pieces (the one-anchor form issues
// nc two-byte loads per lane; nms.hip's nms_filter4_kernel makes the same change).  Same keys.
__global__ __launch_bounds__(256) void topk_amax4_kernel(const TopkK p) {
    const int a0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int b = blockIdx.y;
    if (a0 >= p.A) return;
    const half_t* cp = reinterpret_cast<const half_t*>(p.pred) + ((size_t)b * (4 + p.nc) + 4) * p.A + a0;
    const half4 v0 = *reinterpret_cast<const half4*>(cp);
    float m[4] = {(float)v0[0], (float)v0[1], (float)v0[2], (float)v0[3]};
    for (int c = 1; c < p.nc; ++c) {
        const half4 v = *reinterpret_cast<const half4*>(cp + (size_t)c * p.A);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = (float)v[j];
            if (s > m[j] || s != s) m[j] = (m[j] != m[j]) ? m[j] : s;
        }
    }
    unsigned* o = p.amax + (size_t)b * p.A + a0;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = ord_key(m[j]);
}

// Shared state of one radix select (block-wide).
struct SelState {
    unsigned hist[256];
    unsigned v[3];  // need, digit, done
};

// The key such that exactly `need` of the n keys key(i) are >= it (keys unique, need <= n).  Every thread of the block calls it.
template <typename F>
__device__ u64 radix_threshold(F key, int n, unsigned need, SelState& st) {
    const int tid = threadIdx.x;
    u64 prefix = 0ull, mask = 0ull;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += TOPK_THREADS) st.hist[i] = 0u;
        __syncthreads();
        for (int i0 = tid; i0 < n; i0 += TOPK_U * TOPK_THREADS) {
            u64 kk[TOPK_U];
#pragma unroll
            for (int j = 0; j < TOPK_U; ++j) {
                const int i = i0 + j * TOPK_THREADS;
                kk[j] = i < n ? key(i) : 0ull;
            }
#pragma unroll
            for (int j = 0; j < TOPK_U; ++j)
                if (i0 + j * TOPK_THREADS < n && (kk[j] & mask) == prefix) atomicAdd(&st.hist[(unsigned)(kk[j] >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {
            // lane l holds bins 255 - 4l .. 252 - 4l; an inclusive scan from the top bin finds the bin of the need-th key
            unsigned c[4], s = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = st.hist[255 - 4 * tid - j]; s += c[j]; }
            unsigned inc = s;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned v = __shfl_up(inc, off, 64);
                if (tid >= off) inc += v;
            }
            unsigned cum = inc - s;
            if (cum < need && inc >= need) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (cum + c[j] >= need) {
                        st.v[0] = need - cum;
                        st.v[1] = 255u - 4u * tid - j;
                        st.v[2] = c[j] == need - cum;
                        break;
                    }
                    cum += c[j];
                }
            }
        }
        __syncthreads();
        need = st.v[0];
        prefix |= (u64)st.v[1] << shift;
        mask |= 0xffull << shift;
        const bool done = st.v[2] != 0u;
        __syncthreads();  // st.v is rewritten by the next digit
        if (done) break;  // every key under this prefix is taken: lower digits 0 is the threshold
    }
    return prefix;
}

template <typename T>
__global__ __launch_bounds__(TOPK_THREADS) void topk_select_kernel(const TopkK p) {
    __shared__ SelState st;
    __shared__ unsigned sel[TOPK_MAX_K];  // stage-1 anchors (any order: stage 2's keys carry the anchor)
    __shared__ u64 sk[TOPK_MAX_K];        // stage-2 winners
    __shared__ unsigned cnt;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int A = p.A, nc = p.nc, K = p.K;
    const T* pb = reinterpret_cast<const T*>(p.pred) + (size_t)b * (4 + nc) * A;
    const unsigned* am = p.amax + (size_t)b * A;
    u64* g = p.gath + (size_t)b * K * nc;

    // stage 1: the K best anchors
    auto key1 = [&](int i) -> u64 { return ((u64)am[i] << 32) | (u64)(~(unsigned)i); };
    const u64 t1 = radix_threshold(key1, A, (unsigned)K, st);
    if (tid == 0) cnt = 0u;
    __syncthreads();
    for (int i0 = tid; i0 < A; i0 += TOPK_U * TOPK_THREADS) {
        u64 kk[TOPK_U];
#pragma unroll
        for (int j = 0; j < TOPK_U; ++j) {
            const int i = i0 + j * TOPK_THREADS;
            kk[j] = i < A ? key1(i) : 0ull;
        }
#pragma unroll
        for (int j = 0; j < TOPK_U; ++j)
            if (i0 + j * TOPK_THREADS < A && kk[j] >= t1) {
                const unsigned pos = atomicAdd(&cnt, 1u);
                if (pos < (unsigned)K) sel[pos] = (unsigned)(i0 + j * TOPK_THREADS);  // exactly K pass (unique keys); the bound is a guard
            }
    }
    __syncthreads();

    // stage 2: their K x nc class scores
    const int n2 = K * nc;
    for (int i0 = tid; i0 < n2; i0 += TOPK_U * TOPK_THREADS) {
        float sv[TOPK_U];
        unsigned lo[TOPK_U];
#pragma unroll
        for (int j = 0; j < TOPK_U; ++j) {
            const int i = i0 + j * TOPK_THREADS;
            sv[j] = 0.f;
            lo[j] = 0u;
            if (i < n2) {
                const int r = i / nc, c = i - r * nc;
                unsigned a = sel[r];
                if (a >= (unsigned)A) a = 0u;  // unreachable (exactly K anchors were collected); keeps every read in bounds
                sv[j] = (float)pb[(size_t)(4 + c) * A + a];
                lo[j] = ~(a * (unsigned)nc + (unsigned)c);
            }
        }
#pragma unroll
        for (int j = 0; j < TOPK_U; ++j)
            if (i0 + j * TOPK_THREADS < n2) g[i0 + j * TOPK_THREADS] = ((u64)ord_key(sv[j]) << 32) | (u64)lo[j];
    }
    __syncthreads();
    auto key2 = [&](int i) -> u64 { return g[i]; };
    const u64 t2 = radix_threshold(key2, n2, (unsigned)K, st);
    if (tid == 0) cnt = 0u;
    __syncthreads();
    for (int i0 = tid; i0 < n2; i0 += TOPK_U * TOPK_THREADS) {
        u64 kk[TOPK_U];
#pragma unroll
        for (int j = 0; j < TOPK_U; ++j) {
            const int i = i0 + j * TOPK_THREADS;
            kk[j] = i < n2 ? g[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < TOPK_U; ++j)
            if (i0 + j * TOPK_THREADS < n2 && kk[j] >= t2) {
                const unsigned pos = atomicAdd(&cnt, 1u);
                if (pos < (unsigned)K) sk[pos] = kk[j];
            }
    }
    int np2 = 1;  // (K = 1: nothing to sort)
    while (np2 < K) np2 <<= 1;
    for (int i = K + tid; i < np2; i += TOPK_THREADS) sk[i] = 0ull;  // sorts last: no real key is 0
    __syncthreads();
    block_bitonic_desc(sk, np2);

    float* ob = p.out + (size_t)b * K * 6;
    for (int j = tid; j < K; j += TOPK_THREADS) {
        const u64 k = sk[j];
        const unsigned idx = ~(unsigned)(k & 0xffffffffull);
        unsigned a = idx / (unsigned)nc;
        const unsigned c = idx - a * (unsigned)nc;
        if (a >= (unsigned)A) a = 0u;  // unreachable, as above
        float* o = ob + (size_t)j * 6;
        o[0] = (float)pb[a];
        o[1] = (float)pb[(size_t)A + a];
        o[2] = (float)pb[(size_t)2 * A + a];
        o[3] = (float)pb[(size_t)3 * A + a];
        o[4] = (float)pb[(size_t)(4 + c) * A + a];  // the stored score (its sign on -0, its NaN payload), not the ranking key
        o[5] = (float)c;
    }
}

// Workspace: one score key per anchor, then the K x nc stage-2 keys of every image.  With a null workspace only the returned size
// means anything.
static size_t topk_carve(void* workspace, int B, int A, int nc, size_t K, TopkK& k) {
    Carver c(workspace);
    c.align();
    k.amax = c.take<unsigned>((size_t)B * A, true);
    k.gath = c.take<u64>((size_t)B * K * nc, true);
    return c.need;
}

extern "C" size_t bsy_end2end_topk_workspace_bytes(int B, int A, int nc, int max_det) {
    if (B <= 0 || A <= 0 || nc <= 0 || max_det <= 0) return 0;
    TopkK measured;
    return topk_carve(nullptr, B, A, nc, (size_t)(max_det < A ? max_det : A), measured);
}

extern "C" int bsy_end2end_topk(const void* pred, int pred_dtype, int B, int nc, int A, int max_det, float* out, void* workspace,
                                size_t workspace_bytes, bsy_stream stream) {
    if (!pred || !out || !workspace) BSY_FAIL(BSY_ERR_ARG, "end2end_topk: null pointer");
    if (B <= 0 || B > 65535 || nc <= 0 || A <= 0) BSY_FAIL(BSY_ERR_ARG, "end2end_topk: bad sizes B=%d nc=%d A=%d", B, nc, A);
    if (max_det <= 0 || max_det > TOPK_MAX_K) BSY_FAIL(BSY_ERR_ARG, "end2end_topk: max_det %d out of range (1..%d)", max_det, TOPK_MAX_K);
    // A * nc <= 2^30: the stage-2 key index anchor * nc + class and every loop index (i0 + (TOPK_U - 1) * TOPK_THREADS) stay in int
    if ((long long)A * nc > TOPK_MAX_AN) BSY_FAIL(BSY_ERR_ARG, "end2end_topk: A*nc = %lld too large (<= 2^30)", (long long)A * nc);
    if (pred_dtype != BSY_F16 && pred_dtype != BSY_F32) BSY_FAIL(BSY_ERR_ARG, "end2end_topk: dtype %d unsupported", pred_dtype);
    const size_t need = bsy_end2end_topk_workspace_bytes(B, A, nc, max_det);
    if (workspace_bytes < need) BSY_FAIL(BSY_ERR_ARG, "end2end_topk: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    TopkK k;
    k.pred = pred; k.B = B; k.nc = nc; k.A = A; k.K = max_det < A ? max_det : A;
    topk_carve(workspace, B, A, nc, (size_t)k.K, k);
    k.out = out;
    if (pred_dtype == BSY_F16 && !(A & 3) && !((uintptr_t)pred & 7))
        hipLaunchKernelGGL(topk_amax4_kernel, dim3((A / 4 + 255) / 256, B), dim3(256), 0, s, k);
    else
        dispatch_dtype(pred_dtype, [&](auto t) {
            hipLaunchKernelGGL(topk_amax_kernel<decltype(t)>, dim3((A + 255) / 256, B), dim3(256), 0, s, k);
        });
    dispatch_dtype(pred_dtype, [&](auto t) {
        hipLaunchKernelGGL(topk_select_kernel<decltype(t)>, dim3(B), dim3(TOPK_THREADS), 0, s, k);
    });
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
