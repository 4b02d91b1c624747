// Classify's tail for gfx950 (nn/modules/head.py:300-304 and the argsort ClassificationPredictor / ClassificationValidator take of its
// output, classify/predict.py:51-60, val.py:56-60): y = softmax(logits) in fp32, x = the logits, and the k most probable classes of
// every image, whole batch in ONE launch, no host synchronisation, no allocation, no float atomics.
//   block = image; thread t owns classes t, t + threads, t + 2 threads, ... in every pass (256 threads up to 2048 classes, else 1024).
//   pass 1: row maximum (and the logit copy);  pass 2: e = exp(logit - max) and its sum;  pass 3: y = e / sum rounded to the output
//   dtype;  then k rounds of a block-wide arg-max over 64-bit keys (ord_key(stored y) << 32 | ~class): round j takes the largest key
//   below round j - 1's.  Keys are unique, so the order is total: higher stored probability first, then the lower class -- a stable
//   descending sort, which is what the reference's argsort gives where probabilities differ.
// The row lives in LDS where it fits (CLS_LDS_NC classes: logit, then e, then the stored y in the same word); a longer row is read
// from memory in each pass and the rounds read back the thread's OWN y stores.  Both forms do the same arithmetic in the same order:
// per-thread sums in class order, a butterfly inside the wave, the waves in order.  The block size depends on nc alone, so an image
// gets the same bits whatever the batch.
#include "postproc.h"

#include <math.h>

#define CLS_MAX_NC 65536
#define CLS_MAX_K 16
#define CLS_LDS_NC 32768  // 128 KiB of row; the CU has 160 KiB
#define CLS_THREADS 1024

struct ClsK {
    const float* logits;  // (B, ld)
    int ld, nc, k;
    void* y;              // (B, nc)
    void* x;              // (B, nc) or null
    int32_t* idx;         // (B, k)
    float* val;           // (B, k)
};

template <typename T, bool LDS>
__global__ __launch_bounds__(CLS_THREADS) void classify_tail_kernel(const ClsK p) {
    extern __shared__ float row[];  // LDS form: nc floats
    __shared__ float redf[CLS_THREADS / 64];
    __shared__ u64 redk[CLS_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int nc = p.nc;
    const float* lg = p.logits + (size_t)b * p.ld;
    T* y = reinterpret_cast<T*>(p.y) + (size_t)b * nc;
    T* x = p.x ? reinterpret_cast<T*>(p.x) + (size_t)b * nc : nullptr;

    // pass 1: the row maximum.  fmaxf skips NaN: a row that holds one gets NaN from every exp below, as torch's softmax gives
    float m = -INFINITY;
    for (int i = tid; i < nc; i += nt) {
        const float v = lg[i];
        if (LDS) row[i] = v;
        if (x) x[i] = (T)v;
        m = fmaxf(m, v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) redf[wave] = m;
    __syncthreads();
    m = redf[0];
    for (int w = 1; w < nw; ++w) m = fmaxf(m, redf[w]);
    __syncthreads();  // redf is rewritten below

    // pass 2: e = exp(logit - max) (at most 1: no overflow) and its sum
    float sum = 0.f;
    for (int i = tid; i < nc; i += nt) {
        const float e = expf((LDS ? row[i] : lg[i]) - m);
        if (LDS) row[i] = e;
        sum += e;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) redf[wave] = sum;
    __syncthreads();
    sum = redf[0];
    for (int w = 1; w < nw; ++w) sum += redf[w];

    // pass 3: the probabilities as stored
    for (int i = tid; i < nc; i += nt) {
        const float e = LDS ? row[i] : expf(lg[i] - m);
        const T q = (T)(e / sum);
        y[i] = q;
        if (LDS) row[i] = (float)q;
    }

    // the k most probable classes: every round scans the thread's own classes (its own LDS words / its own stores to y)
    u64 bound = ~0ull;  // above every key: ord_key is at most 0xffc00000
    for (int j = 0; j < p.k; ++j) {
        u64 mine = 0ull;  // below every key: ord_key is at least 0x007fffff
        float mv = 0.f;
        for (int i = tid; i < nc; i += nt) {
            const float v = LDS ? row[i] : (float)y[i];
            const u64 key = ((u64)ord_key(v) << 32) | (u64)(~(unsigned)i);
            if (key < bound && key > mine) { mine = key; mv = v; }
        }
        u64 best = mine;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u64 o = __shfl_xor(best, off, 64);
            best = o > best ? o : best;
        }
        if (lane == 0) redk[wave] = best;
        __syncthreads();
        best = redk[0];
        for (int w = 1; w < nw; ++w) best = redk[w] > best ? redk[w] : best;
        __syncthreads();  // redk is rewritten by the next round
        if (mine == best && best != 0ull) {  // its owner (k <= nc: every round finds a key)
            p.idx[(size_t)b * p.k + j] = (int32_t)(~(unsigned)(best & 0xffffffffull));
            p.val[(size_t)b * p.k + j] = mv;  // the stored probability (its NaN payload), not the ranking key
        }
        bound = best;
    }
}

int launch_classify_tail(const float* logits, int ld, int B, int nc, void* y, void* x, int out_dtype, int k, int32_t* topk_idx,
                         float* topk_val, hipStream_t s) {
    if (!logits || !y) BSY_FAIL(BSY_ERR_ARG, "classify_tail: null pointer");
    if (out_dtype != BSY_F16 && out_dtype != BSY_F32) BSY_FAIL(BSY_ERR_ARG, "classify_tail: dtype %d unsupported", out_dtype);
    if (nc < 1 || nc > CLS_MAX_NC) BSY_FAIL(BSY_ERR_ARG, "classify_tail: nc %d out of range (1..%d)", nc, CLS_MAX_NC);
    if (B < 1 || B > 65535) BSY_FAIL(BSY_ERR_ARG, "classify_tail: B %d out of range (1..65535)", B);
    if (k < 0 || k > CLS_MAX_K || k > nc) BSY_FAIL(BSY_ERR_ARG, "classify_tail: k %d out of range (0..min(nc, %d))", k, CLS_MAX_K);
    if (k > 0 && (!topk_idx || !topk_val)) BSY_FAIL(BSY_ERR_ARG, "classify_tail: k = %d without top-k outputs", k);
    if (ld < nc || (ld & 3)) BSY_FAIL(BSY_ERR_ARG, "classify_tail: ld %d must be a multiple of 4 and >= nc = %d", ld, nc);
    const uintptr_t esz = out_dtype == BSY_F16 ? 2 : 4;
    if (((uintptr_t)logits & 15) || ((uintptr_t)y & (esz - 1)) || ((uintptr_t)x & (esz - 1)) ||
        (k > 0 && (((uintptr_t)topk_idx & 3) || ((uintptr_t)topk_val & 3))))
        BSY_FAIL(BSY_ERR_ARG, "classify_tail: misaligned pointer (logits: 16 bytes, the others: their element)");
    ClsK p;
    p.logits = logits; p.ld = ld; p.nc = nc; p.k = k; p.y = y; p.x = x; p.idx = topk_idx; p.val = topk_val;
    const bool lds = nc <= CLS_LDS_NC;
    const size_t dyn = lds ? (size_t)nc * sizeof(float) : 0;
    // Above 64 KiB of LDS a launch needs the function attribute (gfx950 has 160 KiB per CU).  It belongs to the current device, so it is
    // set with every such launch (rows past 16384 classes: rare) and not remembered in a per-process flag.
    if (dyn > 65536) {
        const int lds_max = CLS_LDS_NC * (int)sizeof(float);
        if (out_dtype == BSY_F16)
            HIP_TRY(hipFuncSetAttribute((const void*)classify_tail_kernel<half_t, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        else
            HIP_TRY(hipFuncSetAttribute((const void*)classify_tail_kernel<float, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    }
    const int threads = nc <= 2048 ? 256 : CLS_THREADS;
    dispatch_dtype(out_dtype, [&](auto t) {
        if (lds) hipLaunchKernelGGL((classify_tail_kernel<decltype(t), true>), dim3(B), dim3(threads), dyn, s, p);
        else hipLaunchKernelGGL((classify_tail_kernel<decltype(t), false>), dim3(B), dim3(threads), 0, s, p);
    });
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

extern "C" int bsy_classify_tail(const float* logits, int ld, int B, int nc, void* y, void* x, int out_dtype, int k, int32_t* topk_idx,
                                 float* topk_val, bsy_stream stream) {
    return launch_classify_tail(logits, ld, B, nc, y, x, out_dtype, k, topk_idx, topk_val, (hipStream_t)stream);
}
