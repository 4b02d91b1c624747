// MaxSigmoidAttnBlock's gate for gfx950 (nn/modules/block.py:3483-3515, the extra chunk of YOLO-World's C2fAttn): per pixel p and head m
//     t = max_n  sum_k embed[p][m hc + k] * G[n][m hc + k]  + bias[m],        dst[p][m hc + j] = proj[p][m hc + j] * scale[m] * sigmoid(t)
// with G the text rows behind the block's Linear, 1 / sqrt(hc) folded in by the host (weights.py kind "maxsig").  A skinny GEMM
// (pixels x hc) . (hc x nc) whose epilogue is a max over the classes: with an open vocabulary (LVIS: 1203 rows) it is more
// multiply-adds per pixel than the 1x1 convs around it.
//
// fp16 storage: v_mfma_f32_32x32x16_f16 with the CLASSES on the accumulator's rows and the PIXELS on its columns.  A wave owns 32 pixels of
// one head.  Its B operand -- 32 pixels x hc channels, lane = pixel (lane & 31), 16 bytes per k-step straight from the NHWC map -- is read
// once and stays in registers (hc / 16 fragments).  The A operand is 32 guide rows, lane = class (lane & 31), 16 bytes of that row per
// k-step; the guide is streamed from memory block by block of 32 classes (1203 classes at C = 256 are 616 KB: L2-resident, not LDS-sized),
// the next block's fragments in flight while this block's hc / 16 MFMAs run.  After each block the running maximum is 16 max operations
// per lane (accumulator register r of lane l holds class (r & 3) + 8 (r >> 2) + 4 (l >> 5) of pixel l & 31); after the last block the 16
// registers fold into one and lanes l and l ^ 32 exchange theirs: every lane then holds its pixel's maximum.  The guide's rows are padded to
// a multiple of 32 with copies of row 0, so a padding row never wins.  The gate is applied in a plain pass over the wave's 32 x hc
// elements, 16 bytes per lane, consecutive lanes on consecutive bytes of a pixel.  No LDS, no barrier, no atomics.
// A dot product's summation order is the MFMA's (a function of hc alone) and a maximum has none: a pixel's bits do not depend on the
// batch, on its place in the map or on which wave computed it.  Pixels past the end of a partial block read the LAST pixel's row (a valid
// address; every column of the product is independent) and store nothing.
//
// fp32 storage (fp32 and fp32x modes): one thread per (pixel, head), one fmaf chain per class in k order starting at 0, the head's
// embedding in LDS where it fits ([k][thread]: conflict-free), sigmoid = 1 / (1 + expf(-t)) as silu32 of common.h.
#include "common.h"

#include <math.h>

template <int KS>  // hc = 16 KS
__global__ __launch_bounds__(256) void maxsig16_kernel(const half_t* __restrict__ embed, int lde, const half_t* proj, int ldp, half_t* dst, int ldd,
                                                       long long P, int heads, int nblk, const half_t* __restrict__ G, int C,
                                                       const float* __restrict__ bs) {
    constexpr int HC = 16 * KS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long unit = (long long)blockIdx.x * 4 + wave;  // (pixel block, head), the head fastest
    const long long pb = unit / heads;
    const int m = (int)(unit - pb * heads);
    if (pb * 32 >= P) return;  // (the whole wave: nothing below synchronises across waves)
    const int col = lane & 31, lh = lane >> 5;
    const long long p = pb * 32 + col, pl = p < P ? p : P - 1;
    const half_t* e = embed + (size_t)pl * lde + m * HC + 8 * lh;
    half8 b[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) b[ks] = *reinterpret_cast<const half8*>(e + 16 * ks);
    const half_t* g = G + (size_t)col * C + m * HC + 8 * lh;
    half8 a[KS], an[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) an[ks] = a[ks] = *reinterpret_cast<const half8*>(g + 16 * ks);
    f32x16 mx;
#pragma unroll
    for (int r = 0; r < 16; ++r) mx[r] = -INFINITY;
    for (int blk = 0; blk < nblk; ++blk) {
        if (blk + 1 < nblk) {
            const half_t* gn = g + (size_t)(blk + 1) * 32 * C;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) an[ks] = *reinterpret_cast<const half8*>(gn + 16 * ks);
        }
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[ks], b[ks], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) mx[r] = fmaxf(mx[r], acc[r]);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = an[ks];
    }
    float t = mx[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) t = fmaxf(t, mx[r]);
    t = fmaxf(t, __shfl_xor(t, 32, 64));
    t += bs[m];
    const float gate = bs[heads + m] * (1.0f / (1.0f + expf(-t)));
    // the gate: 32 pixels x 2 KS chunks of 16 bytes, lane i on chunk i % (2 KS) of pixel i / (2 KS) (32 * 2 KS is a multiple of 64: every
    // lane takes part in every round's shuffle)
    constexpr int NCH = 2 * KS;
    for (int i = lane; i < 32 * NCH; i += 64) {
        const int px = i / NCH, ch = i - px * NCH;
        const float gv = __shfl(gate, px, 64);
        const long long q = pb * 32 + px;
        if (q < P) {
            const half8 v = *reinterpret_cast<const half8*>(proj + (size_t)q * ldp + m * HC + 8 * ch);
            half8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)v[j] * gv);
            *reinterpret_cast<half8*>(dst + (size_t)q * ldd + m * HC + 8 * ch) = o;
        }
    }
}

#define MAXSIG32_THREADS 64
#define MAXSIG32_LDS_HC 256  // 64 KiB of embedding per block

template <bool LDS>
__global__ __launch_bounds__(MAXSIG32_THREADS) void maxsig32_kernel(const float* __restrict__ embed, int lde, const float* proj, int ldp, float* dst,
                                                                    int ldd, long long P, int heads, int hc, int nc, const float* __restrict__ G, int C,
                                                                    const float* __restrict__ bs) {
    extern __shared__ float se[];  // LDS form: [hc][threads], a thread reads its own column alone (no barrier)
    const int m = blockIdx.y, tid = threadIdx.x;
    const long long p = (long long)blockIdx.x * MAXSIG32_THREADS + tid;
    const bool live = p < P;
    const float* e = embed + (size_t)(live ? p : P - 1) * lde + m * hc;
    if (LDS)
        for (int k = 0; k < hc; ++k) se[k * MAXSIG32_THREADS + tid] = e[k];
    const float* g = G + m * hc;
    float mx = -INFINITY;
    for (int n = 0; n < nc; ++n) {
        const float* gn = g + (size_t)n * C;
        float s = 0.0f;
        for (int k = 0; k < hc; ++k) s = fmaf(LDS ? se[k * MAXSIG32_THREADS + tid] : e[k], gn[k], s);
        mx = fmaxf(mx, s);
    }
    const float t = mx + bs[m];
    const float gate = bs[heads + m] * (1.0f / (1.0f + expf(-t)));
    if (live) {
        const float* s1 = proj + (size_t)p * ldp + m * hc;
        float* d = dst + (size_t)p * ldd + m * hc;
        for (int j = 0; j < hc; ++j) d[j] = s1[j] * gate;
    }
}

// Whether two views of C channels over P pixels (first elements a and b, row strides lda and ldb, element size esz) share an element.
// Views of one buffer (equal strides, addresses a whole number of elements apart) may interleave: they overlap where their channel
// windows do.  Anything else overlaps where the address ranges do.
static bool views_overlap(const void* a, int lda, const void* b, int ldb, long long P, int C, int esz) {
    const long long ua = (long long)(uintptr_t)a, ub = (long long)(uintptr_t)b;
    const long long ea = ua + ((P - 1) * lda + C) * esz, eb = ub + ((P - 1) * ldb + C) * esz;
    if (ea <= ub || eb <= ua) return false;
    if (lda != ldb || (ub - ua) % esz) return true;
    long long off = ((ub - ua) / esz) % lda;
    if (off < 0) off += lda;
    return off < C || off + C > lda;
}

int launch_maxsig(const MaxSigArgs& a, hipStream_t s) {
    if (!a.embed || !a.proj || !a.dst || !a.G || !a.bias_scale) BSY_FAIL(BSY_ERR_ARG, "maxsig: null pointer");
    if (a.dtype != BSY_F16 && a.dtype != BSY_F32) BSY_FAIL(BSY_ERR_ARG, "maxsig: dtype %d (f16 or f32 storage)", a.dtype);
    if (a.nc < 1) BSY_FAIL(BSY_ERR_ARG, "maxsig: nc = %d (at least one guide row)", a.nc);
    if (a.B < 1 || a.HW < 1 || a.heads < 1 || a.heads > 65535 || a.hc < 1)
        BSY_FAIL(BSY_ERR_ARG, "maxsig: %d images of %d pixels, %d heads of %d channels", a.B, a.HW, a.heads, a.hc);
    const bool f16 = a.dtype == BSY_F16;
    if (f16 && !maxsig_supported(a.hc)) BSY_FAIL(BSY_ERR_ARG, "maxsig: heads of hc = %d channels are not on the fp16 path (16 to 128 in steps of 16)", a.hc);
    const long long C = (long long)a.heads * a.hc, P = (long long)a.B * a.HW;
    if (C > (1 << 20) || a.lde < C || a.ldp < C || a.ldd < C) BSY_FAIL(BSY_ERR_ARG, "maxsig: row strides %d / %d / %d below the %lld channels", a.lde, a.ldp, a.ldd, C);
    const int esz = f16 ? 2 : 4;
    const uintptr_t mask = f16 ? 15 : 3;
    if ((f16 && ((a.lde | a.ldp | a.ldd) & 7)) || (((uintptr_t)a.embed | (uintptr_t)a.proj | (uintptr_t)a.dst | (uintptr_t)a.G) & mask) ||
        ((uintptr_t)a.bias_scale & 3))
        BSY_FAIL(BSY_ERR_ARG, "maxsig: f16 views need row strides in multiples of 8 and 16-byte aligned pointers (f32: 4-byte)");
    if (views_overlap(a.embed, a.lde, a.dst, a.ldd, P, (int)C, esz)) BSY_FAIL(BSY_ERR_ARG, "maxsig: the destination overlaps the embedding view (src0)");
    if (f16) {
        const long long units = (P + 31) / 32 * a.heads, blocks = (units + 3) / 4;
        if (blocks > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "maxsig: %lld pixels x %d heads exceed one launch", P, a.heads);
        const int nblk = (a.nc + 31) / 32;
#define MAXSIG16(KS)                                                                                                                        \
    case KS:                                                                                                                                \
        hipLaunchKernelGGL((maxsig16_kernel<KS>), dim3((unsigned)blocks), dim3(256), 0, s, (const half_t*)a.embed, a.lde, (const half_t*)a.proj, \
                           a.ldp, (half_t*)a.dst, a.ldd, P, a.heads, nblk, (const half_t*)a.G, (int)C, a.bias_scale);                           \
        break;
        switch (a.hc / 16) {
            MAXSIG16(1) MAXSIG16(2) MAXSIG16(3) MAXSIG16(4) MAXSIG16(5) MAXSIG16(6) MAXSIG16(7) MAXSIG16(8)
        }
#undef MAXSIG16
    } else {
        const long long blocks = (P + MAXSIG32_THREADS - 1) / MAXSIG32_THREADS;
        if (blocks > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "maxsig: %lld pixels exceed one launch", P);
        const dim3 grid((unsigned)blocks, (unsigned)a.heads);
        if (a.hc <= MAXSIG32_LDS_HC) {
            const size_t dyn = (size_t)a.hc * MAXSIG32_THREADS * sizeof(float);
            hipLaunchKernelGGL((maxsig32_kernel<true>), grid, dim3(MAXSIG32_THREADS), dyn, s, (const float*)a.embed, a.lde, (const float*)a.proj, a.ldp,
                               (float*)a.dst, a.ldd, P, a.heads, a.hc, a.nc, (const float*)a.G, (int)C, a.bias_scale);
        } else {
            hipLaunchKernelGGL((maxsig32_kernel<false>), grid, dim3(MAXSIG32_THREADS), 0, s, (const float*)a.embed, a.lde, (const float*)a.proj, a.ldp,
                               (float*)a.dst, a.ldd, P, a.heads, a.hc, a.nc, (const float*)a.G, (int)C, a.bias_scale);
        }
    }
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
