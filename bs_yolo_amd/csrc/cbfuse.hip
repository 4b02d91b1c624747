// CBFuse (nn/modules/block.py:3760-3772; YOLOv9e's second backbone), NHWC, fp16 or fp32 storage, one launch:
//   dst = sum(stack([interpolate(tap_i, size = last.shape[2:], mode = "nearest") for i] + [last]), 0)
// The engine takes image sizes in multiples of 32, so tap i is stored at (H >> k_i, W >> k_i) of the target with k_i in 0 .. 4, and
// nearest means source pixel (y >> k_i, x >> k_i).  k = 0 is an ordinary operand of the target's own size.
// SUM ORDER: an f32 accumulator starts at +0.0 and takes tap 0, tap 1, ..., tap n-1, then `last`, one f32 addition each -- the order in
// which torch.sum(torch.stack(...), 0) adds them on the CPU (its identity is +0.0 as well, so an all -0.0 column gives +0.0).  f16
// storage: the operands are widened exactly, the f32 sum is rounded once.
// IN PLACE: dst may be `last` itself (no __restrict__ on either): a lane reads its piece of `last` before it writes the piece at the same
// place, and no other lane touches it.  dst must not overlap a tap: other lanes read a tap's pixel 4^k times.
// Pure streaming, no LDS: one lane owns one 16-byte piece (8 f16 / 4 f32 channels) of one target pixel -- one 16-byte load per operand,
// one 16-byte store, lanes along C so both coalesce; the coarse taps are re-read by the 4^k pixels they cover and come from L2.  The
// walk is grid-stride over at most CBF_MAX_BLOCKS blocks.  Where a view's row stride, first channel or base is off a 16-byte boundary,
// or C is no multiple of the piece, the scalar form runs: one element per lane, the same sum in the same order, the same bits.
#include "common.h"

#define CBF_MAX_BLOCKS 2048  // 256 CUs x 8 blocks of 256 lanes; the rest of the items are walked grid-stride

namespace {
struct CbFuseTaps {
    const void* p[BSY_CBFUSE_MAX_TAPS];
    int ld[BSY_CBFUSE_MAX_TAPS];
    int shift[BSY_CBFUSE_MAX_TAPS];
};

template <typename T> struct CbfVec;
template <> struct CbfVec<half_t> { typedef half8 vec; static constexpr int N = 8; };
template <> struct CbfVec<float> { typedef f32x4 vec; static constexpr int N = 4; };

// V = channels per lane: CbfVec<T>::N (16-byte pieces) or 1 (the scalar form).  I = the type of the item index and of the three divisions
// that take it apart (channel piece, x, y, image): unsigned where the launch has fewer than 2^31 items -- every plan of the engine --, so
// that they are 32-bit divisions; long long beyond.  Element offsets are size_t in both.
template <typename T, int V, typename I>
__global__ __launch_bounds__(256) void cbfuse_kernel(CbFuseTaps taps, int n, const T* last, int ldl, T* dst, int ldd, int H, int W, int C,
                                                     I items) {
    typedef typename CbfVec<T>::vec vec;
    const I CV = (I)(C / V);
    const I step = (I)gridDim.x * 256;  // (at most 2^19: idx + step stays below 2^32)
    for (I idx = (I)blockIdx.x * 256 + threadIdx.x; idx < items; idx += step) {
        const int c = (int)(idx % CV) * V;
        const I pix = idx / CV;
        const int x = (int)(pix % (I)W);
        const I t = pix / (I)W;
        const int y = (int)(t % (I)H);
        const I img = t / (I)H;
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
#pragma unroll
        for (int i = 0; i < BSY_CBFUSE_MAX_TAPS; ++i) {
            if (i < n) {
                const int k = taps.shift[i];
                const size_t sp = ((size_t)img * (H >> k) + (y >> k)) * (size_t)(W >> k) + (x >> k);
                const T* q = (const T*)taps.p[i] + sp * taps.ld[i] + c;
                if (V > 1) {
                    const vec v = *reinterpret_cast<const vec*>(q);
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] += (float)v[j];
                } else {
                    acc[0] += (float)q[0];
                }
            }
        }
        const size_t dp = (size_t)pix;
        if (V > 1) {
            const vec v = *reinterpret_cast<const vec*>(last + dp * ldl + c);
            vec o;
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = (T)(acc[j] + (float)v[j]);
            *reinterpret_cast<vec*>(dst + dp * ldd + c) = o;
        } else {
            dst[dp * ldd + c] = (T)(acc[0] + (float)last[dp * ldl + c]);
        }
    }
}

// Whether a view of C channels over Pa pixels at `a` (row stride lda) shares an element with one over Pb pixels at `b` (ldb).  Views of one
// buffer at one resolution (equal strides and pixel counts, a whole number of elements apart) may interleave: they overlap where their
// channel windows do.  Anything else overlaps where the address ranges do.
bool cbf_overlap(const void* a, int lda, long long Pa, const void* b, int ldb, long long Pb, int C, int esz) {
    const long long ua = (long long)(uintptr_t)a, ub = (long long)(uintptr_t)b;
    const long long ea = ua + ((Pa - 1) * lda + C) * esz, eb = ub + ((Pb - 1) * ldb + C) * esz;
    if (ea <= ub || eb <= ua) return false;
    if (lda != ldb || Pa != Pb || (ub - ua) % esz) return true;
    long long off = ((ub - ua) / esz) % lda;
    if (off < 0) off += lda;
    return off < C || off + C > lda;
}

template <typename T>
int cbfuse_t(const CbFuseArgs& a, hipStream_t s) {
    constexpr int N = CbfVec<T>::N;
    CbFuseTaps taps;
    bool vec = a.C % N == 0 && a.ldl % N == 0 && a.ldd % N == 0 && !(((uintptr_t)a.last | (uintptr_t)a.dst) & 15);
    for (int i = 0; i < BSY_CBFUSE_MAX_TAPS; ++i) {
        const bool on = i < a.n;
        taps.p[i] = on ? a.tap[i] : nullptr;
        taps.ld[i] = on ? a.ldt[i] : 0;
        taps.shift[i] = on ? a.shift[i] : 0;
        if (on && (a.ldt[i] % N || ((uintptr_t)a.tap[i] & 15))) vec = false;
    }
    const long long P = (long long)a.B * a.H * a.W;
    const long long items = P * (vec ? a.C / N : a.C);
    const unsigned blocks = (unsigned)((items + 255) / 256 < CBF_MAX_BLOCKS ? (items + 255) / 256 : CBF_MAX_BLOCKS);
#define CBF_LAUNCH(V_, I_)                                                                                                                 \
    hipLaunchKernelGGL((cbfuse_kernel<T, V_, I_>), dim3(blocks), dim3(256), 0, s, taps, a.n, (const T*)a.last, a.ldl, (T*)a.dst, a.ldd, a.H, a.W, \
                       a.C, (I_)items)
    const bool small = items < (1LL << 31);
    if (vec && small) CBF_LAUNCH(N, unsigned);
    else if (vec) CBF_LAUNCH(N, long long);
    else if (small) CBF_LAUNCH(1, unsigned);
    else CBF_LAUNCH(1, long long);
#undef CBF_LAUNCH
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
}  // namespace

int launch_cbfuse(const CbFuseArgs& a, hipStream_t s) {
    if (!cbfuse_shape_ok(a.n, a.shift, a.H, a.W)) return BSY_ERR_ARG;
    if (a.dtype != BSY_F16 && a.dtype != BSY_F32) BSY_FAIL(BSY_ERR_ARG, "cbfuse: dtype %d (f16 or f32 storage)", a.dtype);
    if (!a.last || !a.dst) BSY_FAIL(BSY_ERR_ARG, "cbfuse: null pointer");
    if (a.B < 1 || a.C < 1 || a.C > (1 << 20)) BSY_FAIL(BSY_ERR_ARG, "cbfuse: %d images of %d channels", a.B, a.C);
    if (a.ldl < a.C || a.ldd < a.C) BSY_FAIL(BSY_ERR_ARG, "cbfuse: row strides %d / %d below the %d channels", a.ldl, a.ldd, a.C);
    const int esz = a.dtype == BSY_F16 ? 2 : 4;
    const long long P = (long long)a.B * a.H * a.W;
    if (P * (long long)(a.ldd > a.ldl ? a.ldd : a.ldl) >= (1LL << 40)) BSY_FAIL(BSY_ERR_ARG, "cbfuse: %lld pixels exceed one launch", P);
    if ((((uintptr_t)a.last | (uintptr_t)a.dst) & (esz - 1))) BSY_FAIL(BSY_ERR_ARG, "cbfuse: a view is not aligned to its element size");
    if (a.last != a.dst || a.ldl != a.ldd) {
        if (cbf_overlap(a.last, a.ldl, P, a.dst, a.ldd, P, a.C, esz))
            BSY_FAIL(BSY_ERR_ARG, "cbfuse: the destination overlaps the last input without being its view (in place: the same view)");
    }
    for (int i = 0; i < a.n; ++i) {
        if (!a.tap[i]) BSY_FAIL(BSY_ERR_ARG, "cbfuse: null pointer (tap %d)", i);
        if (a.ldt[i] < a.C) BSY_FAIL(BSY_ERR_ARG, "cbfuse: tap %d is narrower (row stride %d) than the %d channels", i, a.ldt[i], a.C);
        if ((uintptr_t)a.tap[i] & (esz - 1)) BSY_FAIL(BSY_ERR_ARG, "cbfuse: a view is not aligned to its element size");
        const long long Pt = (long long)a.B * (a.H >> a.shift[i]) * (a.W >> a.shift[i]);
        if (cbf_overlap(a.tap[i], a.ldt[i], Pt, a.dst, a.ldd, P, a.C, esz)) BSY_FAIL(BSY_ERR_ARG, "cbfuse: the destination overlaps tap %d", i);
    }
    return a.dtype == BSY_F16 ? cbfuse_t<half_t>(a, s) : cbfuse_t<float>(a, s);
}
