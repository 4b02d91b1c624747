// The pooling front end of YOLOv9's downsampling blocks (block.py:3692-3723), NHWC, fp16 or fp32 storage, HBM-bound:
//   AConv : avg_pool2d(x, 2, 1, 0, False, True) -> Conv 3x3 s2 p1
//   ADown : the same average pool, chunk(2, 1); first half -> Conv 3x3 s2 p1; second half -> max_pool2d(., 3, 2, 1) -> Conv 1x1
// Mode 0 writes the averaged map of an even H x W input on an H x W map whose last row and column are ZERO: a 3x3 stride-2
// pad-1 conv over that map reads exactly what it reads from the (H-1) x (W-1) pooled map plus its zero padding, so the conv that
// follows is an ordinary even-sized one.  Mode 1 writes max_pool2d(avg_pool2d(x), 3, 2, 1) on an H/2 x W/2 map straight from x
// (a 4 x 4 input window per output; -inf padding, so it never sees the zero border of mode 0); the pooled map is not stored.
// Arithmetic is ATen's: the average is ((x00 + x01) + x10) + x11 in fp32, times 0.25, rounded once to the storage type before
// the max -- both modes return F.avg_pool2d / F.max_pool2d's bits.
// One lane owns one 16-byte piece (8 fp16 / 4 fp32 channels) of one output pixel: one 16-byte load per tap through a buffer
// descriptor (out-of-range taps read zeros and are masked out of the max), one 16-byte store; lanes run along C, so both are
// coalesced.  blockIdx.y is the image: the descriptor's base is wave-uniform and every offset inside an image fits 32 bits.
#include "common.h"

namespace {
template <typename T> struct Pd;
template <> struct Pd<half_t> { typedef half8 vec; static constexpr int N = 8; };
template <> struct Pd<float> { typedef f32x4 vec; static constexpr int N = 4; };

// avg2x2 of the window whose corners are a (top left), b (top right), c, d, rounded to T, as f32
template <typename T>
__device__ __forceinline__ void pd_avg(const typename Pd<T>::vec& a, const typename Pd<T>::vec& b, const typename Pd<T>::vec& c,
                                       const typename Pd<T>::vec& d, float (&o)[Pd<T>::N]) {
#pragma unroll
    for (int e = 0; e < Pd<T>::N; ++e) {
        const float s = (((float)a[e] + (float)b[e]) + (float)c[e]) + (float)d[e];
        o[e] = (float)(T)(s * 0.25f);
    }
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void pool_down_kernel(const T* __restrict__ src, int lds_, T* __restrict__ dst, int ldd, int H, int W,
                                                        int C, unsigned span) {
    typedef typename Pd<T>::vec vec;
    constexpr int N = Pd<T>::N;
    const int CV = C / N;
    const int OH = MODE ? H >> 1 : H, OW = MODE ? W >> 1 : W;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned)OH * (unsigned)OW * (unsigned)CV) return;
    const int c = (int)(idx % (unsigned)CV) * N;
    const unsigned pix = idx / (unsigned)CV;
    const int j = (int)(pix % (unsigned)OW), i = (int)(pix / (unsigned)OW);
    const size_t n = blockIdx.y;
    const bsy_rsrc_t rs = make_rsrc(src + n * (size_t)H * W * lds_, span);
    // byte offset of this lane's piece of input pixel (y0 + r, x0 + q) = rowoff[r] + coloff[q]; a tap outside the map reads at an
    // out-of-range offset (zeros).  Selects, no branches: the offsets are a handful of integer operations per lane.
    const int y0 = MODE ? 2 * i - 1 : i, x0 = MODE ? 2 * j - 1 : j;
    constexpr int TAPS = MODE ? 4 : 2;
    unsigned rowoff[TAPS], coloff[TAPS];
    bool rowok[TAPS], colok[TAPS];
#pragma unroll
    for (int r = 0; r < TAPS; ++r) {
        rowok[r] = (unsigned)(y0 + r) < (unsigned)H;
        colok[r] = (unsigned)(x0 + r) < (unsigned)W;
        rowoff[r] = (unsigned)sizeof(T) * (unsigned)(y0 + r) * (unsigned)W * (unsigned)lds_;
        coloff[r] = (unsigned)sizeof(T) * ((unsigned)(x0 + r) * (unsigned)lds_ + (unsigned)c);
    }
    auto off = [&](int r, int q) -> unsigned { return (rowok[r] & colok[q]) ? rowoff[r] + coloff[q] : BSY_OOB; };
    vec o;
    if (MODE == 0) {
        if (i < H - 1 && j < W - 1) {
            const vec a = buf_load16<vec>(rs, off(0, 0)), b = buf_load16<vec>(rs, off(0, 1));
            const vec p = buf_load16<vec>(rs, off(1, 0)), q = buf_load16<vec>(rs, off(1, 1));
            float r[N];
            pd_avg<T>(a, b, p, q, r);
#pragma unroll
            for (int e = 0; e < N; ++e) o[e] = (T)r[e];
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) o[e] = (T)0.0f;
        }
    } else {
        // pooled positions (2i-1+a, 2j-1+b), a, b in 0..2, inside [0, H-2] x [0, W-2]; input rows / columns 2i-1 .. 2i+2
        vec x[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) x[r][q] = buf_load16<vec>(rs, off(r, q));
        float m[N];
#pragma unroll
        for (int e = 0; e < N; ++e) m[e] = -INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const bool ok = ((unsigned)(y0 + a) < (unsigned)(H - 1)) & ((unsigned)(x0 + b) < (unsigned)(W - 1));
                float v[N];
                pd_avg<T>(x[a][b], x[a][b + 1], x[a + 1][b], x[a + 1][b + 1], v);
#pragma unroll
                for (int e = 0; e < N; ++e) m[e] = (ok & ((v[e] > m[e]) | (v[e] != v[e]))) ? v[e] : m[e];  // a NaN wins and stays, as in ATen
            }
#pragma unroll
        for (int e = 0; e < N; ++e) o[e] = (T)m[e];
    }
    *reinterpret_cast<vec*>(dst + ((n * OH + i) * OW + j) * (size_t)ldd + c) = o;
}

template <typename T>
int pool_down_t(const T* src, int lds_, T* dst, int ldd, int B, int H, int W, int C, int mode, hipStream_t s) {
    constexpr int N = Pd<T>::N;
    const int OH = mode ? H / 2 : H, OW = mode ? W / 2 : W;
    const long long lanes = (long long)OH * OW * (C / N);                                // per image
    const long long span = (((long long)H * W - 1) * lds_ + C) * (long long)sizeof(T);  // bytes of one image's view
    if (lanes >= (1LL << 31) || span >= (1LL << 31)) BSY_FAIL(BSY_ERR_ARG, "pool_down: an image of the source view exceeds 2^31 bytes");
    if (B > 65535) BSY_FAIL(BSY_ERR_ARG, "pool_down: batch %d (at most 65535 images per launch)", B);
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)B);
    if (mode) hipLaunchKernelGGL((pool_down_kernel<T, 1>), grid, dim3(256), 0, s, src, lds_, dst, ldd, H, W, C, (unsigned)span);
    else hipLaunchKernelGGL((pool_down_kernel<T, 0>), grid, dim3(256), 0, s, src, lds_, dst, ldd, H, W, C, (unsigned)span);
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
}  // namespace

// src / dst: the buffers' first element (NOT offset); soff / doff: first channel of the views
int launch_pool_down(const void* src, int lds_, int soff, void* dst, int ldd, int doff, int B, int H, int W, int C, int mode, int dtype,
                     hipStream_t s) {
    if (!src || !dst) BSY_FAIL(BSY_ERR_ARG, "pool_down: null pointer");
    if (dtype != BSY_F16 && dtype != BSY_F32) BSY_FAIL(BSY_ERR_ARG, "pool_down: dtype %d (f16 or f32 storage)", dtype);
    if (mode != 0 && mode != 1) BSY_FAIL(BSY_ERR_ARG, "pool_down: mode %d (0 averaged map with a zero border, 1 stride-2 max of it)", mode);
    if (B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) BSY_FAIL(BSY_ERR_ARG, "pool_down: %d images of %d x %d (even sizes >= 2)", B, H, W);
    const int v = dtype == BSY_F16 ? 8 : 4;
    if (C < v || C % v || lds_ % v || ldd % v || soff % v || doff % v || soff < 0 || doff < 0 || soff + C > lds_ || doff + C > ldd ||
        ((uintptr_t)src & 15) || ((uintptr_t)dst & 15))
        BSY_FAIL(BSY_ERR_ARG, "pool_down: channels, row strides and channel offsets must be multiples of %d inside their rows, buffers 16-byte aligned", v);
    if (dtype == BSY_F16) return pool_down_t<half_t>((const half_t*)src + soff, lds_, (half_t*)dst + doff, ldd, B, H, W, C, mode, s);
    return pool_down_t<float>((const float*)src + soff, lds_, (float*)dst + doff, ldd, B, H, W, C, mode, s);
}
