// The 2x2 max pools of YOLOv3-tiny (cfg/models/v3/yolov3-tiny.yaml), NHWC, fp16 or fp32 storage, HBM-bound:
//   mode 0 : nn.MaxPool2d(2, 2, 0) on an even H x W map -> H/2 x W/2
//   mode 1 : nn.ZeroPad2d((0, 1, 0, 1)) then nn.MaxPool2d(2, 1, 0) on H x W -> H x W.  The pad is part of the DATA, not of the pool:
//            a tap past the last row or column counts as 0.0 (not -inf), so an all-negative window on that border returns 0.
// The update rule is ATen's (pool_max.h): a NaN wins and stays.  Both modes return F.max_pool2d's bits.
// One lane owns one 16-byte piece (8 fp16 / 4 fp32 channels) of one output pixel, as in pool_down.hip: one 16-byte load per tap
// through a buffer descriptor -- an out-of-range tap reads zeros, which is exactly mode 1's padding value; mode 0 has no such tap --
// and one 16-byte store; lanes run along C, so both are coalesced.  blockIdx.y is the image: the descriptor's base is wave-uniform
// and every offset inside an image fits 32 bits.
#include "pool_max.h"

namespace {
template <typename T, int MODE>
__global__ __launch_bounds__(256) void maxpool_kernel(const T* __restrict__ src, int lds_, T* __restrict__ dst, int ldd, int H, int W, int C,
                                                      unsigned span) {
    typedef typename PoolVec<T>::vec vec;
    constexpr int N = PoolVec<T>::N;
    const int CV = C / N;
    const int OH = MODE ? H : H >> 1, OW = MODE ? W : W >> 1;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned)OH * (unsigned)OW * (unsigned)CV) return;
    const int c = (int)(idx % (unsigned)CV) * N;
    const unsigned pix = idx / (unsigned)CV;
    const int j = (int)(pix % (unsigned)OW), i = (int)(pix / (unsigned)OW);
    const size_t n = blockIdx.y;
    const bsy_rsrc_t rs = make_rsrc(src + n * (size_t)H * W * lds_, span);
    const int y0 = MODE ? i : 2 * i, x0 = MODE ? j : 2 * j;
    unsigned rowoff[2], coloff[2];
    bool rowok[2], colok[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        rowok[r] = y0 + r < H;
        colok[r] = x0 + r < W;
        rowoff[r] = (unsigned)sizeof(T) * (unsigned)(y0 + r) * (unsigned)W * (unsigned)lds_;
        coloff[r] = (unsigned)sizeof(T) * ((unsigned)(x0 + r) * (unsigned)lds_ + (unsigned)c);
    }
    auto off = [&](int r, int q) -> unsigned { return (rowok[r] & colok[q]) ? rowoff[r] + coloff[q] : BSY_OOB; };
    const vec a = buf_load16<vec>(rs, off(0, 0)), b = buf_load16<vec>(rs, off(0, 1));
    const vec p = buf_load16<vec>(rs, off(1, 0)), q = buf_load16<vec>(rs, off(1, 1));
    *reinterpret_cast<vec*>(dst + ((n * OH + i) * OW + j) * (size_t)ldd + c) = pool_max4<T>(a, b, p, q);
}

template <typename T>
int maxpool_t(const T* src, int lds_, T* dst, int ldd, int B, int H, int W, int C, int mode, hipStream_t s) {
    constexpr int N = PoolVec<T>::N;
    const int OH = mode ? H : H / 2, OW = mode ? W : W / 2;
    const long long lanes = (long long)OH * OW * (C / N);                               // per image
    const long long span = (((long long)H * W - 1) * lds_ + C) * (long long)sizeof(T);  // bytes of one image's view
    if (lanes >= (1LL << 31) || span >= (1LL << 31)) BSY_FAIL(BSY_ERR_ARG, "maxpool: an image of the source view exceeds 2^31 bytes");
    if (B > 65535) BSY_FAIL(BSY_ERR_ARG, "maxpool: batch %d (at most 65535 images per launch)", B);
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)B);
    if (mode) hipLaunchKernelGGL((maxpool_kernel<T, 1>), grid, dim3(256), 0, s, src, lds_, dst, ldd, H, W, C, (unsigned)span);
    else hipLaunchKernelGGL((maxpool_kernel<T, 0>), grid, dim3(256), 0, s, src, lds_, dst, ldd, H, W, C, (unsigned)span);
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
}  // namespace

// src / dst: the buffers' first element (NOT offset); soff / doff: first channel of the views
int launch_maxpool(const void* src, int lds_, int soff, void* dst, int ldd, int doff, int B, int H, int W, int C, int mode, int dtype,
                   hipStream_t s) {
    if (!src || !dst) BSY_FAIL(BSY_ERR_ARG, "maxpool: null pointer");
    if (dtype != BSY_F16 && dtype != BSY_F32) BSY_FAIL(BSY_ERR_ARG, "maxpool: dtype %d (f16 or f32 storage)", dtype);
    if (mode != 0 && mode != 1) BSY_FAIL(BSY_ERR_ARG, "maxpool: mode %d (0: 2x2 stride 2, 1: zero pad right / bottom + 2x2 stride 1)", mode);
    if (B < 1 || H < 1 || W < 1 || (mode == 0 && ((H & 1) || (W & 1))))
        BSY_FAIL(BSY_ERR_ARG, "maxpool: %d images of %d x %d (mode 0 takes even sizes)", B, H, W);
    const int v = dtype == BSY_F16 ? 8 : 4;
    if (C < v || C % v || lds_ % v || ldd % v || soff % v || doff % v || soff < 0 || doff < 0 || soff + C > lds_ || doff + C > ldd ||
        ((uintptr_t)src & 15) || ((uintptr_t)dst & 15))
        BSY_FAIL(BSY_ERR_ARG, "maxpool: channels, row strides and channel offsets must be multiples of %d inside their rows, buffers 16-byte aligned", v);
    if (dtype == BSY_F16) return maxpool_t<half_t>((const half_t*)src + soff, lds_, (half_t*)dst + doff, ldd, B, H, W, C, mode, s);
    return maxpool_t<float>((const float*)src + soff, lds_, (float*)dst + doff, ldd, B, H, W, C, mode, s);
}
