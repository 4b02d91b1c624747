// Test-time augmentation (augment=True) glue for gfx950: the input side (flip + bilinear resize + pad of every scaled pass) and
// the output side (descale / de-flip of the box rows, tail clipping and concatenation of the passes) of
// DetectionModel._predict_augment (nn/tasks.py:354-370).  Both are HBM-bound element maps: no atomics, bitwise deterministic.
//
// bsy_scale_img replaces scale_img (utils/torch_utils.py:430-442) applied to x.flip(fi): F.interpolate(bilinear,
// align_corners=False) + F.pad(value=0.447).  The arithmetic is ATen's device kernel upsample_bilinear2d_out_frame, step for step
// in fp32 (accscalar_t), so that the engine's scaled input is torch's on the device; the flip is a mirrored read index.
//
// bsy_tta_merge replaces _descale_pred (:372-380) + _clip_augmented (:382-391) + torch.cat(y, -1): per pass, the kept anchor window,
// rows 0..3 multiplied by the fp32 reciprocal of the scale (what torch on the device runs for `p /= python_float`) and rounded to
// the storage dtype, then `img_w - x` (flip 3) or `img_h - y` (flip 2) rounded again; the other rows copied.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;  // memory-bound: cap the grid and grid-stride the rest
constexpr int64_t kIntItems = INT32_MAX - (int64_t)kMaxBlocks * kThreads;  // 32-bit item index: its grid-stride step cannot overflow

template <typename T> struct Vec;
template <> struct Vec<half_t> { static constexpr int N = 8; typedef half8 type; };   // 16-B stores
template <> struct Vec<float> { static constexpr int N = 4; typedef f32x4 type; };    // 16-B stores

template <typename T>
__device__ __forceinline__ float ld(const T* p) { return (float)*p; }

// One thread = N adjacent output columns of one output row of one (b, c) plane.  I: the work-item index type -- 32-bit divisions
// unless the item count needs 64 bits (pointer offsets are 64-bit either way).
template <typename T, typename I>
__global__ __launch_bounds__(kThreads) void scale_img_kernel(const T* __restrict__ in, int64_t planes, int H, int W, int OH, int OW,
                                                             int PH, int PW, int flip, T* __restrict__ out) {
    constexpr int N = Vec<T>::N;
    const I nvec = (PW + N - 1) / N;
    const I total = (I)planes * PH * nvec;
    const float rh = (float)H / (float)OH;  // area_pixel_compute_scale, align_corners = false, no explicit scale
    const float rw = (float)W / (float)OW;
    const T pad = (T)0.447f;
    const bool vec_ok = (PW % N) == 0 && ((uintptr_t)out % 16) == 0;
    for (I i = (I)blockIdx.x * kThreads + threadIdx.x; i < total; i += (I)gridDim.x * kThreads) {
        const I rowi = i / nvec;  // plane * PH + oh
        const int x0 = (int)(i - rowi * nvec) * N;
        const int oh = (int)(rowi % PH);
        const int64_t plane = rowi / PH;
        const int64_t row = rowi;
        T v[N];
        if (oh >= OH) {
#pragma unroll
            for (int j = 0; j < N; ++j) v[j] = pad;
        } else {
            // area_pixel_compute_source_index (ATen UpSample.cuh) on the resized grid, then the ud mirror on the read
            float h1r = rh * ((float)oh + 0.5f) - 0.5f;
            h1r = h1r < 0.f ? 0.f : h1r;
            const int h1 = min((int)h1r, H - 1);  // (ATen does not clamp; the index is < H for every in-range oh)
            const int h1p = (h1 < H - 1) ? 1 : 0;
            const float h1lambda = h1r - (float)h1;
            const float h0lambda = 1.0f - h1lambda;
            int ra = h1, rb = h1 + h1p;
            if (flip == 2) { ra = H - 1 - ra; rb = H - 1 - rb; }
            const T* pa = in + (plane * H + ra) * (int64_t)W;
            const T* pb = in + (plane * H + rb) * (int64_t)W;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int ow = x0 + j;
                if (ow >= OW) {
                    v[j] = pad;
                    continue;
                }
                float w1r = rw * ((float)ow + 0.5f) - 0.5f;
                w1r = w1r < 0.f ? 0.f : w1r;
                const int w1 = min((int)w1r, W - 1);
                const int w1p = (w1 < W - 1) ? 1 : 0;
                const float w1lambda = w1r - (float)w1;
                const float w0lambda = 1.0f - w1lambda;
                int ca = w1, cb = w1 + w1p;
                if (flip == 3) { ca = W - 1 - ca; cb = W - 1 - cb; }
                const float val = h0lambda * (w0lambda * ld(pa + ca) + w1lambda * ld(pa + cb)) +
                                  h1lambda * (w0lambda * ld(pb + ca) + w1lambda * ld(pb + cb));
                v[j] = (T)val;
            }
        }
        T* op = out + row * PW + x0;
        if (vec_ok) {
            typename Vec<T>::type pk;
#pragma unroll
            for (int j = 0; j < N; ++j) pk[j] = v[j];
            *reinterpret_cast<typename Vec<T>::type*>(op) = pk;
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (x0 + j < PW) op[j] = v[j];
        }
    }
}

struct MergeArgs {
    const void* src[BSY_TTA_MAX_PASSES];
    int A[BSY_TTA_MAX_PASSES];      // anchors of each pass's prediction
    int a0[BSY_TTA_MAX_PASSES];     // kept window [a0, a0 + len)
    int cum[BSY_TTA_MAX_PASSES + 1];  // output column where each pass's window starts; cum[n] = total
    float inv[BSY_TTA_MAX_PASSES];  // fp32 reciprocal of the scale
    int flip[BSY_TTA_MAX_PASSES];
    int n, no, B;
    float img_h, img_w;
};

template <typename T>
__device__ __forceinline__ T descale(T x, float inv, int r, int flip, float img_h, float img_w) {
#pragma clang fp contract(off)  // the reference rounds to the storage dtype after each of its two tensor operations
    T d = (T)((float)x * inv);  // p[:, :4] /= scale
    if (r == 0 && flip == 3) d = (T)(img_w - (float)d);
    if (r == 1 && flip == 2) d = (T)(img_h - (float)d);
    return d;
}

template <typename T, int K>
__device__ __forceinline__ void pick_shifted(int sh, const T* w, T* v) {
    if constexpr (K < Vec<T>::N) {
        if (sh == K) {
#pragma unroll
            for (int j = 0; j < Vec<T>::N; ++j) v[j] = w[K + j];
        } else {
            pick_shifted<T, K + 1>(sh, w, v);
        }
    }
}

// v = p[0 .. N-1] for any element alignment of p, as one or two aligned 16-B loads and a register shift.  The loads stay inside the
// 16-B blocks that hold p[0] and p[N-1], so they never touch a page the elements do not.  The shift is the same for every thread
// of a row and pass: no divergence.
template <typename T>
__device__ __forceinline__ void load_vec(const T* p, T* v) {
    constexpr int N = Vec<T>::N;
    typedef typename Vec<T>::type V;
    const int sh = (int)(((uintptr_t)p / sizeof(T)) % N);
    const V* q = reinterpret_cast<const V*>(p - sh);
    const V lo = q[0];
    if (sh == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = lo[j];
        return;
    }
    const V hi = q[1];
    T w[2 * N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        w[j] = lo[j];
        w[N + j] = hi[j];
    }
    pick_shifted<T, 1>(sh, w, v);
}

// Element `col` of output row (b, r): its pass and its source.
template <typename T>
__device__ __forceinline__ T merge_one(const MergeArgs& a, int r, int64_t srow, int col) {
    int p = 0;
    while (p + 1 < a.n && col >= a.cum[p + 1]) ++p;
    const T x = ((const T*)a.src[p])[srow * a.A[p] + a.a0[p] + (col - a.cum[p])];
    return r < 4 ? descale<T>(x, a.inv[p], r, a.flip[p], a.img_h, a.img_w) : x;
}

// One workgroup = one output row (b, r) at a time (grid-strided over the B * no rows), one thread = N consecutive columns of it.
// An odd `total` starts rows anywhere inside a vector: the row's first `head` columns (up to the next 16-B boundary) and its last
// partial vector are stored element by element, everything between as aligned 16-B vectors.  A vector inside one pass's window
// (all but at most n - 1 per row) reads its N source elements as aligned 16-B loads (load_vec).
template <typename T>
__global__ __launch_bounds__(kThreads) void tta_merge_kernel(MergeArgs a, T* __restrict__ out) {
    constexpr int N = Vec<T>::N;
    const int total = a.cum[a.n];
    const int rows = a.B * a.no;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int r = row % a.no;
        const int64_t srow = row;  // (b * no + r): the same row index in every pass's (B, no, A_p)
        T* orow = out + (int64_t)row * total;
        const int head = (int)(((16 - ((uintptr_t)orow % 16)) % 16) / sizeof(T));  // (a T* is sizeof(T)-aligned)
        const int h = head < total ? head : total;
        if ((int)threadIdx.x < h) orow[threadIdx.x] = merge_one<T>(a, r, srow, threadIdx.x);
        for (int c0 = h + (int)threadIdx.x * N; c0 < total; c0 += kThreads * N) {
            int p = 0;
            while (p + 1 < a.n && c0 >= a.cum[p + 1]) ++p;
            T v[N];
            if (c0 + N <= a.cum[p + 1]) {  // one pass
                const T* sp = (const T*)a.src[p] + srow * a.A[p] + a.a0[p] + (c0 - a.cum[p]);
                const float inv = a.inv[p];
                const int fl = a.flip[p];
                T x[N];
                load_vec<T>(sp, x);
#pragma unroll
                for (int j = 0; j < N; ++j) v[j] = r < 4 ? descale<T>(x[j], inv, r, fl, a.img_h, a.img_w) : x[j];
            } else {
#pragma unroll
                for (int j = 0; j < N; ++j)
                    if (c0 + j < total) v[j] = merge_one<T>(a, r, srow, c0 + j);
            }
            if (c0 + N <= total) {
                typename Vec<T>::type pk;
#pragma unroll
                for (int j = 0; j < N; ++j) pk[j] = v[j];
                *reinterpret_cast<typename Vec<T>::type*>(orow + c0) = pk;
            } else {
#pragma unroll
                for (int j = 0; j < N; ++j)
                    if (c0 + j < total) orow[c0 + j] = v[j];
            }
        }
    }
}

int grid_for(int64_t items) {
    const int64_t g = (items + kThreads - 1) / kThreads;
    return (int)(g < kMaxBlocks ? (g > 0 ? g : 1) : kMaxBlocks);
}

}  // namespace

extern "C" int bsy_scale_img(const void* in, int dtype, int B, int C, int H, int W, int OH, int OW, int PH, int PW, int flip,
                             void* out, bsy_stream stream) {
    if (!in || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || OH > PH || OW > PW)
        BSY_FAIL(BSY_ERR_ARG, "scale_img: bad shape (B %d C %d %dx%d -> %dx%d padded %dx%d)", B, C, H, W, OH, OW, PH, PW);
    if (flip != 0 && flip != 2 && flip != 3) BSY_FAIL(BSY_ERR_ARG, "scale_img: flip %d (0, 2 = ud, 3 = lr)", flip);
    const int64_t planes = (int64_t)B * C;
    if (dtype == BSY_F16) {
        const int64_t items = planes * PH * ((PW + 7) / 8);
        hipLaunchKernelGGL((items < kIntItems ? scale_img_kernel<half_t, int> : scale_img_kernel<half_t, int64_t>), dim3(grid_for(items)),
                           dim3(kThreads), 0, (hipStream_t)stream, (const half_t*)in, planes, H, W, OH, OW, PH, PW, flip, (half_t*)out);
    } else if (dtype == BSY_F32) {
        const int64_t items = planes * PH * ((PW + 3) / 4);
        hipLaunchKernelGGL((items < kIntItems ? scale_img_kernel<float, int> : scale_img_kernel<float, int64_t>), dim3(grid_for(items)),
                           dim3(kThreads), 0, (hipStream_t)stream, (const float*)in, planes, H, W, OH, OW, PH, PW, flip, (float*)out);
    } else {
        BSY_FAIL(BSY_ERR_ARG, "scale_img: dtype %d unsupported", dtype);
    }
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

extern "C" int bsy_tta_merge(const void* const* src, const int32_t* A, const int32_t* a_begin, const int32_t* a_end,
                             const float* scale, const int32_t* flip, int n, int B, int no, int img_h, int img_w, int dtype,
                             void* out, bsy_stream stream) {
    if (!src || !A || !a_begin || !a_end || !scale || !flip || !out || n <= 0 || n > BSY_TTA_MAX_PASSES || B <= 0 || no < 4)
        BSY_FAIL(BSY_ERR_ARG, "tta_merge: bad argument (n %d, B %d, no %d)", n, B, no);
    MergeArgs a = {};
    a.n = n;
    a.no = no;
    a.B = B;
    a.img_h = (float)img_h;
    a.img_w = (float)img_w;
    int64_t total = 0;
    for (int p = 0; p < n; ++p) {
        if (!src[p] || a_begin[p] < 0 || a_end[p] <= a_begin[p] || a_end[p] > A[p] || !(scale[p] > 0.f) ||
            (flip[p] != 0 && flip[p] != 2 && flip[p] != 3))
            BSY_FAIL(BSY_ERR_ARG, "tta_merge: pass %d: window [%d, %d) of %d anchors, scale %g, flip %d", p, a_begin[p], a_end[p], A[p],
                     (double)scale[p], flip[p]);
        a.src[p] = src[p];
        a.A[p] = A[p];
        a.a0[p] = a_begin[p];
        a.cum[p] = (int)total;
        a.inv[p] = 1.0f / scale[p];
        a.flip[p] = flip[p];
        total += a_end[p] - a_begin[p];
    }
    if (total >= (1LL << 31)) BSY_FAIL(BSY_ERR_ARG, "tta_merge: %lld anchors", (long long)total);
    a.cum[n] = (int)total;
    if ((int64_t)B * no >= INT32_MAX) BSY_FAIL(BSY_ERR_ARG, "tta_merge: %d x %d rows", B, no);
    const int rows = B * no;
    const int grid = rows < kMaxBlocks ? rows : kMaxBlocks;
    if (dtype == BSY_F16)
        hipLaunchKernelGGL(tta_merge_kernel<half_t>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, a, (half_t*)out);
    else if (dtype == BSY_F32)
        hipLaunchKernelGGL(tta_merge_kernel<float>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, a, (float*)out);
    else
        BSY_FAIL(BSY_ERR_ARG, "tta_merge: dtype %d unsupported", dtype);
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
