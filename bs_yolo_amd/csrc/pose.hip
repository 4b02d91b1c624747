// Pose models on the device: the head's keypoint decode and the predictor's per-image scaling.  (The validator's OKS matching lives
// beside its siblings in val_match.hip, which owns the shared second half of the matching rule.)
//   nn/modules/head.py:273-279          Pose.kpts_decode, the non-export branch           -> kpts_decode_kernel, one launch
//   models/yolo/pose/predict.py:50-52   scale_boxes(...).round() + scale_coords per image  -> pose_scale_kernel, one launch, in place
// Compiled with -ffp-contract=off: both must round like the fp32 / fp16 torch ops they replace.
#include "common.h"
#include "postproc.h"
#include "kpt_decode.h"

constexpr int KPT_MAX = 64;     // keypoints per instance the entry points take
constexpr int KD_THREADS = 256; // anchors per workgroup of the decode
constexpr int KD_GROUP = 4;     // keypoints (= KD_GROUP * ndim channels) per workgroup of the decode

struct KptDecodeK {
    const void* in;
    void* out;
    long long out_bstride;  // elements between two images of `out`
    int h[BSY_MAX_LEVELS], w[BSY_MAX_LEVELS], a0[BSY_MAX_LEVELS];  // a0 = first anchor index of the level
    float stride[BSY_MAX_LEVELS];
    int nl, nkpt, ndim, A;
};

// The per-element arithmetic (kpt_xy / kpt_vis, both overloads) is kpt_decode.h, which detect.hip's keypoint mode shares.

// Thread = anchor, workgroup = KD_THREADS consecutive anchors of one (image, group of KD_GROUP keypoints): every load and store is
// coalesced along A.  HBM-bound: nk * sizeof(T) read and written per anchor; no LDS, no transposes.
template <typename T>
__global__ __launch_bounds__(KD_THREADS) void kpts_decode_kernel(const KptDecodeK p) {
    const int a = blockIdx.x * KD_THREADS + threadIdx.x;
    if (a >= p.A) return;
    const int b = blockIdx.z;
    int l = 0;
#pragma unroll
    for (int i = 1; i < BSY_MAX_LEVELS; ++i)
        if (i < p.nl && a >= p.a0[i]) l = i;
    const int la = a - p.a0[l];
    const float ax = (float)(la % p.w[l]), ay = (float)(la / p.w[l]);  // the anchor is (ax + 0.5, ay + 0.5)
    const float st = p.stride[l];
    const int nk = p.nkpt * p.ndim;
    const T* in = static_cast<const T*>(p.in) + (size_t)b * nk * p.A + a;
    T* out = static_cast<T*>(p.out) + (size_t)b * p.out_bstride + a;
    const int k0 = blockIdx.y * KD_GROUP, k1 = min(k0 + KD_GROUP, p.nkpt);
    for (int k = k0; k < k1; ++k) {
        const size_t c = (size_t)k * p.ndim * p.A;
        out[c] = kpt_xy(in[c], ax, st);
        out[c + p.A] = kpt_xy(in[c + p.A], ay, st);
        if (p.ndim == 3) out[c + 2 * (size_t)p.A] = kpt_vis(in[c + 2 * (size_t)p.A]);
    }
}

extern "C" int bsy_kpts_decode(const void* kpt, int dtype, int B, int nkpt, int ndim, int A, const int* lvl_h, const int* lvl_w,
                               const float* lvl_stride, int nl, void* out, long long out_bstride, bsy_stream stream) {
    if (!kpt || !out || !lvl_h || !lvl_w || !lvl_stride) BSY_FAIL(BSY_ERR_ARG, "kpts_decode: null pointer");
    if (B <= 0 || B > 65535 || nkpt < 1 || nkpt > KPT_MAX || (ndim != 2 && ndim != 3) || nl < 1 || nl > BSY_MAX_LEVELS || A <= 0)
        BSY_FAIL(BSY_ERR_ARG, "kpts_decode: bad sizes (B <= 65535, nkpt in 1..64, ndim 2 or 3, nl in 1..%d)", BSY_MAX_LEVELS);
    if (dtype != BSY_F16 && dtype != BSY_F32) BSY_FAIL(BSY_ERR_ARG, "kpts_decode: dtype must be f16 or f32");
    KptDecodeK k = {};
    long long a = 0;
    for (int l = 0; l < nl; ++l) {
        if (lvl_h[l] <= 0 || lvl_w[l] <= 0 || (long long)lvl_h[l] * lvl_w[l] > 0x7fffffffLL - a)
            BSY_FAIL(BSY_ERR_ARG, "kpts_decode: bad sizes (level %d is %d x %d)", l, lvl_h[l], lvl_w[l]);
        k.h[l] = lvl_h[l]; k.w[l] = lvl_w[l]; k.stride[l] = lvl_stride[l]; k.a0[l] = (int)a;
        a += (long long)lvl_h[l] * lvl_w[l];
    }
    if (a != A) BSY_FAIL(BSY_ERR_ARG, "kpts_decode: bad sizes (the levels hold %lld anchors, A is %d)", a, A);
    if (out_bstride < (long long)nkpt * ndim * A)
        BSY_FAIL(BSY_ERR_ARG, "kpts_decode: bad sizes (batch stride %lld of out < nk * A = %lld)", out_bstride, (long long)nkpt * ndim * A);
    k.in = kpt; k.out = out; k.out_bstride = out_bstride; k.nl = nl; k.nkpt = nkpt; k.ndim = ndim; k.A = A;
    const dim3 grid((A + KD_THREADS - 1) / KD_THREADS, (nkpt + KD_GROUP - 1) / KD_GROUP, B);
    dispatch_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(kpts_decode_kernel<decltype(t)>, grid, dim3(KD_THREADS), 0, (hipStream_t)stream, k);
    });
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

// ---- PosePredictor.postprocess's per-image tail ----------------------------------------------------------------------------------
struct PoseScaleK {
    float* det;
    const int32_t* counts;
    const float* params;  // (7, B): gain, box pad x, box pad y, keypoint pad x, keypoint pad y, h0, w0
    int B, max_det, row, nkpt, ndim;
    int round_boxes, normalize, padding;
};

// Thread = one item of one row: item 0 is the box (columns 0..3), item 1 + k keypoint k (columns 6 + k * ndim ..).  Every operation
// is the reference's, in its order: subtract the pad, divide by the gain (an IEEE division), clamp, then round (boxes) or
// normalise (keypoints).  The visibility column and columns 4, 5 are not touched; rows past counts[b] are not touched.
__global__ __launch_bounds__(256) void pose_scale_kernel(const PoseScaleK p) {
    const int items = 1 + p.nkpt;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const int i = t / items, j = t - i * items;
    if (i >= p.max_det || i >= p.counts[b]) return;
    float* o = p.det + ((size_t)b * p.max_det + i) * p.row;
    const float g = p.params[b], hh = p.params[5 * p.B + b], ww = p.params[6 * p.B + b];
    if (j == 0) {  // scale_boxes (ops.py:110-127) + clip_boxes (:331-334) + .round()
        const float px = p.params[p.B + b], py = p.params[2 * p.B + b];
        float x1 = o[0], y1 = o[1], x2 = o[2], y2 = o[3];
        if (p.padding) { x1 -= px; y1 -= py; x2 -= px; y2 -= py; }
        x1 = fminf(fmaxf(x1 / g, 0.f), ww);
        y1 = fminf(fmaxf(y1 / g, 0.f), hh);
        x2 = fminf(fmaxf(x2 / g, 0.f), ww);
        y2 = fminf(fmaxf(y2 / g, 0.f), hh);
        if (p.round_boxes) { x1 = rintf(x1); y1 = rintf(y1); x2 = rintf(x2); y2 = rintf(y2); }  // torch.round: half to even
        o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
    } else {       // scale_coords (ops.py:756-772) + clip_coords (:353-354)
        float* q = o + 6 + (j - 1) * p.ndim;
        float x = q[0], y = q[1];
        if (p.padding) { x -= p.params[3 * p.B + b]; y -= p.params[4 * p.B + b]; }
        x = fminf(fmaxf(x / g, 0.f), ww);
        y = fminf(fmaxf(y / g, 0.f), hh);
        if (p.normalize) { x /= ww; y /= hh; }
        q[0] = x; q[1] = y;
    }
}

extern "C" int bsy_pose_scale(float* det, const int32_t* counts, int B, int max_det, int row, int nkpt, int ndim, const float* params,
                              int round_boxes, int normalize, int padding, bsy_stream stream) {
    if (!det || !counts || !params) BSY_FAIL(BSY_ERR_ARG, "pose_scale: null pointer");
    if (B <= 0 || B > 65535 || max_det <= 0 || max_det > (1 << 20) || nkpt < 1 || nkpt > KPT_MAX || (ndim != 2 && ndim != 3) ||
        row < 6 + nkpt * ndim)
        BSY_FAIL(BSY_ERR_ARG, "pose_scale: bad sizes (B <= 65535, max_det <= 2^20, nkpt in 1..64, ndim 2 or 3, row >= 6 + nkpt * ndim)");
    PoseScaleK k;
    k.det = det; k.counts = counts; k.params = params; k.B = B; k.max_det = max_det; k.row = row; k.nkpt = nkpt; k.ndim = ndim;
    k.round_boxes = round_boxes; k.normalize = normalize; k.padding = padding;
    const dim3 grid((unsigned)(((long long)max_det * (1 + nkpt) + 255) / 256), B);
    hipLaunchKernelGGL(pose_scale_kernel, grid, dim3(256), 0, (hipStream_t)stream, k);
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
