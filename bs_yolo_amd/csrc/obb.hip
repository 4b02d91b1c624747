// Rotated NMS and the OBB postprocess tail for gfx950, no host synchronisation.  Compile with -ffp-contract=off: probiou must
// round like the fp32 CPU reference, one operation at a time (no FMA contraction).
//
// Replaces non_max_suppression(..., rotated=True) (utils/ops.py:241-297) with nms_rotated (:146-164) and batch_probiou
// (utils/metrics.py:261-278, :327-358), and the per-image tail of OBBPredictor.postprocess (models/yolo/obb/predict.py:48-49).
// bsy_nms_rotated, whole batch per launch:
//   1. nms_candidates (nms.hip, declared in postproc.h): bsy_nms's confidence / class filter and key sort, score descending, ties
//      by ascending index; the prediction stays xywhr (no xyxy conversion).  The argument checks are nms.hip's nms_check_args.
//   2. obb_gather_kernel   (thread = sorted candidate < max_nms): the class-offset centre and the covariance terms of
//      _get_covariance_matrix, computed once per candidate into the workspace.
//   3. obb_suppress_kernel (workgroup = 256 sorted candidates of one image): FAST-NMS -- candidate i is kept iff
//      probiou(j, i) < thr for EVERY earlier j, suppressed j included (ious.triu_(1).max(0) < thr).  No decision depends on
//      another decision, so every candidate is tested independently: earlier candidates are staged through LDS 256 at a time,
//      a lane stops once its candidate is suppressed and the workgroup once all of its lanes are.
//   4. obb_compact_kernel  (workgroup = image): order-preserving compaction of the kept flags (postproc.h block_kept_rank), cut
//      at max_det (exact: the decisions of the first max_det kept candidates do not depend on the ones after them).
#include "postproc.h"
#include "probiou.h"

struct ObbK {
    const void* pred;
    int B, nc, ne, A, C;  // C = 4 + nc + ne
    float iou;
    int agnostic, multi_label, max_det;
    int nmax;             // records per image: min(max_nms, candidates the filter can produce)
    float max_wh;
    int cap;              // keys per image
    u64* keys;
    int32_t* cand_count;
    float* cov;           // (B, nmax, 8): x + off, y + off, a, b, c, clamp(a b - c^2, 0), -, -
    float* rows;          // (B, nmax, 8): x, y, w, h, conf, cls, anchor (int bits), -
    int32_t* keep;        // (B, nmax)
    float* out;
    int32_t* counts;
};

__device__ __forceinline__ int obb_n(const ObbK& p, int b) {
    const int n = p.cand_count[b];
    return n < p.nmax ? n : p.nmax;
}

template <typename T>
__global__ __launch_bounds__(256) void obb_gather_kernel(const ObbK p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= obb_n(p, b)) return;
    const T* pb = reinterpret_cast<const T*>(p.pred) + (size_t)b * p.C * p.A;
    float score;
    int anchor, cls;
    decode_score_key(p.keys[(size_t)b * p.cap + i], p.nc, p.multi_label, pb, p.A, score, anchor, cls);
    const float x = (float)pb[anchor], y = (float)pb[(size_t)p.A + anchor];
    const float w = (float)pb[(size_t)2 * p.A + anchor], h = (float)pb[(size_t)3 * p.A + anchor];
    // theta = the last column of the candidate's row (ops.py:292 x[:, -1:]): the last extra row, the class index without one
    const float th = p.ne ? (float)pb[(size_t)(p.C - 1) * p.A + anchor] : (float)cls;
    const float off = (float)cls * (p.agnostic ? 0.0f : p.max_wh);
    const ObbCov g = obb_covariance(w, h, th);  // probiou.h
    float* cv = p.cov + ((size_t)b * p.nmax + i) * 8;
    float* rw = p.rows + ((size_t)b * p.nmax + i) * 8;
    *reinterpret_cast<f32x4*>(cv) = f32x4{x + off, y + off, g.a, g.b};
    *reinterpret_cast<f32x4*>(cv + 4) = f32x4{g.c, g.det, 0.0f, 0.0f};
    *reinterpret_cast<f32x4*>(rw) = f32x4{x, y, w, h};
    *reinterpret_cast<f32x4*>(rw + 4) = f32x4{score, (float)cls, __int_as_float(anchor), 0.0f};
}

// probiou(j, i) of probiou.h: batch_probiou (metrics.py:342-358) of obb1 = j and obb2 = i on (x, y, a, b, c, det) as gathered
#define OBB_TILE 256
__global__ __launch_bounds__(OBB_TILE) void obb_suppress_kernel(const ObbK p) {
    __shared__ f32x4 s0[OBB_TILE];  // x, y, a, b of the staged earlier candidates
    __shared__ float s1[OBB_TILE][2];  // c, det
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = obb_n(p, b);
    const int i0 = blockIdx.x * OBB_TILE;
    if (i0 >= n) return;  // uniform over the workgroup
    const int i = i0 + tid;
    const bool have = i < n;
    f32x4 me0 = {0.f, 0.f, 0.f, 0.f};
    float mc = 0.f, md = 0.f;
    if (have) {
        const float* cv = p.cov + ((size_t)b * p.nmax + i) * 8;
        me0 = *reinterpret_cast<const f32x4*>(cv);
        mc = cv[4]; md = cv[5];
    }
    // the column max over j < i includes the zeros of triu_(1): a candidate survives only if 0 < thr as well
    bool alive = have && (0.0f < p.iou);
    for (int t0 = 0; t0 <= i0; t0 += OBB_TILE) {  // tiles of earlier candidates, this workgroup's own chunk last
        __syncthreads();  // the previous tile has been read by every lane
        const int j = t0 + tid;
        if (j < n) {
            const float* cv = p.cov + ((size_t)b * p.nmax + j) * 8;
            s0[tid] = *reinterpret_cast<const f32x4*>(cv);
            s1[tid][0] = cv[4];
            s1[tid][1] = cv[5];
        }
        if (!__syncthreads_or(alive)) break;
        const int lim = i - t0 < OBB_TILE ? i - t0 : OBB_TILE;  // j < i (and j < n, as i < n)
        for (int jj = 0; alive && jj < lim; ++jj)
            if (!(probiou(s0[jj], s1[jj][0], s1[jj][1], me0, mc, md) < p.iou)) alive = false;
    }
    if (have) p.keep[(size_t)b * p.nmax + i] = alive ? 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(1024) void obb_compact_kernel(const ObbK p) {
    __shared__ int wsum[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = obb_n(p, b);
    const int row = 6 + p.ne;
    const T* pb = reinterpret_cast<const T*>(p.pred) + (size_t)b * p.C * p.A;
    float* ob = p.out + (size_t)b * p.max_det * row;
    int base = 0;  // kept so far (the same value in every lane)
    for (int c0 = 0; c0 < n && base < p.max_det; c0 += 1024) {
        const int i = c0 + tid;
        const bool k = i < n && p.keep[(size_t)b * p.nmax + i] != 0;
        int tot;
        const int slot = base + block_kept_rank<16>(k, wsum, tot);
        if (k && slot < p.max_det) {
            const float* r = p.rows + ((size_t)b * p.nmax + i) * 8;
            float* o = ob + (size_t)slot * row;
#pragma unroll
            for (int e = 0; e < 6; ++e) o[e] = r[e];
            const int anchor = __float_as_int(r[6]);
            for (int e = 0; e < p.ne; ++e) o[6 + e] = (float)pb[(size_t)(4 + p.nc + e) * p.A + anchor];
        }
        base += tot;
        __syncthreads();  // wsum is rewritten by the next chunk
    }
    if (tid == 0) p.counts[b] = base < p.max_det ? base : p.max_det;
}

// Workspace: bsy_nms's candidate counts and keys, then nmax records per image.  With a null workspace only the returned size
// means anything.
static size_t obb_carve(void* workspace, int B, size_t cap, size_t nmax, ObbK& k) {
    Carver c(workspace);
    c.align();
    k.cand_count = c.take<int32_t>(B, true);
    k.keys = c.take<u64>((size_t)B * cap, true);
    k.cov = c.take<float>((size_t)B * nmax * 8, true);
    k.rows = c.take<float>((size_t)B * nmax * 8, true);
    k.keep = c.take<int32_t>((size_t)B * nmax, true);
    return c.need;
}

extern "C" size_t bsy_nms_rotated_workspace_bytes(int B, int A, int nc, int multi_label, int max_nms) {
    if (B <= 0 || A <= 0 || nc <= 0 || max_nms <= 0) return 0;
    const long long per = (multi_label && nc > 1) ? (long long)A * nc : (long long)A;
    ObbK measured;
    return obb_carve(nullptr, B, (size_t)pow2_at_least(per), (size_t)(per < max_nms ? per : max_nms), measured);
}

extern "C" int bsy_nms_rotated(void* pred, int pred_dtype, int B, int nc, int ne, int A, float conf_thres, float iou_thres,
                               const int32_t* classes, int n_classes, int agnostic, int multi_label, int max_det, int max_nms,
                               float max_wh, float* out, int32_t* counts, void* workspace, size_t workspace_bytes,
                               bsy_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    const int bad = nms_check_args("nms_rotated", "ne", pred, out, counts, workspace, pred_dtype, B, nc, ne, A, conf_thres, iou_thres, max_det,
                                   max_nms);
    if (bad != BSY_OK) return bad;
    if ((long long)B * (4 + nc + ne) * A > 0x7fffffffffffLL) BSY_FAIL(BSY_ERR_ARG, "nms_rotated: A*nc too large");
    multi_label = (multi_label && nc > 1) ? 1 : 0;  // ops.py:239
    const size_t need = bsy_nms_rotated_workspace_bytes(B, A, nc, multi_label, max_nms);
    if (workspace_bytes < need) BSY_FAIL(BSY_ERR_ARG, "nms_rotated: workspace %zu < %zu bytes", workspace_bytes, need);
    const long long per = multi_label ? (long long)A * nc : (long long)A;
    ObbK k = {};
    k.pred = pred; k.B = B; k.nc = nc; k.ne = ne; k.A = A; k.C = 4 + nc + ne;
    k.iou = iou_thres; k.agnostic = agnostic; k.multi_label = multi_label; k.max_det = max_det;
    k.nmax = (int)(per < max_nms ? per : max_nms); k.max_wh = max_wh; k.cap = (int)pow2_at_least(per);
    obb_carve(workspace, B, (size_t)k.cap, (size_t)k.nmax, k);
    k.out = out; k.counts = counts;
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)B * max_det * (6 + ne) * sizeof(float), s));
    const int rc = nms_candidates(pred, pred_dtype, B, nc, k.C, A, conf_thres, classes, classes ? n_classes : 0, multi_label, 0, k.cap,
                                  k.keys, k.cand_count, s);
    if (rc != BSY_OK) return rc;
    const dim3 grid((k.nmax + OBB_TILE - 1) / OBB_TILE, B);
    dispatch_dtype(pred_dtype, [&](auto t) {
        hipLaunchKernelGGL(obb_gather_kernel<decltype(t)>, grid, dim3(OBB_TILE), 0, s, k);
        hipLaunchKernelGGL(obb_suppress_kernel, grid, dim3(OBB_TILE), 0, s, k);
        hipLaunchKernelGGL(obb_compact_kernel<decltype(t)>, dim3(B), dim3(1024), 0, s, k);
    });
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

__global__ void obb_scale_kernel(float* det, const int32_t* counts, int max_det, int row, const float* gain, const float* pad_x,
                                 const float* pad_y, const float* h0, const float* w0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= max_det || i >= counts[b]) return;
    float* o = det + ((size_t)b * max_det + i) * row;
    const float pi = 3.14159265358979323846f, half_pi = 1.57079632679489661923f;  // math.pi, math.pi / 2 as fp32 scalars
    const float x = o[0], y = o[1], w = o[2], h = o[3], t = o[row - 1];
    // regularize_rboxes (ops.py:785-790): swap w / h when h >= w; torch's remainder: fmod, then + pi where it is negative
    const bool wide = w > h;
    const float wr = wide ? w : h, hr = wide ? h : w;
    float r = fmodf(wide ? t : t + half_pi, pi);
    if (r != 0.0f && r < 0.0f) r += pi;
    // scale_boxes(xywh=True) (ops.py:120-127): pad off x and y only, all four divided by the gain; clip_boxes (:331-334)
    const float g = gain[b], ww = w0[b], hh = h0[b];
    const float xs = (x - pad_x[b]) / g, ys = (y - pad_y[b]) / g, ws = wr / g, hs = hr / g;
    o[0] = fminf(fmaxf(xs, 0.f), ww);
    o[1] = fminf(fmaxf(ys, 0.f), hh);
    o[2] = fminf(fmaxf(ws, 0.f), ww);
    o[3] = fminf(fmaxf(hs, 0.f), hh);
    o[row - 1] = r;
}

extern "C" int bsy_obb_scale(float* det, const int32_t* counts, int B, int max_det, int row, const float* gain, const float* pad_x,
                             const float* pad_y, const float* h0, const float* w0, bsy_stream stream) {
    if (!det || !counts || !gain || !pad_x || !pad_y || !h0 || !w0 || B <= 0 || max_det <= 0 || row < 7)
        BSY_FAIL(BSY_ERR_ARG, "obb_scale: bad argument");
    dim3 grid((max_det + 127) / 128, B);
    hipLaunchKernelGGL(obb_scale_kernel, grid, dim3(128), 0, (hipStream_t)stream, det, counts, max_det, row, gain, pad_x, pad_y, h0,
                       w0);
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
