// Batched non_max_suppression for gfx950, no host synchronisation.  Compile with -ffp-contract=off: the IoU test must
// round exactly like the fp32 CPU reference (inter / (area_i + area_j - inter) > thr, no FMA contraction).
//
// Replaces utils/ops.py:167-316 (non_max_suppression), :416-433 (xywh2xyxy) and the greedy suppression the reference
// delegates to torchvision.ops.nms (:296).  Three kernels per call, whole batch each (the shared pieces are postproc.h's):
//   1. nms_filter_kernel  (thread = anchor): xywh->xyxy in the prediction dtype (optionally written back, as the
//      reference mutates its input :243-244); confidence filter -- best class (:273-275) or multi-label expansion
//      (:270-272) --; optional class filter (:278-279); survivors are appended as 64-bit keys
//      (fp32 score bits << 32 | ~candidate_index): ONE descending sort gives "score descending, ties by ascending
//      candidate index", which is the order torchvision's sort + the reference's max_nms argsort produce.
//   2. key_sort_kernel    (block = image): bitonic sort of the keys (LDS up to 8192 keys, else in global memory).  The
//      library's ONE sort of 64-bit keys: launch_key_sort also serves sahi.hip.
//   3. nms_greedy_kernel  (block = image): walks the sorted candidates 256 at a time.  Each candidate is first
//      tested against the boxes already kept (LDS), then the survivors of the chunk are resolved among themselves
//      by greedy_resolve_256 -- identical to the sequential greedy order, without 256 serial steps.  Stops at max_det
//      kept (:297 `i[:max_det]`).
// Steps 1-2 are nms_candidates, which obb.hip's rotated NMS starts from as well; nms_check_args is shared with it too.
// The class offset `boxes + cls * max_wh` (:289-295) is applied in fp32 exactly as on the CPU.  Input fp16 is
// upcast to fp32 (the fp16 reference path overflows 7680*cls; we follow the fp32 CPU reference instead).
#include "postproc.h"

struct NmsK {
    void* pred;
    int B, nc, nm, A, C;  // C = 4+nc+nm
    float conf, iou;
    const int32_t* classes;
    int n_classes, agnostic, multi_label, max_det, max_nms;
    float max_wh;
    int in_place;
    int cap;  // keys per image
    u64* keys;
    int32_t* cand_count;
    float* out;
    int32_t* counts;
};

template <typename T>
__device__ __forceinline__ void load_xyxy(const T* pb, int A, int a, bool is_xyxy, float* o) {
    const float v0 = (float)pb[a], v1 = (float)pb[(size_t)A + a], v2 = (float)pb[(size_t)2 * A + a],
                v3 = (float)pb[(size_t)3 * A + a];
    if (is_xyxy) {
        o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3;
    } else {  // xywh2xyxy in the tensor's own precision (ops.py:428-432)
        const float hw = (float)(T)(v2 / 2.0f), hh = (float)(T)(v3 / 2.0f);
        o[0] = (float)(T)(v0 - hw); o[1] = (float)(T)(v1 - hh); o[2] = (float)(T)(v0 + hw); o[3] = (float)(T)(v1 + hh);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void nms_filter_kernel(const NmsK p) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (a >= p.A) return;
    T* pb = reinterpret_cast<T*>(p.pred) + (size_t)b * p.C * p.A;
    if (p.in_place) {
        float bx[4];
        load_xyxy<T>(pb, p.A, a, false, bx);
        pb[a] = (T)bx[0]; pb[(size_t)p.A + a] = (T)bx[1]; pb[(size_t)2 * p.A + a] = (T)bx[2]; pb[(size_t)3 * p.A + a] = (T)bx[3];
    }
    const T* cp = pb + (size_t)4 * p.A + a;
    u64* keys = p.keys + (size_t)b * p.cap;
    if (p.multi_label) {
        for (int c = 0; c < p.nc; ++c) {
            const float s = (float)cp[(size_t)c * p.A];
            if (!(s > p.conf)) continue;
            bool ok = p.n_classes == 0;
            for (int k = 0; k < p.n_classes; ++k) ok |= (p.classes[k] == c);
            if (!ok) continue;
            const int pos = atomicAdd(p.cand_count + b, 1);
            const unsigned idx = (unsigned)a * (unsigned)p.nc + (unsigned)c;
            keys[pos] = score_key(s, idx);
        }
    } else {
        float best;
        const int bc = first_max_class(cp, p.A, p.nc, best);
        if (!(best > p.conf)) return;
        bool ok = p.n_classes == 0;
        for (int k = 0; k < p.n_classes; ++k) ok |= (p.classes[k] == bc);
        if (!ok) return;
        const int pos = atomicAdd(p.cand_count + b, 1);
        keys[pos] = score_key(best, (unsigned)a);
    }
}

// Best-class filter, 4 anchors per thread (fp16 predictions, A % 4 == 0): every class row is
// read as 8-byte pieces instead of 2-byte ones -- the one-anchor form issues 80 two-byte loads per lane and ran at 1.4 TB/s.
// Same keys as nms_filter_kernel (their order in the list differs, the sort that follows removes that).
__global__ __launch_bounds__(256) void nms_filter4_kernel(const NmsK p) {
    const int a0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int b = blockIdx.y;
    if (a0 >= p.A) return;
    half_t* pb = reinterpret_cast<half_t*>(p.pred) + (size_t)b * p.C * p.A + a0;
    if (p.in_place) {  // xywh -> xyxy in the tensor's own precision, written back (ops.py:243-244, :428-432)
        const half4 x = *reinterpret_cast<const half4*>(pb), y = *reinterpret_cast<const half4*>(pb + (size_t)p.A),
                    w = *reinterpret_cast<const half4*>(pb + (size_t)2 * p.A), h = *reinterpret_cast<const half4*>(pb + (size_t)3 * p.A);
        half4 o0, o1, o2, o3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float hw = (float)(half_t)((float)w[j] / 2.0f), hh = (float)(half_t)((float)h[j] / 2.0f);
            o0[j] = (half_t)((float)x[j] - hw); o1[j] = (half_t)((float)y[j] - hh);
            o2[j] = (half_t)((float)x[j] + hw); o3[j] = (half_t)((float)y[j] + hh);
        }
        *reinterpret_cast<half4*>(pb) = o0; *reinterpret_cast<half4*>(pb + (size_t)p.A) = o1;
        *reinterpret_cast<half4*>(pb + (size_t)2 * p.A) = o2; *reinterpret_cast<half4*>(pb + (size_t)3 * p.A) = o3;
    }
    const half_t* cp = pb + (size_t)4 * p.A;
    half4 best = *reinterpret_cast<const half4*>(cp);
    int bc[4] = {0, 0, 0, 0};
    for (int c = 1; c < p.nc; ++c) {
        const half4 v = *reinterpret_cast<const half4*>(cp + (size_t)c * p.A);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((float)v[j] > (float)best[j]) { best[j] = v[j]; bc[j] = c; }
    }
    u64* keys = p.keys + (size_t)b * p.cap;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float s = (float)best[j];
        if (!(s > p.conf)) continue;
        bool ok = p.n_classes == 0;
        for (int k = 0; k < p.n_classes; ++k) ok |= (p.classes[k] == bc[j]);
        if (!ok) continue;
        const int pos = atomicAdd(p.cand_count + b, 1);
        keys[pos] = score_key(s, (unsigned)(a0 + j));
    }
}

// Segment b = keys[b * stride ..), counts[b] keys, sorted descending in place (launch_key_sort, postproc.h).
__global__ __launch_bounds__(1024) void key_sort_kernel(u64* keys_all, int stride, const int32_t* counts) {
    __shared__ u64 sk[SORT_LDS_KEYS];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int n = counts[b];
    if (n <= 1) return;
    const int np2 = pow2_at_least(n);
    u64* keys = keys_all + (size_t)b * stride;
    if (np2 <= SORT_LDS_KEYS) {
        for (int i = tid; i < np2; i += nt) sk[i] = i < n ? keys[i] : 0ull;
        __syncthreads();
        block_bitonic_desc(sk, np2);
        for (int i = tid; i < n; i += nt) keys[i] = sk[i];
    } else {
        for (int i = n + tid; i < np2; i += nt) keys[i] = 0ull;  // stride is a power of two >= np2
        __syncthreads();
        block_bitonic_desc(keys, np2);
    }
}

__device__ __forceinline__ bool iou_gt(const float* bi, float ai, const float* bj, float aj, float thr) {
    const float xx1 = fmaxf(bi[0], bj[0]), yy1 = fmaxf(bi[1], bj[1]);
    const float xx2 = fminf(bi[2], bj[2]), yy2 = fminf(bi[3], bj[3]);
    const float w = fmaxf(0.0f, xx2 - xx1), h = fmaxf(0.0f, yy2 - yy1);
    const float inter = w * h;
    const float ovr = inter / (ai + aj - inter);
    return ovr > thr;
}

template <typename T>
__global__ __launch_bounds__(256) void nms_greedy_kernel(const NmsK p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // layout: 64-bit words first, then ints, then floats (the host sizes it in bsy_nms)
    u64* keepw = reinterpret_cast<u64*>(smem_raw);       // [4]  keepw / supw / alw / sh_i[0]: greedy_resolve_256's
    u64* supw = keepw + 4;                               // [4]
    u64* alw = supw + 4;                                 // [4]
    int* sh_i = reinterpret_cast<int*>(alw + 4);         // [4]: [0] = undecided count, [1] = n_kept
    float* cbox = reinterpret_cast<float*>(sh_i + 4);    // [256][4]
    float* carea = cbox + 256 * 4;                       // [256]
    float* kbox = carea + 256;                           // [max_det][4]  kept boxes (offset by class)
    float* karea = kbox + (size_t)p.max_det * 4;         // [max_det]

    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const T* pb = reinterpret_cast<const T*>(p.pred) + (size_t)b * p.C * p.A;
    const u64* keys = p.keys + (size_t)b * p.cap;
    int n = p.cand_count[b];
    if (n > p.max_nms) n = p.max_nms;
    const int row = 6 + p.nm;
    float* ob = p.out + (size_t)b * p.max_det * row;
    const GreedyLds sh = {keepw, supw, alw, sh_i};
    if (tid == 0) sh_i[1] = 0;
    __syncthreads();

    for (int c0 = 0; c0 < n; c0 += 256) {
        const int n_kept = sh_i[1];
        if (n_kept >= p.max_det) break;
        const int i = c0 + tid;
        const bool have = i < n;
        float bx[4] = {0.f, 0.f, 0.f, 0.f}, obx[4] = {0.f, 0.f, 0.f, 0.f};
        float score = 0.f, area = 0.f;
        int cls = 0, anchor = 0;
        if (have) {
            decode_score_key(keys[i], p.nc, p.multi_label, pb, p.A, score, anchor, cls);
            load_xyxy<T>(pb, p.A, anchor, p.in_place != 0, bx);
            const float off = (float)cls * (p.agnostic ? 0.0f : p.max_wh);
#pragma unroll
            for (int e = 0; e < 4; ++e) obx[e] = bx[e] + off;
            area = (obx[2] - obx[0]) * (obx[3] - obx[1]);
        }
        // phase A: against everything kept so far
        bool alive = have;
        for (int j = 0; j < n_kept && alive; ++j)
            if (iou_gt(kbox + 4 * j, karea[j], obx, area, p.iou)) alive = false;
        // stage the chunk
#pragma unroll
        for (int e = 0; e < 4; ++e) cbox[4 * tid + e] = obx[e];
        carea[tid] = area;
        // the chunk's survivors among themselves
        u64 mrow[4], kw[4];
        const int state = greedy_resolve_256(alive, [&](int j) { return iou_gt(cbox + 4 * j, carea[j], obx, area, p.iou); }, sh, mrow, kw);
        // append kept candidates in order
        const int slot = n_kept + kept_rank<4>(kw, wave, kw[wave], lane);
        if (state == 1 && slot < p.max_det) {
#pragma unroll
            for (int e = 0; e < 4; ++e) kbox[4 * slot + e] = obx[e];
            karea[slot] = area;
            float* o = ob + (size_t)slot * row;
            o[0] = bx[0]; o[1] = bx[1]; o[2] = bx[2]; o[3] = bx[3];
            o[4] = score;
            o[5] = (float)cls;
            for (int k = 0; k < p.nm; ++k) o[6 + k] = (float)pb[(size_t)(4 + p.nc + k) * p.A + anchor];
        }
        __syncthreads();
        if (tid == 0) {
            const int tot = n_kept + __popcll(kw[0]) + __popcll(kw[1]) + __popcll(kw[2]) + __popcll(kw[3]);
            sh_i[1] = tot < p.max_det ? tot : p.max_det;
        }
        __syncthreads();
    }
    if (tid == 0) p.counts[b] = sh_i[1];
}

int launch_key_sort(u64* keys, int stride, const int32_t* counts, int segments, hipStream_t s) {
    hipLaunchKernelGGL(key_sort_kernel, dim3(segments), dim3(1024), 0, s, keys, stride, counts);
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

// The one place that chooses a filter kernel: the 4-anchor form needs f16, best-class keys, A % 4 == 0 and 8-byte rows.
int nms_candidates(void* pred, int pred_dtype, int B, int nc, int C, int A, float conf_thres, const int32_t* classes, int n_classes,
                   int multi_label, int in_place, int cap, u64* keys, int32_t* cand_count, hipStream_t s) {
    NmsK k = {};
    k.pred = pred; k.B = B; k.nc = nc; k.nm = C - 4 - nc; k.A = A; k.C = C;
    k.conf = conf_thres; k.classes = classes; k.n_classes = classes ? n_classes : 0; k.multi_label = multi_label;
    k.in_place = in_place; k.cap = cap; k.keys = keys; k.cand_count = cand_count;
    HIP_TRY(hipMemsetAsync(cand_count, 0, (size_t)B * 4, s));
    if (pred_dtype == BSY_F16 && !multi_label && !(A & 3) && !((uintptr_t)pred & 7))
        hipLaunchKernelGGL(nms_filter4_kernel, dim3((A / 4 + 255) / 256, B), dim3(256), 0, s, k);
    else
        dispatch_dtype(pred_dtype, [&](auto t) {
            hipLaunchKernelGGL(nms_filter_kernel<decltype(t)>, dim3((A + 255) / 256, B), dim3(256), 0, s, k);
        });
    return launch_key_sort(keys, cap, cand_count, B, s);
}

int nms_check_args(const char* op, const char* extra, const void* pred, const void* out, const void* counts, const void* workspace,
                   int pred_dtype, int B, int nc, int n_extra, int A, float conf_thres, float iou_thres, int max_det, int max_nms) {
    if (!pred || !out || !counts || !workspace) BSY_FAIL(BSY_ERR_ARG, "%s: null pointer", op);
    if (B <= 0 || nc <= 0 || n_extra < 0 || A <= 0)
        BSY_FAIL(BSY_ERR_ARG, "%s: bad sizes B=%d nc=%d %s=%d A=%d", op, B, nc, extra, n_extra, A);
    if (!(conf_thres >= 0.f && conf_thres <= 1.f))  // the two texts of the reference's asserts (ops.py:218-219)
        BSY_FAIL(BSY_ERR_ARG, "Invalid Confidence threshold %g, valid values are between 0.0 and 1.0", conf_thres);
    if (!(iou_thres >= 0.f && iou_thres <= 1.f))
        BSY_FAIL(BSY_ERR_ARG, "Invalid IoU %g, valid values are between 0.0 and 1.0", iou_thres);
    if (max_det <= 0 || max_det > NMS_MAX_DET) BSY_FAIL(BSY_ERR_ARG, "%s: max_det %d out of range (1..%d)", op, max_det, NMS_MAX_DET);
    if (max_nms <= 0) BSY_FAIL(BSY_ERR_ARG, "%s: max_nms must be positive", op);
    if (pred_dtype != BSY_F16 && pred_dtype != BSY_F32) BSY_FAIL(BSY_ERR_ARG, "%s: dtype %d unsupported", op, pred_dtype);
    if ((long long)A * nc > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "%s: A*nc too large", op);
    return BSY_OK;
}

// Workspace: per-image candidate counts, then `cap` keys per image.  With a null workspace only the returned size means anything.
static size_t nms_carve(void* workspace, int B, size_t cap, NmsK& k) {
    Carver c(workspace);
    c.align();
    k.cand_count = c.take<int32_t>(B);
    c.align();
    k.keys = c.take<u64>((size_t)B * cap);
    return c.need;
}

// nms_greedy_kernel's LDS: 112 + (1280 + 5 * max_det) * 4 bytes, 87 152 at the ABI's max_det = 4096
static size_t nms_greedy_lds(int max_det) { return 12 * 8 + 4 * 4 + ((size_t)256 * 5 + (size_t)max_det * 5) * 4; }

extern "C" size_t bsy_nms_workspace_bytes(int B, int A, int nc, int multi_label, int max_nms) {
    (void)max_nms;
    if (B <= 0 || A <= 0 || nc <= 0) return 0;
    NmsK measured;
    return nms_carve(nullptr, B, (size_t)pow2_at_least((multi_label && nc > 1) ? (long long)A * nc : (long long)A), measured);
}

extern "C" int bsy_nms(void* pred, int pred_dtype, int B, int nc, int nm, int A, float conf_thres, float iou_thres,
                       const int32_t* classes, int n_classes, int agnostic, int multi_label, int max_det, int max_nms,
                       float max_wh, int in_place, float* out, int32_t* counts, void* workspace, size_t workspace_bytes,
                       bsy_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    const int bad = nms_check_args("nms", "nm", pred, out, counts, workspace, pred_dtype, B, nc, nm, A, conf_thres, iou_thres, max_det, max_nms);
    if (bad != BSY_OK) return bad;
    multi_label = (multi_label && nc > 1) ? 1 : 0;  // ops.py:239
    const size_t need = bsy_nms_workspace_bytes(B, A, nc, multi_label, max_nms);
    if (workspace_bytes < need) BSY_FAIL(BSY_ERR_ARG, "nms: workspace %zu < %zu bytes", workspace_bytes, need);
    NmsK k;
    k.pred = pred; k.B = B; k.nc = nc; k.nm = nm; k.A = A; k.C = 4 + nc + nm;
    k.conf = conf_thres; k.iou = iou_thres; k.classes = classes; k.n_classes = classes ? n_classes : 0;
    k.agnostic = agnostic; k.multi_label = multi_label; k.max_det = max_det; k.max_nms = max_nms; k.max_wh = max_wh;
    k.in_place = in_place;
    k.cap = (int)pow2_at_least(multi_label ? (long long)A * nc : (long long)A);
    nms_carve(workspace, B, (size_t)k.cap, k);
    k.out = out; k.counts = counts;
    // Above 64 KiB of LDS a launch needs the function attribute (gfx950 has 160 KiB per CU); it is set once per process, for the
    // bound's size.
    static bool attr_set = false;
    if (!attr_set) {
        const int lds_max = (int)nms_greedy_lds(NMS_MAX_DET);
        HIP_TRY(hipFuncSetAttribute((const void*)nms_greedy_kernel<half_t>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        HIP_TRY(hipFuncSetAttribute((const void*)nms_greedy_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        attr_set = true;
    }
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)B * max_det * (6 + nm) * sizeof(float), s));
    const int rc = nms_candidates(pred, pred_dtype, B, nc, k.C, A, conf_thres, classes, k.n_classes, multi_label, in_place, k.cap, k.keys,
                                  k.cand_count, s);
    if (rc != BSY_OK) return rc;
    dispatch_dtype(pred_dtype, [&](auto t) {
        hipLaunchKernelGGL(nms_greedy_kernel<decltype(t)>, dim3(B), dim3(256), nms_greedy_lds(max_det), s, k);
    });
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

__global__ void scale_boxes_kernel(float* det, const int32_t* counts, int B, int max_det, int row, const float* gain,
                                   const float* pad_x, const float* pad_y, const float* h0, const float* w0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= max_det || i >= counts[b]) return;
    float* o = det + ((size_t)b * max_det + i) * row;
    const float g = gain[b], px = pad_x[b], py = pad_y[b], hh = h0[b], ww = w0[b];
    // ops.py:116-127: subtract pad, divide by gain, clip to the original image
    float x1 = (o[0] - px) / g, y1 = (o[1] - py) / g, x2 = (o[2] - px) / g, y2 = (o[3] - py) / g;
    o[0] = fminf(fmaxf(x1, 0.f), ww);
    o[1] = fminf(fmaxf(y1, 0.f), hh);
    o[2] = fminf(fmaxf(x2, 0.f), ww);
    o[3] = fminf(fmaxf(y2, 0.f), hh);
}

extern "C" int bsy_scale_boxes(float* det, const int32_t* counts, int B, int max_det, int row, const float* gain,
                               const float* pad_x, const float* pad_y, const float* h0, const float* w0,
                               bsy_stream stream) {
    if (!det || !counts || !gain || !pad_x || !pad_y || !h0 || !w0 || B <= 0 || max_det <= 0 || row < 4)
        BSY_FAIL(BSY_ERR_ARG, "scale_boxes: bad argument");
    dim3 grid((max_det + 127) / 128, B);
    hipLaunchKernelGGL(scale_boxes_kernel, grid, dim3(128), 0, (hipStream_t)stream, det, counts, B, max_det, row, gain,
                       pad_x, pad_y, h0, w0);
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
