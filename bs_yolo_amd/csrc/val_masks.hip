// Mask IoU of the segment validator on the device, as bit planes, and the matching on it.  Replaces, per batch,
//   models/yolo/segment/val.py:204-217   SegmentationValidator._process_batch(..., masks=True)
//   utils/metrics.py:220-236             mask_iou: a float matmul over H W pixels, two row sums, one division
// followed by BaseValidator.match_predictions (the rule of val_match.hip, run here on the IoU matrix by val_match_from_iou).
//
// Masks on both sides are 0 / 1, so the matmul entry is the number of common pixels and the row sums are pixel counts: integers
// below 2^24 for masks up to 4096 x 4096, exact in fp32 in any summation order.  Only
//   inter / ((area_gt + area_pred) - inter + 1e-7f)
// rounds, twice (the eps addition and the division), and is computed here with the same fp32 operations (-ffp-contract=off), so
// the matrix equals the reference's bit for bit.
//
//   pack_masks_kernel      (n, H W) f32 / f16 / u8 -> (n, ceil(H W / 64)) 64-bit planes, bit (p & 63) of word (p >> 6) = pixel p is
//                          non-zero, tail bits zero; one wave64 __ballot per word, a wave keeps 64 of them (lane i the i-th) and
//                          stores them as one coalesced row; the area is the popcount, added per wave with one integer atomic.
//   pack_label_map_kernel  the overlap_mask=True form (segment/val.py:205-209): one (H W) index map, value l + 1 marks label l ->
//                          the nl planes in one pass over the map (a wave keeps its 64 x 64 pixels in registers).
//   mask_iou_kernel        workgroup = 16 detections x 8 labels of one image.  The labels' planes are staged through LDS 512 words
//                          at a time; each wave owns 4 detections and walks the words, a lane takes two of them per step -- one
//                          16-byte global load per detection, one 16-byte LDS load per label -- and adds popcount(gt & pred) into
//                          its 32 integer counters; 6 xor-shuffles per counter fold the lanes at the end.  Per step a lane issues
//                          4 global + 8 LDS loads for 256 VALU operations, so the kernel is bound by v_and / v_bcnt.  Rows of an
//                          odd word count are only 8-byte aligned and take 8-byte loads.
#include "common.h"

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <typename T>
__global__ __launch_bounds__(256) void pack_masks_kernel(const T* masks, int hw, int words, u64* planes, int32_t* areas) {
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w0 = (blockIdx.y * 4 + wave) * 64;  // this wave's first word
    if (w0 >= words) return;                      // wave-uniform; the kernel has no barrier
    const T* m = masks + (size_t)n * hw;
    const int ni = words - w0 < 64 ? words - w0 : 64;
    u64 mine = 0;
    for (int i0 = 0; i0 < ni; i0 += 8) {  // 8 independent loads in flight, then their ballots
        bool set[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int px = (w0 + i0 + k) * 64 + lane;  // a word past the last one lies past hw as well
            set[k] = px < hw && m[px] != (T)0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const u64 bal = __ballot(set[k]);
            if (lane == i0 + k) mine = bal;
        }
    }
    if (lane < ni) planes[(size_t)n * words + w0 + lane] = mine;
    const int cnt = wave_sum(__popcll(mine));
    if (lane == 0 && cnt) atomicAdd(&areas[n], cnt);
}

#define PLM_LABELS 8  // labels per workgroup of pack_label_map_kernel
template <typename T>
__global__ __launch_bounds__(256) void pack_label_map_kernel(const T* map, int hw, int words, int nl, u64* planes, int32_t* areas) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w0 = (blockIdx.x * 4 + wave) * 64;
    if (w0 >= words) return;
    const int ni = words - w0 < 64 ? words - w0 : 64;
    float v[64];  // pixel 64 (w0 + i) + lane; 0 marks no label
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int px = (w0 + i) * 64 + lane;
        v[i] = (i < ni && px < hw) ? (float)map[px] : 0.0f;
    }
    const int l0 = blockIdx.y * PLM_LABELS;
    for (int l = l0; l < nl && l < l0 + PLM_LABELS; ++l) {
        const float key = (float)(l + 1);
        u64 mine = 0;
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const u64 bal = __ballot(v[i] == key);
            if (lane == i) mine = bal;
        }
        if (lane < ni) planes[(size_t)l * words + w0 + lane] = mine;
        const int cnt = wave_sum(__popcll(mine));
        if (lane == 0 && cnt) atomicAdd(&areas[l], cnt);
    }
}

extern "C" int bsy_pack_masks(const void* masks, int dtype, int n, int hw, int label_map, uint64_t* planes, int32_t* areas,
                              bsy_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!masks || !planes || !areas) BSY_FAIL(BSY_ERR_ARG, "pack_masks: null pointer");
    if (n <= 0 || hw <= 0 || hw > (1 << 24) || (label_map && n > 65535 * PLM_LABELS))
        BSY_FAIL(BSY_ERR_ARG, "pack_masks: bad sizes n=%d hw=%d (hw <= 2^24)", n, hw);
    if (dtype != BSY_F16 && dtype != BSY_F32 && dtype != BSY_U8) BSY_FAIL(BSY_ERR_ARG, "pack_masks: dtype %d unsupported", dtype);
    if ((uintptr_t)planes & 7) BSY_FAIL(BSY_ERR_ARG, "pack_masks: planes must be 8-byte aligned");
    const int words = (hw + 63) / 64, wb = (words + 255) / 256;
    HIP_TRY(hipMemsetAsync(areas, 0, (size_t)n * sizeof(int32_t), s));
    u64* pl = (u64*)planes;
    if (label_map) {
        dim3 grid(wb, (n + PLM_LABELS - 1) / PLM_LABELS);
        if (dtype == BSY_F32) hipLaunchKernelGGL(pack_label_map_kernel<float>, grid, dim3(256), 0, s, (const float*)masks, hw, words, n, pl, areas);
        else if (dtype == BSY_F16) hipLaunchKernelGGL(pack_label_map_kernel<half_t>, grid, dim3(256), 0, s, (const half_t*)masks, hw, words, n, pl, areas);
        else hipLaunchKernelGGL(pack_label_map_kernel<uint8_t>, grid, dim3(256), 0, s, (const uint8_t*)masks, hw, words, n, pl, areas);
    } else {
        dim3 grid(n, wb);
        if (dtype == BSY_F32) hipLaunchKernelGGL(pack_masks_kernel<float>, grid, dim3(256), 0, s, (const float*)masks, hw, words, pl, areas);
        else if (dtype == BSY_F16) hipLaunchKernelGGL(pack_masks_kernel<half_t>, grid, dim3(256), 0, s, (const half_t*)masks, hw, words, pl, areas);
        else hipLaunchKernelGGL(pack_masks_kernel<uint8_t>, grid, dim3(256), 0, s, (const uint8_t*)masks, hw, words, pl, areas);
    }
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

#define MI_TL 8    // labels per workgroup
#define MI_TD 4    // detections per wave (4 waves: 16 per workgroup)
#define MI_CH 512  // words of each label staged per pass (32 KiB of LDS)

struct MaskIouK {
    const u64* pred;  // (B, max_det, words)
    const int32_t* pred_area;
    const u64* gt;    // (B, Lmax, words)
    const int32_t* gt_area;
    const int32_t* counts;
    const int32_t* gt_counts;
    float* iou;       // (B, Lmax, max_det), zeroed by the caller
    int max_det, Lmax, words;
    int vec;          // rows are 16-byte aligned (even word count, aligned bases)
};

// words w and w + 1 of a row (w even), zero past its end
__device__ __forceinline__ void load2(const u64* row, const int w, const int words, const int vec, u64& lo, u64& hi) {
    if (vec && w + 1 < words) {
        const u64x2 v = *reinterpret_cast<const u64x2*>(row + w);
        lo = v[0];
        hi = v[1];
    } else {
        lo = w < words ? row[w] : 0ull;
        hi = w + 1 < words ? row[w + 1] : 0ull;
    }
}

__global__ __launch_bounds__(256) void mask_iou_kernel(const MaskIouK p) {
    __shared__ __attribute__((aligned(16))) u64 sl[MI_TL][MI_CH];
    const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nd = min(p.counts[b], p.max_det), nl = min(p.gt_counts[b], p.Lmax);
    const int l0 = blockIdx.y * MI_TL, dbase = blockIdx.x * (4 * MI_TD);
    if (l0 >= nl || dbase >= nd) return;  // uniform over the workgroup
    const int ntl = nl - l0 < MI_TL ? nl - l0 : MI_TL;
    const int d0 = dbase + wave * MI_TD;
    const bool active = d0 < nd;          // uniform over the wave; an idle wave still stages and meets the barriers
    const u64* pp[MI_TD];
#pragma unroll
    for (int j = 0; j < MI_TD; ++j)       // a detection past the count re-reads the last one; its result is not written
        pp[j] = p.pred + ((size_t)b * p.max_det + (d0 + j < nd ? d0 + j : nd - 1)) * p.words;
    const u64* gl = p.gt + ((size_t)b * p.Lmax + l0) * p.words;
    int acc[MI_TD][MI_TL];
#pragma unroll
    for (int j = 0; j < MI_TD; ++j)
#pragma unroll
        for (int l = 0; l < MI_TL; ++l) acc[j][l] = 0;
    for (int c0 = 0; c0 < p.words; c0 += MI_CH) {
        __syncthreads();  // the previous chunk has been read by every wave
        for (int e = tid; e < MI_TL * (MI_CH / 2); e += 256) {
            const int l = e / (MI_CH / 2), w = 2 * (e % (MI_CH / 2));
            if (l < ntl && c0 + w < p.words) {  // rows >= ntl and words past the end are never read
                u64 lo, hi;
                load2(gl + (size_t)l * p.words, c0 + w, p.words, p.vec, lo, hi);
                *reinterpret_cast<u64x2*>(&sl[l][w]) = u64x2{lo, hi};
            }
        }
        __syncthreads();
        if (active) {
            const int cw = p.words - c0 < MI_CH ? p.words - c0 : MI_CH;
            for (int w = 2 * lane; w < cw; w += 128) {
                u64 dlo[MI_TD], dhi[MI_TD];
#pragma unroll
                for (int j = 0; j < MI_TD; ++j) load2(pp[j], c0 + w, p.words, p.vec, dlo[j], dhi[j]);
#pragma unroll
                for (int l = 0; l < MI_TL; ++l) {
                    if (l < ntl) {  // uniform
                        const u64x2 g = *reinterpret_cast<const u64x2*>(&sl[l][w]);
#pragma unroll
                        for (int j = 0; j < MI_TD; ++j) acc[j][l] += __popcll(g[0] & dlo[j]) + __popcll(g[1] & dhi[j]);
                    }
                }
            }
        }
    }
    if (!active) return;
    int mine = 0;  // lane 8 j + l keeps the count of (detection j, label l)
#pragma unroll
    for (int j = 0; j < MI_TD; ++j)
#pragma unroll
        for (int l = 0; l < MI_TL; ++l) {
            const int t = wave_sum(acc[j][l]);
            if (lane == j * MI_TL + l) mine = t;
        }
    const int j = lane / MI_TL, l = lane % MI_TL;
    if (lane < MI_TD * MI_TL && d0 + j < nd && l < ntl) {
        // mask_iou (metrics.py:234-236): every term is an exact integer in fp32 up to the eps addition
        const float inter = (float)mine;
        const float ag = (float)p.gt_area[(size_t)b * p.Lmax + l0 + l], ap = (float)p.pred_area[(size_t)b * p.max_det + d0 + j];
        p.iou[((size_t)b * p.Lmax + l0 + l) * p.max_det + d0 + j] = inter / (((ag + ap) - inter) + 1e-7f);
    }
}

extern "C" size_t bsy_val_match_masks_workspace_bytes(int B, int max_det, int Lmax) {
    if (B <= 0 || max_det <= 0 || Lmax <= 0) return 0;
    return (size_t)B * Lmax * max_det * sizeof(float);
}

extern "C" int bsy_val_match_masks(const float* det, int row, const int32_t* counts, int B, int max_det, const uint64_t* pred_planes,
                                   const int32_t* pred_areas, const uint64_t* gt_planes, const int32_t* gt_areas, int words,
                                   const float* gt_cls, const int32_t* gt_counts, int Lmax, const float* iouv_host, int n_iou,
                                   unsigned char* out, float* iou_out, void* workspace, size_t workspace_bytes, bsy_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!det || !counts || !pred_planes || !pred_areas || !gt_planes || !gt_areas || !gt_cls || !gt_counts || !iouv_host || !out)
        BSY_FAIL(BSY_ERR_ARG, "val_match_masks: null pointer");
    if (B <= 0 || B > 65535 || max_det <= 0 || max_det > 1024 || row < 6 || Lmax <= 0 || Lmax > 8192 || n_iou <= 0 || n_iou > 16 ||
        words <= 0 || words > (1 << 18))
        BSY_FAIL(BSY_ERR_ARG, "val_match_masks: bad sizes (B <= 65535, max_det <= 1024, Lmax <= 8192, n_iou <= 16, words <= 2^18)");
    if (((uintptr_t)pred_planes | (uintptr_t)gt_planes) & 7) BSY_FAIL(BSY_ERR_ARG, "val_match_masks: planes must be 8-byte aligned");
    const size_t need = bsy_val_match_masks_workspace_bytes(B, max_det, Lmax);
    float* iou = iou_out;
    if (!iou) {
        if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 3))
            BSY_FAIL(BSY_ERR_ARG, "val_match_masks: without iou_out the workspace must hold %zu bytes", need);
        iou = (float*)workspace;
    }
    MaskIouK k;
    k.pred = (const u64*)pred_planes; k.pred_area = pred_areas; k.gt = (const u64*)gt_planes; k.gt_area = gt_areas;
    k.counts = counts; k.gt_counts = gt_counts; k.iou = iou; k.max_det = max_det; k.Lmax = Lmax; k.words = words;
    k.vec = (words % 2 == 0 && !(((uintptr_t)pred_planes | (uintptr_t)gt_planes) & 15)) ? 1 : 0;
    HIP_TRY(hipMemsetAsync(iou, 0, need, s));
    dim3 grid((max_det + 4 * MI_TD - 1) / (4 * MI_TD), (Lmax + MI_TL - 1) / MI_TL, B);
    hipLaunchKernelGGL(mask_iou_kernel, grid, dim3(256), 0, s, k);
    HIP_TRY(hipGetLastError());
    return val_match_from_iou(iou, det, row, counts, B, max_det, gt_cls, gt_counts, Lmax, iouv_host, n_iou, out, s);
}
