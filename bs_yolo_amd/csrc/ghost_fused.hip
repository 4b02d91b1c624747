// GhostConv with a 1x1 stride-1 cv1 as ONE launch (conv.py:280-293; BSY_OP_GHOST):
//     y = act(cv1 x)   Conv 1x1, Cin -> CH              z = act(cv2 y)   depthwise 5x5 on CH channels          dst = [y | z] (+ res)
// A ghost graph is a long chain of very small launches (YOLOv8s-ghost: 30 GhostBottlenecks of two GhostConvs each); unfused, every
// GhostConv is a 1x1 conv, a depthwise 5x5 that re-reads the half-width map the conv just wrote, and -- in the second GhostConv of
// a bottleneck -- an add that re-reads both halves.  Here x is read once and dst written once:
//   * S1  a workgroup owns an 8 x 16 output tile and computes y on the 12 x 20 patch the depthwise conv reads (240 pixels = eight
//         32-pixel MFMA column blocks, the last half empty; two blocks per wave).  A B fragment (lane = patch pixel, lane half = 8
//         consecutive channels) is one 16-byte buffer load straight from the NHWC source: pixels outside the map, the tail past the
//         patch and channels past Cin come back as zeros from the descriptor, so x needs no LDS.  One accumulator per 32 output
//         channels, K walked once.  The activated patch goes to LDS as f16, ZERO outside the map (cv2's padding applies to y).
//   * S2  the depthwise 5x5 from that patch, item = (tile row, 4 consecutive pixels, 8-channel chunk), and the copy of the patch's
//         interior: both halves of dst, each with the shortcut operand added where there is one.
// cv1's weights stay in LDS for the whole launch where they fit beside the patch (WLDS), else the A fragments come from global
// memory (the wide, small maps at the end of a backbone: few tiles, the weights stay in L2); cv2's weights and bias are always in LDS.
//
// Arithmetic = the launches this replaces, step for step, so the same bits: cv1 as the conv kernels run a 1x1 layer (conv_select.hip
// conv_korder 0: accumulators start at the bias, v_mfma_f32_32x32x16_f16 over k = 16 ks + 8 lh in ascending order; SiLU in f32, one
// rounding to f16); cv2 as bsyolo_ops.hip dwconv_tile_kernel (accumulator starts at the bias, taps in (dy, dx) order, one f32 FMA on
// the f16 input per tap); the shortcut as add_kernel / conv_kernels.h conv_epilogue_lds (the f16 value + res in f32, rounded again).
#include "fused_tile.h"

namespace {
constexpr int GH_TH = 8, GH_TW = 16, GH_K = 5;
constexpr int GH_PH = GH_TH + GH_K - 1, GH_PW = GH_TW + GH_K - 1, GH_NPX = GH_PH * GH_PW;  // 12 x 20 = 240 patch pixels
constexpr int GH_NBLK = (GH_NPX + 31) / 32;                                                  // 8 MFMA pixel blocks
constexpr int GH_MAX_CIN = 512, GH_MAX_CH = 192;
constexpr size_t GH_WLDS_BYTES = 120 * 1024;  // cv1's weights go to LDS while the workgroup then still needs no more than this (measured:
                                              // the 128 -> 128 GhostConv at 20 x 20, 111 KiB, runs from LDS; docs/experiments.md)
constexpr size_t GH_MAX_SMEM = 128 * 1024;

struct GhostK {
    const half_t* src;
    int lds, H, W, Cin, CH, kpad, act;
    const half_t* w1;
    const float *b1, *w2, *b2;
    half_t* dst;
    int ldd;
    const half_t* res;
    int ldr;
    unsigned span;  // bytes of the source view (buffer descriptor)
    TileGrid grid;
};

// LDS layout: [y patch 240 x (CH + 8) f16][cv2 weights 25 x CH + bias CH, f32][cv1 weights NCB * 32 x (kpad + 8) f16, WLDS only]
__host__ __device__ inline size_t gh_patch_bytes(int CH) { return (size_t)GH_NPX * (CH + 8) * 2; }
__host__ __device__ inline size_t gh_dw_bytes(int CH) { return (size_t)(GH_K * GH_K + 1) * CH * 4; }
inline size_t gh_w1_bytes(int CH, int kpad) { return (size_t)ceil_div(CH, 32) * 32 * (kpad + 8) * 2; }

template <int NCB, bool WLDS>
__global__ __launch_bounds__(256) void ghost_fused_kernel(const GhostK p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ghost_smem[];
    const int CH = p.CH, PS = CH + 8;  // PS: halves per patch pixel, one 16-byte piece of padding (dwconv_tile_kernel's pitch)
    half_t* sp = reinterpret_cast<half_t*>(ghost_smem);
    float* sdw = reinterpret_cast<float*>(ghost_smem + gh_patch_bytes(CH));
    half_t* sw = reinterpret_cast<half_t*>(ghost_smem + gh_patch_bytes(CH) + gh_dw_bytes(CH));
    const int WP = p.kpad + 8;  // kpad is a multiple of 32: a pitch of 16 x odd bytes (fused_tile.h stage_rows)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 31, lh = lane >> 5;
    const int nch = CH >> 3, nks = (p.Cin + 15) >> 4;

    for (int i = tid; i < (GH_K * GH_K + 1) * CH; i += 256) sdw[i] = i < GH_K * GH_K * CH ? p.w2[i] : p.b2[i - GH_K * GH_K * CH];
    if (WLDS) stage_rows<256>(sw, p.w1, p.kpad, tid, NCB * 32, p.kpad >> 3, WP);
    const bsy_rsrc_t rs = make_rsrc(p.src, p.span);
    const half_t* abase = WLDS ? sw + lrow * WP + 8 * lh : p.w1 + (size_t)lrow * p.kpad + 8 * lh;  // A fragment of cout block 0, K-step 0
    const int astep = 32 * (WLDS ? WP : p.kpad);                                                  // to the next cout block
    __syncthreads();  // weights visible

    const TileWalk tw = xcd_tile_walk(blockIdx.x, gridDim.x, p.grid.ntiles);
    for (int tile = tw.tile; tile < tw.end; tile += tw.step) {
        const TileOrigin o = tile_origin<GH_TH, GH_TW>(p.grid, tile);
        if (o.oy0 >= p.H || o.ox0 >= p.W) continue;  // a padding tile of make_tile_grid (uniform: the whole workgroup skips it)
        // ---- S1: y = act(cv1 x) on the patch -> LDS --------------------------------------------------------------------------
        for (int pb = wave; pb < GH_NBLK; pb += 4) {
            const int e = 32 * pb + lrow, r = e / GH_PW, c = e - r * GH_PW;  // this lane's patch pixel
            const int y = o.oy0 - 2 + r, x = o.ox0 - 2 + c;
            const bool in = e < GH_NPX && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
            const unsigned base = 2u * ((unsigned)((o.n * p.H + y) * p.W + x) * (unsigned)p.lds + 8u * lh);
            // K-step ks of this lane: channels 16 ks + 8 lh .. + 7; zeros outside the map and past Cin
            auto bfrag = [&](int ks) { return buf_load16<half8>(rs, (in && 16 * ks + 8 * lh < p.Cin) ? base + 32u * ks : BSY_OOB); };
            f32x16 acc[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc_bias(acc[cb], p.b1 + 32 * cb, lh);  // accumulators start at the bias (common.h)
            half8 bf = bfrag(0);
            for (int ks = 0; ks < nks; ++ks) {
                const half8 nb = bfrag(ks + 1 < nks ? ks + 1 : ks);  // the next step's fragment is in flight during this step's MFMAs
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb)
                    acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8*>(abase + cb * astep + 16 * ks), bf, acc[cb], 0, 0, 0);
                bf = nb;
            }
            const unsigned keep = in ? 0xffffffffu : 0u;  // outside the map: cv2's zero padding
            if (e < GH_NPX) {
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (32 * cb + 8 * g < CH)
                            *reinterpret_cast<half4*>(sp + e * PS + 32 * cb + 8 * g + 4 * lh) = act_f16(acc_group(acc[cb], g), p.act, keep);
            }
        }
        lds_barrier();  // y patch complete
        // ---- S2a: z = act(cv2 y), depthwise 5x5 from the patch (dwconv_tile_kernel's arithmetic) -> dst[CH : 2 CH] ----------------
        for (int it = tid; it < GH_TH * (GH_TW / 4) * nch; it += 256) {
            const int ch = it % nch, q = it / nch, gx = q % (GH_TW / 4), gy = q / (GH_TW / 4);
            float acc[4][8];
            {
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(sdw + GH_K * GH_K * CH + ch * 8), b1 = *reinterpret_cast<const f32x4*>(sdw + GH_K * GH_K * CH + ch * 8 + 4);
#pragma unroll
                for (int px = 0; px < 4; ++px)
#pragma unroll
                    for (int j = 0; j < 4; ++j) { acc[px][j] = b0[j]; acc[px][4 + j] = b1[j]; }
            }
#pragma unroll 1
            for (int dy = 0; dy < GH_K; ++dy) {
                const half_t* row = sp + ((gy + dy) * GH_PW + 4 * gx) * PS + ch * 8;
                half8 win[4 + GH_K - 1];
#pragma unroll
                for (int w = 0; w < 4 + GH_K - 1; ++w) win[w] = *reinterpret_cast<const half8*>(row + w * PS);
#pragma unroll
                for (int dx = 0; dx < GH_K; ++dx) {
                    const float* wp = sdw + (dy * GH_K + dx) * CH + ch * 8;
                    const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp), w1 = *reinterpret_cast<const f32x4*>(wp + 4);
#pragma unroll
                    for (int px = 0; px < 4; ++px) fma_mix8(acc[px], win[px + dx], w0, w1);
                }
            }
            const int oy = o.oy0 + gy;
            if (oy >= p.H) continue;
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                const int ox = o.ox0 + 4 * gx + px;
                if (ox >= p.W) break;
                const size_t pix = (size_t)(o.n * p.H + oy) * p.W + ox;
                const f32x4 t0 = {acc[px][0], acc[px][1], acc[px][2], acc[px][3]}, t1 = {acc[px][4], acc[px][5], acc[px][6], acc[px][7]};
                union { half8 v; half4 h[2]; } ov;
                if (p.res) {
                    union { half8 v; half4 h[2]; } rv;
                    rv.v = *reinterpret_cast<const half8*>(p.res + pix * p.ldr + CH + ch * 8);
                    ov.h[0] = act_res_f16(rv.h[0], t0, p.act);
                    ov.h[1] = act_res_f16(rv.h[1], t1, p.act);
                } else {
                    ov.h[0] = act_f16(t0, p.act);
                    ov.h[1] = act_f16(t1, p.act);
                }
                *reinterpret_cast<half8*>(p.dst + pix * p.ldd + CH + ch * 8) = ov.v;
            }
        }
        // ---- S2b: the patch's interior is y -> dst[0 : CH]; the values are f16 already, so the shortcut add is add_kernel's -------
        for (int i = tid; i < GH_TH * GH_TW * nch; i += 256) {
            const int ch = i % nch, px = i / nch, py = px / GH_TW, pxx = px % GH_TW;
            const int oy = o.oy0 + py, ox = o.ox0 + pxx;
            if (oy >= p.H || ox >= p.W) continue;
            const size_t pix = (size_t)(o.n * p.H + oy) * p.W + ox;
            half8 v = *reinterpret_cast<const half8*>(sp + ((py + 2) * GH_PW + pxx + 2) * PS + ch * 8);
            if (p.res) {
                const half8 rv = *reinterpret_cast<const half8*>(p.res + pix * p.ldr + ch * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (half_t)((float)v[j] + (float)rv[j]);
            }
            *reinterpret_cast<half8*>(p.dst + pix * p.ldd + ch * 8) = v;
        }
        lds_barrier();  // the patch is free for the next tile
    }
}

template <int NCB, bool WLDS>
int launch_cfg(const GhostK& k, int grid, size_t smem, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void*)ghost_fused_kernel<NCB, WLDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GH_MAX_SMEM));
        attr_set = true;
    }
    hipLaunchKernelGGL((ghost_fused_kernel<NCB, WLDS>), dim3(grid), dim3(256), smem, s, k);
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
template <int NCB>
int launch_ncb(const GhostK& k, bool wlds, int grid, size_t smem, hipStream_t s) {
    return wlds ? launch_cfg<NCB, true>(k, grid, smem, s) : launch_cfg<NCB, false>(k, grid, smem, s);
}
}  // namespace

// Every width in 8-channel pieces up to the limits: the stock ghost graphs of scales n .. x need Cin <= 320 and CH <= 160 after padding
bool ghost_fused_supported(int Cin, int CH) {
    return Cin >= 8 && CH >= 8 && !(Cin & 7) && !(CH & 7) && Cin <= GH_MAX_CIN && CH <= GH_MAX_CH;
}

int launch_ghost_fused(const GhostArgs& a, hipStream_t s) {
    if (!ghost_fused_supported(a.Cin, a.CH)) BSY_FAIL(BSY_ERR_ARG, "ghost_fused: widths %d -> %d not supported (multiples of 8 up to %d / %d)", a.Cin, a.CH, GH_MAX_CIN, GH_MAX_CH);
    if (!a.src || !a.dst || !a.w1 || !a.b1 || !a.w2 || !a.b2 || a.B <= 0 || a.H <= 0 || a.W <= 0) BSY_FAIL(BSY_ERR_ARG, "ghost_fused: null pointer or empty map");
    if ((a.lds & 7) || (a.ldd & 7) || (a.res && (a.ldr & 7)) || !all_aligned16(a.src, a.dst, a.res, a.w1, a.b1, a.w2, a.b2))
        BSY_FAIL(BSY_ERR_ARG, "ghost_fused: strides must be multiples of 8 and pointers 16-byte aligned");
    if (a.lds < a.Cin || a.ldd < 2 * a.CH || (a.res && a.ldr < 2 * a.CH)) BSY_FAIL(BSY_ERR_ARG, "ghost_fused: a view is wider than its buffer's rows");
    const long long npix = (long long)a.B * a.H * a.W;
    const long long widest = a.lds > a.ldd ? (a.lds > a.ldr ? a.lds : a.ldr) : (a.ldd > a.ldr ? a.ldd : a.ldr);
    if (npix * widest >= (1LL << 31)) BSY_FAIL(BSY_ERR_ARG, "ghost_fused: a view exceeds 2^31 elements (split the batch)");
    GhostK k;
    k.src = a.src; k.lds = a.lds; k.H = a.H; k.W = a.W; k.Cin = a.Cin; k.CH = a.CH; k.act = a.act;
    k.w1 = a.w1; k.b1 = a.b1; k.w2 = a.w2; k.b2 = a.b2; k.dst = a.dst; k.ldd = a.ldd; k.res = a.res; k.ldr = a.ldr;
    int cp = 0;
    if (int rc = bsy_conv_packed_dims(a.CH, a.Cin, 1, &cp, &k.kpad)) return rc;
    k.span = (unsigned)(((npix - 1) * a.lds + a.Cin) * 2);
    if (int rc = make_tile_grid(k.grid, a.B, a.H, a.W, GH_TH, GH_TW, "ghost_fused")) return rc;
    size_t smem = gh_patch_bytes(a.CH) + gh_dw_bytes(a.CH);
    const bool wlds = smem + gh_w1_bytes(a.CH, k.kpad) <= GH_WLDS_BYTES;
    if (wlds) smem += gh_w1_bytes(a.CH, k.kpad);
    if (smem > GH_MAX_SMEM) BSY_FAIL(BSY_ERR_ARG, "ghost_fused: %zu bytes of LDS", smem);
    // workgroups resident per CU: LDS first (160 KiB), four waves each; at most four (one per SIMD and 128 registers)
    const int per_cu = (int)(160 * 1024 / smem) < 4 ? ((int)(160 * 1024 / smem) > 1 ? (int)(160 * 1024 / smem) : 1) : 4;
    const int grid = persistent_grid(k.grid.ntiles, 256 * per_cu);
    switch (ceil_div(a.CH, 32)) {
        case 1: return launch_ncb<1>(k, wlds, grid, smem, s);
        case 2: return launch_ncb<2>(k, wlds, grid, smem, s);
        case 3: return launch_ncb<3>(k, wlds, grid, smem, s);
        case 4: return launch_ncb<4>(k, wlds, grid, smem, s);
        case 5: return launch_ncb<5>(k, wlds, grid, smem, s);
        default: return launch_ncb<6>(k, wlds, grid, smem, s);
    }
}
