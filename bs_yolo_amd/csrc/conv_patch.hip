// The patch-based 3x3 stride-1 conv kernel and its box-branch tail (3x3 conv + 1x1 conv + DFL decoder in one launch).
// conv_select.hip decides where it runs (conv_cfg_valid, conv_candidates).
#include "conv_kernels.h"

// ---------------------------------------------------------------------------------------------------------------------
// Patch-based 3x3 stride-1 kernel (configuration tiles 10 / 11).
//
// The implicit-GEMM kernel (conv_gemm.hip) stages every input pixel NINE times (once per tap) through the vector-memory path and
// LDS; at 128 x 128 tiles that is 64 B/clk/CU of LDS-DMA -- the texture-addresser's peak -- plus the matching LDS
// writes, and measured MFMA utilisation stalls near 25-30 %.  A 3x3 stride-1 conv only needs each input pixel once
// per workgroup: here a workgroup owns an 8 x 16 output tile, keeps the 10 x 18 input patch of the current 32-channel
// chunk in LDS and reads all nine taps' B fragments from it (a tap is a constant entry offset); only the weights
// (3 taps x TN x 32 per (chunk, kernel row) step) stream through the DMA ring.  Vector-memory bytes per MFMA drop ~2.5x.
//   * K order: chunk-major, taps inside (the packed weights stay k = (kh, kw, c): tap (kh, kw) of a chunk reads K offset
//     (3 kh + kw) * Cin + 32 * chunk).  That differs from the implicit-GEMM kernel's tap-major order, so results agree with it
//     to fp32 accumulation rounding, not bit for bit.
//   * patch: 192 entries (180 used) x 64 B, filled by LDS-DMA 16 entries per wave-instruction; slot s of entry q holds
//     channel chunk s ^ ((q >> 2) & 3) (the DMA lane picks its source chunk), so 16 consecutive entries read
//     conflict-free.  Double-buffered: chunk c + 1 is fetched at tap 0 of chunk c.
//   * counted vmcnt: a wave has WIW weight DMAs per step in flight for STAGES - 1 steps, plus PIW patch DMAs issued at
//     kernel row 0 of every chunk.
// Restrictions (conv_cfg_valid): 3x3, stride 1, one source, no upsample, Cin % 32 == 0, fp16 output.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int CP_TW = 16;  // default tile width (pixels)
// A K-step is one (32-channel chunk, kernel row): 3 taps x 32 channels = 6 MFMA sub-steps per wave tile.  (One tap per
// step left 4-8 MFMAs between barriers and a two-step prefetch distance far below the L2 latency.)
// WM = wave rows: 2 -> 8 x 16 output tile, 4 waves (the shipped form).  4 -> 16 x 16 tile, 8 waves: measured 8-25 % SLOWER
// on every YOLO11s layer (r01 notes in DESIGN.md) and therefore not instantiated.
// TW_ = tile width: 16 (8 x 16 tile: 128 pixels = the 128 pixel slots of the four MFMA pixel tiles) or 20 (6 x 20 tile: 120
// pixels in the 128 slots, slot i = pixel (i / 20, i % 20)) -- a 20 x 20 map is 4 tiles of 6 x 20 instead of 6 tiles of
// 8 x 16 (48 % of whose slots lie outside the map), a 40 x 40 map 14 instead of 15.
// TAIL (NT == 1, four waves): the Detect box branch's last two layers in one launch -- this 3x3 conv (64 couts), then the
// branch's 1x1 conv (64 -> 64 box logits) on the activated fp16 tile straight from LDS and the DFL decoder on its accumulators
// (ConvArgs::tail_wgt).  Wave w takes pixel slots 32 w .. 32 w + 31 and all 64 couts (the decoder's layout: a side's 16 bins in
// one lane pair).  Same operands, same K order as the separate 1x1 launch -> the same bits; the 64-channel map stays on chip.
#define BSY_K(n) n
#define BSY_RELU false
#include "conv_patch_kernel.h"
#undef BSY_K
#undef BSY_RELU
#define BSY_K(n) n##_relu
#define BSY_RELU true
#include "conv_patch_kernel.h"
#undef BSY_K
#undef BSY_RELU

template <int NT, int STAGES, int WM, int TW_ = CP_TW, bool TAIL = false>
static int launch_patch(const ConvK& k, hipStream_t s) {
    ConvK p = k;
    p.ntn = ceil_div(k.Cout, 64 * NT);
    p.tiles_x = ceil_div(k.W, TW_);
    p.tiles_y = ceil_div(k.H, TW_ == 16 ? 4 * WM : 6);
    const long long nblk = (long long)k.B * p.tiles_x * p.tiles_y * p.ntn;
    if (nblk <= 0 || nblk > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "conv: tile count %lld out of range", nblk);
    { if (p.act == 2) hipLaunchKernelGGL((conv3x3_patch_kernel_relu<NT, STAGES, WM, TW_, TAIL>), dim3((unsigned)nblk), dim3(128 * WM), 0, s, p); else hipLaunchKernelGGL((conv3x3_patch_kernel<NT, STAGES, WM, TW_, TAIL>), dim3((unsigned)nblk), dim3(128 * WM), 0, s, p); }
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

// One case per patch row of kConvCfgs (conv_select.hip): the row's <NT, STAGES, TW> with the shipped four-wave form (WM = 2); the
// 64-cout ids have a second instantiation with the box-branch tail.
int launch_patch_cfg(int id, bool tail, const ConvK& k, hipStream_t s) {
    if (tail) {
        switch (id) {
            case 0xB1: return launch_patch<1, 3, 2, 16, true>(k, s);
            case 0xB2: return launch_patch<1, 2, 2, 16, true>(k, s);
            case 0xB3: return launch_patch<1, 4, 2, 16, true>(k, s);
            case 0xD1: return launch_patch<1, 3, 2, 20, true>(k, s);
            case 0xD2: return launch_patch<1, 2, 2, 20, true>(k, s);
            case 0xD3: return launch_patch<1, 4, 2, 20, true>(k, s);
        }
    } else {
        switch (id) {
            case 0xA1: return launch_patch<2, 2, 2, 16>(k, s);
            case 0xB1: return launch_patch<1, 3, 2, 16>(k, s);
            case 0xB2: return launch_patch<1, 2, 2, 16>(k, s);
            case 0xB3: return launch_patch<1, 4, 2, 16>(k, s);
            case 0xC1: return launch_patch<2, 2, 2, 20>(k, s);
            case 0xD1: return launch_patch<1, 3, 2, 20>(k, s);
            case 0xD2: return launch_patch<1, 2, 2, 20>(k, s);
            case 0xD3: return launch_patch<1, 4, 2, 20>(k, s);
        }
    }
    BSY_FAIL(BSY_ERR_ARG, "conv: no patch kernel%s is built for configuration 0x%02x", tail ? " with a box-branch tail" : "", id);
}
