// Implicit-GEMM convolution for gfx950 (MI355X): y = act(conv2d(x, W) + b) [+ residual], NHWC fp16 activations.
//
// Replaces Conv.forward_fuse (nn/modules/conv.py:149-151) for k in {1,3}, stride in {1,2}, groups=1, together with
// the tensor plumbing around it that the reference materialises in HBM:
//   * torch.cat (Concat conv.py:445-455; C2f/C3/SPPF/C2PSA cat) -> the K loop walks up to two source views,
//     producers write straight into channel slices of the consumer's buffer (dst ld/offset);
//   * nn.Upsample(nearest, x2) -> a source flagged `up` is read at (iy>>1, ix>>1);
//   * chunk/split -> a source view is a channel slice (pointer offset + row stride);
//   * Bottleneck / PSABlock shortcut add -> residual added after the activation in the epilogue.
//
// GEMM view: D[cout][pixel] = sum_k Wt[cout][k] * P[pixel][k], k = (kh, kw, cin) with cin fastest, so both MFMA
// operands are K-contiguous 16-byte fragments: NHWC gives P, the host packs Wt as [CoutPad][Kpad].
// MFMA: v_mfma_f32_32x32x16_f16, A operand = weights (rows = cout), B operand = pixels (cols = pixel).  The
// accumulator then holds, per lane, ONE pixel and groups of 4 consecutive output channels.
//
// Tile: 256 threads = 4 waves (WAVES_M x WAVES_N), wave tile (MT*32 pixels) x (NT*32 couts), BK = 32.
// LDS rows are 64 B (32 halves) with the 16-B chunk index XOR-swizzled by (row>>2)&3 so that ds_read_b128 of 16
// consecutive rows hits 16 distinct slots of the 256-B bank row (guide T2).
//
// Staging (v2): LDS-DMA (`global_load_lds_dwordx4`, 1 KiB per wave-instruction = 16 rows x 64 B, lane-linear LDS image;
// the swizzle is applied to the per-lane SOURCE chunk, guide rule 21) into a ring of STAGES K-steps.  A conv K-step is
// only 8 MFMAs per wave (~0.1-0.3 us) while a fetch takes 1-3 us under load, so the ring keeps STAGES-1 K-steps in
// flight behind a COUNTED `s_waitcnt vmcnt(N)` and one raw `s_barrier` per K-step (never `__syncthreads()`, which would
// drain the DMA queue).  Out-of-image taps / K padding read a zero page instead of branching.
// The epilogue pairs lanes l and l+32 with v_permlane32_swap so each lane stores 16 B (8 consecutive channels).
#include "conv_kernels.h"

// Ablations for profiling (tools/abl_1x1.py) exist at compile time only: -DBSY_ABLATE=<bits>, 1 = no DMA, 4 = no epilogue.  Results are
// WRONG under them; the shipped build defines nothing and contains neither branch (a run-time switch inside a K loop costs time).

__device__ __attribute__((aligned(16))) unsigned int bsy_zero_page[16];  // zero-initialised; source of padded taps

// BK = channels per K-step (32 or 64).  LDS rows hold BK halves (64 / 128 B); a 1-KiB DMA wave-instruction fills
// RPI = 512/BK rows.  BK = 64 needs Cin % 64 == 0: every staged row is then a full 128-B line of its source, which halves
// the L2 request count per byte (the LDS-DMA gather rate from L2 is request-bound: ~35 GB/s/CU with 64-B pieces).
// ALIGNED: Cin % BK == 0 and C0 % BK == 0, so every K-step lies inside ONE tap of ONE source: all of the K bookkeeping
// (tap, source, channel base, tap displacement) is wave-uniform scalar work and a DMA address is row_offset + scalar,
// issued through a buffer descriptor (out-of-range lanes -> zeros).  The generic variant (thin layers: Cin = 8 / 16 /
// 48 ..., BK = 32 only) keeps it per lane and uses flat LDS-DMA + a zero page.
#define BSY_K(n) n
#define BSY_RELU false
#include "conv_gemm_kernel.h"
#undef BSY_K
#undef BSY_RELU
#define BSY_K(n) n##_relu
#define BSY_RELU true
#include "conv_gemm_kernel.h"
#undef BSY_K
#undef BSY_RELU

#undef BSY_ADVANCE_K

// Split-K second step: out[pixel][c] = act(sum over slices, IN SLICE ORDER, of the raw f32 sums) (+ shortcut) -> f16 NHWC.  One thread
// per (pixel, 8 couts); the order of the adds is fixed by the slice index, so the result does not depend on which workgroup finished
// first, on the tile configuration or on the batch.

template <int KS, int WM, int WN, int MT, int NT, int STAGES, bool ALIGNED, int BK>
static int launch_cfg(const ConvK& k, hipStream_t s) {
    constexpr int TM = WM * MT * 32, TN = WN * NT * 32;
    ConvK p = k;
    p.ntn = ceil_div(k.Cout, TN);
    const int nsl = k.nsl_c * k.nsl_t;  // split-K: conv_cfg_valid admits only aligned rows whose BK divides the channel slices
    const long long nblk = (long long)ceil_div(k.M, TM) * p.ntn * (nsl > 1 ? nsl : 1);
    if (nblk <= 0 || nblk > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "conv: grid %lld out of range", nblk);
    { if (p.act == 2) hipLaunchKernelGGL((conv_mfma_kernel_relu<KS, WM, WN, MT, NT, STAGES, ALIGNED, BK>), dim3((unsigned)nblk), dim3(64 * WM * WN), 0, s, p); else hipLaunchKernelGGL((conv_mfma_kernel<KS, WM, WN, MT, NT, STAGES, ALIGNED, BK>), dim3((unsigned)nblk), dim3(64 * WM * WN), 0, s, p); }
    HIP_TRY(hipGetLastError());
    if (nsl > 1) {
        const long long items = (long long)k.M * (k.Cout >> 3);
        if (k.act == 2)
            hipLaunchKernelGGL(splitk_reduce_kernel_relu, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, k.split_ws, nsl, k.slab, k.ldw, k.M, k.Cout, k.act,
                           k.res, k.ldr, reinterpret_cast<half_t*>(k.dst), k.ldd);
        else
            hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, k.split_ws, nsl, k.slab, k.ldw, k.M, k.Cout, k.act,
                           k.res, k.ldr, reinterpret_cast<half_t*>(k.dst), k.ldd);
        HIP_TRY(hipGetLastError());
    }
    return BSY_OK;
}

// One case per implicit-GEMM row of kConvCfgs (conv_select.hip), the row's template arguments verbatim:
// <WAVES_M, WAVES_N, MT, NT, STAGES, ALIGNED, BK>.
template <int WM, int WN, int MT, int NT, int S, bool AL, int BK>
static int launch_gemm(int ksize, const ConvK& k, hipStream_t s) {
    return ksize == 3 ? launch_cfg<3, WM, WN, MT, NT, S, AL, BK>(k, s) : launch_cfg<1, WM, WN, MT, NT, S, AL, BK>(k, s);
}

int launch_gemm_cfg(int id, int ksize, const ConvK& k, hipStream_t s) {
    switch (id) {
        case 0x00: return launch_gemm<4, 1, 2, 1, 3, false, 32>(ksize, k, s);
        case 0x01: return launch_gemm<4, 1, 2, 1, 3, true, 32>(ksize, k, s);
        case 0x02: return launch_gemm<4, 1, 2, 1, 2, true, 32>(ksize, k, s);
        case 0x03: return launch_gemm<4, 1, 2, 1, 2, true, 64>(ksize, k, s);
        case 0x10: return launch_gemm<4, 1, 2, 2, 3, false, 32>(ksize, k, s);
        case 0x11: return launch_gemm<4, 1, 2, 2, 3, true, 32>(ksize, k, s);
        case 0x12: return launch_gemm<4, 1, 2, 2, 2, true, 32>(ksize, k, s);
        case 0x13: return launch_gemm<4, 1, 2, 2, 2, true, 64>(ksize, k, s);
        case 0x20: return launch_gemm<2, 2, 2, 2, 3, false, 32>(ksize, k, s);
        case 0x21: return launch_gemm<2, 2, 2, 2, 3, true, 32>(ksize, k, s);
        case 0x22: return launch_gemm<2, 2, 2, 2, 2, true, 32>(ksize, k, s);
        case 0x23: return launch_gemm<2, 2, 2, 2, 2, true, 64>(ksize, k, s);
        case 0x30: return launch_gemm<2, 2, 2, 1, 3, false, 32>(ksize, k, s);
        case 0x31: return launch_gemm<2, 2, 2, 1, 3, true, 32>(ksize, k, s);
        case 0x32: return launch_gemm<2, 2, 2, 1, 2, true, 32>(ksize, k, s);
        case 0x33: return launch_gemm<2, 2, 2, 1, 2, true, 64>(ksize, k, s);
        case 0x41: return launch_gemm<4, 2, 2, 2, 3, true, 32>(ksize, k, s);
        case 0x42: return launch_gemm<4, 2, 2, 2, 2, true, 32>(ksize, k, s);
        case 0x43: return launch_gemm<4, 2, 2, 2, 2, true, 64>(ksize, k, s);
        case 0x50: return launch_gemm<1, 4, 2, 1, 3, false, 32>(ksize, k, s);
        case 0x51: return launch_gemm<1, 4, 2, 1, 3, true, 32>(ksize, k, s);
        case 0x52: return launch_gemm<1, 4, 2, 1, 2, true, 32>(ksize, k, s);
        case 0x53: return launch_gemm<1, 4, 2, 1, 2, true, 64>(ksize, k, s);
        case 0x60: return launch_gemm<2, 2, 1, 1, 3, false, 32>(ksize, k, s);
        case 0x61: return launch_gemm<2, 2, 1, 1, 3, true, 32>(ksize, k, s);
        case 0x62: return launch_gemm<2, 2, 1, 1, 2, true, 32>(ksize, k, s);
        case 0x63: return launch_gemm<2, 2, 1, 1, 2, true, 64>(ksize, k, s);
        case 0x71: return launch_gemm<4, 2, 2, 4, 3, true, 32>(ksize, k, s);
        case 0x72: return launch_gemm<4, 2, 2, 4, 2, true, 32>(ksize, k, s);
        case 0x73: return launch_gemm<4, 2, 2, 4, 2, true, 64>(ksize, k, s);
    }
    BSY_FAIL(BSY_ERR_ARG, "conv: no implicit-GEMM kernel is built for configuration 0x%02x", id);
}
