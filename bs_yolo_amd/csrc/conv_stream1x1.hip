// The two streaming kernels for 1x1 stride-1 layers (fp16, aligned channels, no shortcut): persistent tiles with dedicated store
// waves, and the weights-resident form for the HBM-bound layers.  Same K order and epilogue arithmetic as the implicit-GEMM kernel
// (conv_gemm.hip): the same bits.  conv_select.hip decides where they run (conv_cfg_valid, conv_candidates).
#include "conv_kernels.h"

// ---------------------------------------------------------------------------------------------------------------------
// Persistent 1x1 kernel with dedicated store waves ("thin-K" layers: 2-24 K-steps per tile).
//
// With one tile per workgroup the load -> MFMA -> store phases of those layers only overlap across the 2-5 resident
// workgroups: removing the epilogue alone made them 2.4x faster, removing the DMA alone 2x.  Here a workgroup of 8 waves
// walks tiles (XCD-aware order, common.h xcd_tile_walk) with ONE continuous DMA ring:
//   waves 0-3 (compute): issue the LDS-DMA (running STAGES-1 K-steps ahead, ACROSS tile boundaries), MFMA, then park
//                        bias + SiLU results as an fp16 tile in LDS and carry straight on with the next tile;
//   waves 4-7 (store)  : walk the same barrier sequence, and after each tile's hand-over barrier move the parked tile to
//                        HBM with coalesced 16-byte stores.  Their stores sit in THEIR OWN vmcnt queues, so the compute
//                        waves' counted `s_waitcnt vmcnt(N)` keeps seeing nothing but DMA.
// Barrier protocol (every wave executes every s_barrier): per tile nk "K-step" barriers B(t,k) + one hand-over barrier
// E(t) after the compute waves' tile writes.  Store waves read tile t between E(t) and B(t+1,0); compute waves overwrite
// the parked tile only after B(t+1,nk-1) >= B(t+1,0): no second tile buffer needed.
// Restrictions (checked by conv_cfg_valid): ksize 1, ALIGNED channels, fp16 output, no residual, Cout % 8 == 0.
// ---------------------------------------------------------------------------------------------------------------------
#define BSY_K(n) n
#define BSY_RELU false
#include "conv_stream1x1_kernel.h"
#undef BSY_K
#undef BSY_RELU
#define BSY_K(n) n##_relu
#define BSY_RELU true
#include "conv_stream1x1_kernel.h"
#undef BSY_K
#undef BSY_RELU

template <int WM, int WN, int MT, int NT, int STAGES, int BK>
static int launch_persist(const ConvK& k, hipStream_t s) {
    constexpr int TM = WM * MT * 32, TN = WN * NT * 32;
    ConvK p = k;
    p.ntn = ceil_div(k.Cout, TN);
    p.ntm = ceil_div(k.M, TM);
    const long long ntiles = (long long)p.ntm * p.ntn;
    if (ntiles <= 0 || ntiles > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "conv: tile count %lld out of range", ntiles);
    constexpr int lds_bytes = ((TM + (TN < 64 ? 64 : TN)) * BK * STAGES + TM * (TN + 8) + 2 * PERSIST_MAX_COUT) * 2;
    const int per_cu = 160 * 1024 / lds_bytes > 2 ? 2 : (160 * 1024 / lds_bytes);  // 512-thread workgroups: <= 2 per CU
    const long long grid = ntiles < 256LL * per_cu ? ntiles : 256LL * per_cu;
    { if (p.act == 2) hipLaunchKernelGGL((conv1x1_persist_kernel_relu<WM, WN, MT, NT, STAGES, BK>), dim3((unsigned)grid), dim3(512), 0, s, p); else hipLaunchKernelGGL((conv1x1_persist_kernel<WM, WN, MT, NT, STAGES, BK>), dim3((unsigned)grid), dim3(512), 0, s, p); }
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Weights-resident streaming 1x1 kernel (configuration tiles 14 / 15; round 3) for the HBM-bound 1x1 layers at 160^2 / 80^2.
//
// What held those layers at 3.3-4.6 TB/s (a device copy runs at 5.4): every 128-pixel tile re-staged the layer's whole weight
// matrix from L2 into LDS (model.4.cv2: 49 KB of pixels + 98 KB of weights per tile pair = 14 B/clk/CU, the LDS-DMA rate of a CU),
// and load / MFMA / store phases of a tile only overlap across workgroups.  Here a persistent workgroup (4 waves, two per CU)
// works on ONE cout tile for the whole launch and keeps its weights -- every wave the A fragments of its 32 NT couts over all of K
// -- in REGISTERS; only pixels stream through LDS (one continuous DMA ring across tile boundaries, STAGES K-steps deep), so the
// L2 -> LDS traffic is the input itself.  Workgroups b and b + 8 (one XCD under round-robin dispatch) take the same pixel tiles and
// different cout tiles: the second reads the pixels from that XCD's L2.
// A tile's results leave through an LDS tile as 16-byte stores issued by the same waves; they sit in the vmcnt queue BEHIND the DMA
// of the next steps and are accounted for in the counted waits (a wait for K-step g sees the stores of the previous tile as younger
// operations during the first STAGES - 1 steps of a tile).
// Same K order and epilogue arithmetic as the other 1x1 kernels: the same bits.
// Restrictions (conv_cfg_valid): as the persistent kernel, and K / 16 x NT <= 32 fragments at NT = 1, 24 at NT = 2 (more spills).
// ---------------------------------------------------------------------------------------------------------------------
// NFR = A fragments held per wave (K / 16 x NT <= NFR): 32 = 128 VGPRs

template <int NT, int STAGES, int NFR>
static int launch_wres(const ConvK& k, hipStream_t s) {
    constexpr int TM = 128, TN = 64 * NT;
    ConvK p = k;
    p.ntn = ceil_div(k.Cout, TN);
    p.ntm = ceil_div(k.M, TM);
    // two workgroups per CU; a multiple of 8 ntn so that every XCD runs the same number of walkers for every cout tile
    int grid = 512 / (8 * p.ntn) * (8 * p.ntn);
    if (grid < 8 * p.ntn) grid = 8 * p.ntn;
    const int walkers_per_xcd = grid / 8 / p.ntn;
    if (walkers_per_xcd > ceil_div(p.ntm, 8)) grid = 8 * p.ntn * (ceil_div(p.ntm, 8) > 0 ? ceil_div(p.ntm, 8) : 1);
    { if (p.act == 2) hipLaunchKernelGGL((conv1x1_wres_kernel_relu<NT, STAGES, NFR>), dim3((unsigned)grid), dim3(256), 0, s, p); else hipLaunchKernelGGL((conv1x1_wres_kernel<NT, STAGES, NFR>), dim3((unsigned)grid), dim3(256), 0, s, p); }
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

template <int NT, int S, int NFR> static int launch_wres_nfr(const ConvK& k, hipStream_t s) {  // 16 fragments where they hold K
    return NT * ((k.C0 + k.C1) / 16) <= 16 ? launch_wres<NT, S, 16>(k, s) : launch_wres<NT, S, NFR>(k, s);
}

// One case per persistent / weights-resident row of kConvCfgs (conv_select.hip), the row's template arguments verbatim:
// persistent <WAVES_M, WAVES_N, MT, NT, STAGES, BK>, weights-resident <NT, STAGES, NFR>.
int launch_stream1x1_cfg(int id, const ConvK& k, hipStream_t s) {
    switch (id) {
        case 0x81: return launch_persist<2, 2, 2, 2, 3, 32>(k, s);
        case 0x82: return launch_persist<2, 2, 2, 2, 2, 32>(k, s);
        case 0x83: return launch_persist<2, 2, 2, 2, 2, 64>(k, s);
        case 0x91: return launch_persist<2, 2, 2, 1, 3, 32>(k, s);
        case 0x92: return launch_persist<2, 2, 2, 1, 2, 32>(k, s);
        case 0x93: return launch_persist<2, 2, 2, 1, 2, 64>(k, s);
        case 0xE1: return launch_wres_nfr<2, 4, 24>(k, s);
        case 0xE2: return launch_wres_nfr<2, 3, 24>(k, s);
        case 0xF1: return launch_wres_nfr<1, 4, 32>(k, s);
        case 0xF2: return launch_wres_nfr<1, 3, 32>(k, s);
    }
    BSY_FAIL(BSY_ERR_ARG, "conv: no streaming 1x1 kernel is built for configuration 0x%02x", id);
}
