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
template <int WAVES_M, int WAVES_N, int MT, int NT, int STAGES, int BK>
__global__ __launch_bounds__(512) void conv1x1_persist_kernel(const ConvK p) {
    constexpr int TM = WAVES_M * MT * 32, TN = WAVES_N * NT * 32;
    constexpr int TNS = TN < 64 ? 64 : TN;
    constexpr int CPR = BK / 8, RPI = 64 / CPR;
    constexpr int PIW = TM / (RPI * 4), WIW = TNS / (RPI * 4);
    constexpr int STAGE = (TM + TNS) * BK, NDMA = PIW + WIW;
    constexpr int SWS = BK == 32 ? 2 : 1;
    constexpr int LDT = TN + 8, OT = TM * LDT;
    static_assert(WAVES_M * WAVES_N == 4 && PIW >= 1 && WIW >= 1 && (BK == 32 || (!(PIW & 1) && !(WIW & 1))), "bad tile");
    __shared__ __attribute__((aligned(16))) half_t smem[STAGES * STAGE + OT + 2 * PERSIST_MAX_COUT];
    half_t* otile = smem + STAGES * STAGE;
    float* sbias = reinterpret_cast<float*>(otile + OT);  // the whole (padded) bias vector, loaded once: keeps ordinary VMEM
                                                          // loads -- and the vmcnt(0) they imply -- out of the tile loop

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk = p.Kpad / BK;
    const int ntiles = p.ntm * p.ntn;
    // XCD-aware tile walk (common.h xcd_tile_walk): the cout tiles of one pixel tile are neighbours in the tile order, so they run on
    // ONE XCD at the same time and the second reads the pixels from its L2 (model.4.cv2: 540 MB of traffic for 367 MB otherwise)
    const TileWalk tw = xcd_tile_walk(blockIdx.x, gridDim.x, ntiles);
    const int T0 = tw.tile, G = tw.step;
    const int my_tiles = T0 < tw.end ? (tw.end - T0 + G - 1) / G : 0;
    for (int i = tid; i < p.ntn * TN; i += 512) sbias[i] = p.bias[i];  // bias is padded to CoutPad (multiple of 128)
    __syncthreads();

    if (wave >= 4) {
        // ------------------------------------------------ store waves ------------------------------------------------
        const int st = tid - 256;
        constexpr int CPRW = TN / 8, ITER = TM * CPRW / 256;
        half_t* dst = reinterpret_cast<half_t*>(p.dst);
        for (int t = 0; t < my_tiles; ++t) {
            const int tile = T0 + t * G;
            const int m0 = (tile / p.ntn) * TM, n0 = (tile % p.ntn) * TN;
            for (int k = 0; k < nk; ++k) __builtin_amdgcn_s_barrier();  // B(t, k)
            __builtin_amdgcn_s_barrier();                              // E(t): tile t is parked
            half8 v[ITER];
#pragma unroll
            for (int i = 0; i < ITER; ++i) {
                const int id = st + 256 * i;
                v[i] = *reinterpret_cast<const half8*>(otile + (id / CPRW) * LDT + (id % CPRW) * 8);
            }
#pragma unroll
            for (int i = 0; i < ITER; ++i) {
                const int id = st + 256 * i;
                const int m = m0 + id / CPRW, c = n0 + (id % CPRW) * 8;
                if (m < p.M && c < p.Cout) *reinterpret_cast<half8*>(dst + (size_t)m * p.ldd + c) = v[i];
            }
            // all LDS reads have returned (their values were consumed by the stores' operands): the next barrier this
            // wave joins is B(t+1, 0), before which the compute waves cannot touch the parked tile again
        }
        return;
    }

    // ------------------------------------------------ compute + DMA waves ------------------------------------------------
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int rsub = lane / CPR, slot = lane % CPR;
    const int kc0 = BK == 32 ? (slot ^ ((rsub >> 2) & 3)) : (slot ^ (rsub >> 1));
    const int kc1 = BK == 32 ? kc0 : (slot ^ (4 | (rsub >> 1)));
    const bsy_rsrc_t rs0 = make_rsrc(p.src0, p.span0), rs1 = make_rsrc(p.src1 ? p.src1 : p.src0, p.src1 ? p.span1 : 0u),
                     rsw = make_rsrc(p.wgt, p.wspan);
    const int ohw = p.OH * p.OW;
    const int Cin = p.Cin8 * 8;

    // issue-side state (runs ahead of the compute side, across tile boundaries)
    unsigned off0[PIW], off1[PIW], woff[WIW];
    bool rv[PIW];
    int it = 0, ikt = 0, s_cb = 0;
    auto setup_tile = [&](int tcount) {
        const int tile = T0 + tcount * G;
        const int m0 = (tile / p.ntn) * TM, n0 = (tile % p.ntn) * TN;
#pragma unroll
        for (int i = 0; i < PIW; ++i) {
            const int m = m0 + (wave * PIW + i) * RPI + rsub;
            rv[i] = m < p.M;
            const int mm = rv[i] ? m : 0;
            if (!(p.up0 | p.up1) && p.stride == 1) {
                off0[i] = (unsigned)mm * (unsigned)p.ld0;
                off1[i] = (unsigned)mm * (unsigned)p.ld1;
            } else {
                const int n = mm / ohw, rem = mm - n * ohw, oh = rem / p.OW, ow = rem - oh * p.OW;
                const int iy = oh * p.stride, ix = ow * p.stride;
                const int H0 = p.H >> p.up0, W0 = p.W >> p.up0, H1 = p.H >> p.up1, W1 = p.W >> p.up1;
                off0[i] = (unsigned)((n * H0 + (iy >> p.up0)) * W0 + (ix >> p.up0)) * (unsigned)p.ld0;
                off1[i] = (unsigned)((n * H1 + (iy >> p.up1)) * W1 + (ix >> p.up1)) * (unsigned)p.ld1;
            }
        }
#pragma unroll
        for (int j = 0; j < WIW; ++j)
            woff[j] = (unsigned)(n0 + (wave * WIW + j) * RPI + rsub) * (unsigned)p.Kpad + ((j & 1) ? kc1 : kc0) * 8;
        s_cb = 0;
    };
    auto issue_step = [&](int stage) {
        if (ikt == 0) setup_tile(it);
        half_t* sP = smem + stage * STAGE;
        half_t* sW = sP + TM * BK;
        const bool s1 = s_cb >= p.C0;
        const unsigned sc = 2u * (unsigned)(s1 ? s_cb - p.C0 : s_cb);
#pragma unroll
        for (int i = 0; i < PIW; ++i) {
            const unsigned kcb = 16u * (unsigned)((i & 1) ? kc1 : kc0);
            const unsigned o = rv[i] ? 2u * (s1 ? off1[i] : off0[i]) + sc + kcb : BSY_OOB;
            if (s1) dma16_buf(rs1, o, 0u, sP + (wave * PIW + i) * RPI * BK);
            else dma16_buf(rs0, o, 0u, sP + (wave * PIW + i) * RPI * BK);
        }
#pragma unroll
        for (int j = 0; j < WIW; ++j)
            dma16_buf(rsw, 2u * woff[j], (unsigned)ikt * (2u * BK), sW + (wave * WIW + j) * RPI * BK);
        s_cb += BK;
        if (++ikt == nk) { ikt = 0; ++it; }
    };

    const int lrow = lane & 31, lh = lane >> 5;
    f32x16 acc[NT][MT];  // start at the bias of the tile's couts (common.h acc_bias), from the LDS copy of the bias vector
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc_bias(acc[a][b], sbias + (T0 % p.ntn) * TN + (wn * NT + a) * 32, lh);
    const int total = my_tiles * nk;
    int ip = 0;
    for (; ip < STAGES - 1 && ip < total; ++ip) issue_step(ip % STAGES);
    int ckt = 0, ct = 0;
    for (int cp = 0; cp < total; ++cp) {
        const int later = min(STAGES - 2, total - 1 - cp);
        if (later >= STAGES - 2 && STAGES > 2) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * NDMA) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();  // B(ct, ckt)
        if (ip < total) { issue_step(ip % STAGES); ++ip; }
        const half_t* sP = smem + (cp % STAGES) * STAGE;
        const half_t* sW = sP + TM * BK;
        constexpr int KSUB = BK / 16;
        half8 bfr[KSUB][MT], afr[KSUB][NT];
#pragma unroll
        for (int ks = 0; ks < KSUB; ++ks) {
            const int chunk = 2 * ks + lh;
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int row = (wm * MT + b) * 32 + lrow;
                bfr[ks][b] = *reinterpret_cast<const half8*>(sP + row * BK + ((chunk ^ ((row >> SWS) & (CPR - 1))) << 3));
            }
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                const int row = (wn * NT + a) * 32 + lrow;
                afr[ks][a] = *reinterpret_cast<const half8*>(sW + row * BK + ((chunk ^ ((row >> SWS) & (CPR - 1))) << 3));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < KSUB; ++ks)
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
                for (int b = 0; b < MT; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afr[ks][a], bfr[ks][b], acc[a][b], 0, 0, 0);
        if (++ckt == nk) {
            ckt = 0;
            const int n1 = ((T0 + (ct + 1) * G) % p.ntn) * TN;  // cout tile of the NEXT tile: its biases restart the accumulators
            // park SiLU(acc) as fp16 (the store waves finished reading the previous tile before B(ct, 0))
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int prow = (wm * MT + b) * 32 + lrow;
#pragma unroll
                for (int a = 0; a < NT; ++a) {
                    const int cl = (wn * NT + a) * 32;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c = cl + 8 * g + 4 * lh;
                        const f32x4 bn = *reinterpret_cast<const f32x4*>(sbias + n1 + c);
                        half4 o;
                        f32x4 tv = f32x4{acc[a][b][4 * g], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]};
                        if (p.act) tv = silu4_f(tv);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            o[e] = (half_t)tv[e];
                            acc[a][b][4 * g + e] = bn[e];
                        }
                        *reinterpret_cast<half4*>(otile + prow * LDT + c) = o;
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();  // E(ct)
            ++ct;
        }
    }
}

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
    hipLaunchKernelGGL((conv1x1_persist_kernel<WM, WN, MT, NT, STAGES, BK>), dim3((unsigned)grid), dim3(512), 0, s, p);
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
__global__ __launch_bounds__(256, 2) void conv1x1_wres_kernel(const ConvK p) {
    constexpr int BK = 32, MT = 2, TM = 128, TN = 64 * NT;
    constexpr int CPR = 4, RPI = 16;
    constexpr int PIW = TM / (RPI * 4);  // 2 pixel DMA wave-instructions per wave per K-step
    constexpr int STAGE = TM * BK;
    constexpr int LDT = TN + 8, OT = TM * LDT;
    constexpr int CPRW = TN / 8, NST = TM * CPRW / 256;  // 16-byte output pieces per thread per tile
    __shared__ __attribute__((aligned(16))) half_t smem[STAGES * STAGE + OT + 2 * TN];
    half_t* otile = smem + STAGES * STAGE;
    float* sbias = reinterpret_cast<float*>(otile + OT);  // this cout tile's biases: no ordinary VMEM load inside the tile loop

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = lane & 31, lh = lane >> 5;
    const int nk = p.Kpad / BK;
    // workgroup -> (cout tile, walk over the pixel tiles): blocks b, b + 8, .. b + 8 (ntn - 1) share their pixel tiles
    // (host: gridDim.x is a multiple of 8 ntn)
    constexpr int X = 8;
    const int x = blockIdx.x % X, q = blockIdx.x / X;
    const int ct = q % p.ntn, slot = q / p.ntn;                   // cout tile, walker index on this XCD
    const int walkers = (gridDim.x / X) / p.ntn;
    const int per = p.ntm / X, rem = p.ntm % X;
    const int pt0 = x * per + (x < rem ? x : rem), ptn = per + (x < rem ? 1 : 0);  // this XCD's range of pixel tiles
    const int my_tiles = slot < ptn ? (ptn - slot + walkers - 1) / walkers : 0;
    const int n0 = ct * TN;

    // A fragments of this wave's couts for the whole of K (rows past Cout: the packed matrix is padded to 128 rows with zeros)
    half8 afr[NFR];
    const int nfr = nk * 2 * NT;  // (k sub-step of 16, cout tile a)
#pragma unroll
    for (int i = 0; i < NFR; ++i) {
        afr[i] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        if (i < nfr) {
            const int ks = i / NT, a = i - ks * NT;
            afr[i] = *reinterpret_cast<const half8*>(p.wgt + (size_t)(n0 + (wn * NT + a) * 32 + lrow) * p.Kpad + 16 * ks + 8 * lh);
        }
    }
    if (tid < TN) sbias[tid] = p.bias[n0 + tid];  // bias is padded to CoutPad (a multiple of 128)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // weights and bias are in: from here on the vector-memory queue holds DMA and stores only
    __syncthreads();

    const int rsub = lane / CPR, slot4 = lane % CPR;
    const int kc = slot4 ^ ((rsub >> 2) & 3);
    const bsy_rsrc_t rs0 = make_rsrc(p.src0, p.span0), rs1 = make_rsrc(p.src1 ? p.src1 : p.src0, p.src1 ? p.span1 : 0u);
    const int ohw = p.OH * p.OW;
    unsigned off0[PIW], off1[PIW];
    bool rv[PIW];
    int it = 0, ikt = 0, s_cb = 0;
    auto setup_tile = [&](int tcount) {
        const int m0 = (pt0 + slot + tcount * walkers) * TM;
#pragma unroll
        for (int i = 0; i < PIW; ++i) {
            const int m = m0 + (wave * PIW + i) * RPI + rsub;
            rv[i] = m < p.M;
            const int mm = rv[i] ? m : 0;
            if (!(p.up0 | p.up1)) {
                off0[i] = (unsigned)mm * (unsigned)p.ld0;
                off1[i] = (unsigned)mm * (unsigned)p.ld1;
            } else {
                const int n = mm / ohw, r2 = mm - n * ohw, oh = r2 / p.OW, ow = r2 - oh * p.OW;
                const int H0 = p.H >> p.up0, W0 = p.W >> p.up0, H1 = p.H >> p.up1, W1 = p.W >> p.up1;
                off0[i] = (unsigned)((n * H0 + (oh >> p.up0)) * W0 + (ow >> p.up0)) * (unsigned)p.ld0;
                off1[i] = (unsigned)((n * H1 + (oh >> p.up1)) * W1 + (ow >> p.up1)) * (unsigned)p.ld1;
            }
        }
        s_cb = 0;
    };
    auto issue_step = [&](int stage) {
        if (ikt == 0) setup_tile(it);
        half_t* sP = smem + stage * STAGE;
        const bool s1 = s_cb >= p.C0;
        const unsigned sc = 2u * (unsigned)(s1 ? s_cb - p.C0 : s_cb) + 16u * (unsigned)kc;
#pragma unroll
        for (int i = 0; i < PIW; ++i) {
            const unsigned o = rv[i] ? 2u * (s1 ? off1[i] : off0[i]) + sc : BSY_OOB;
            if (s1) dma16_buf(rs1, o, 0u, sP + (wave * PIW + i) * RPI * BK);
            else dma16_buf(rs0, o, 0u, sP + (wave * PIW + i) * RPI * BK);
        }
        s_cb += BK;
        if (++ikt == nk) { ikt = 0; ++it; }
    };

    f32x16 acc[NT][MT];  // start at the bias of this cout tile (common.h acc_bias)
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc_bias(acc[a][b], sbias + (wn * NT + a) * 32, lh);
    const int total = my_tiles * nk;
    int ip = 0;
    for (; ip < STAGES - 1 && ip < total; ++ip) issue_step(ip % STAGES);
    int ckt = 0, ct_done = 0;
    half_t* dst = reinterpret_cast<half_t*>(p.dst);
    for (int cp = 0; cp < total; ++cp) {
        // wait for K-step cp.  Younger in this thread's vector-memory queue: the DMA of the next min(STAGES - 2, remaining) steps (PIW
        // each) and, while cp is one of the first STAGES - 1 steps of a tile after the first, the NST stores of the previous tile
        // (they were issued after the DMA of step cp, which went out STAGES - 1 steps ago)
        const int later = min(STAGES - 2, total - 1 - cp);
        const bool st_young = ct_done > 0 && ckt < STAGES - 1;
        if (later >= STAGES - 2) {
            if (st_young) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * PIW + NST) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * PIW) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        if (ip < total) { issue_step(ip % STAGES); ++ip; }
        const half_t* sP = smem + (cp % STAGES) * STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int chunk = 2 * ks + lh;
            half8 bfr[MT];
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int row = (wm * MT + b) * 32 + lrow;
                bfr[b] = *reinterpret_cast<const half8*>(sP + row * BK + ((chunk ^ ((row >> 2) & 3)) << 3));
            }
            // the A fragment index depends on the K-step: a uniform switch over compile-time register indices
#pragma unroll
            for (int kk = 0; kk < NFR / (2 * NT); ++kk)
                if (kk == ckt) {
#pragma unroll
                    for (int a = 0; a < NT; ++a)
#pragma unroll
                        for (int b = 0; b < MT; ++b)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afr[(2 * kk + ks) * NT + a], bfr[b], acc[a][b], 0, 0, 0);
                }
        }
        if (++ckt == nk) {
            ckt = 0;
            const int m0 = (pt0 + slot + ct_done * walkers) * TM;
            // bias + SiLU -> fp16 tile in LDS (the previous tile's stores have read it: their LDS reads completed before they were issued,
            // and every wave passed at least one barrier since)
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int prow = (wm * MT + b) * 32 + lrow;
#pragma unroll
                for (int a = 0; a < NT; ++a)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c = (wn * NT + a) * 32 + 8 * g + 4 * lh;
                        half4 o;
                        const f32x4 bn = *reinterpret_cast<const f32x4*>(sbias + c);  // the next tile's accumulators restart at the bias
                        f32x4 tv = f32x4{acc[a][b][4 * g], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]};
                        if (p.act) tv = silu4_f(tv);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            o[e] = (half_t)tv[e];
                            acc[a][b][4 * g + e] = bn[e];
                        }
                        *reinterpret_cast<half4*>(otile + prow * LDT + c) = o;
                    }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();  // (never __syncthreads(): it would drain the DMA ring)
            half8 v[NST];
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int id = tid + 256 * i;
                v[i] = *reinterpret_cast<const half8*>(otile + (id / CPRW) * LDT + (id % CPRW) * 8);
            }
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int id = tid + 256 * i;
                const int m = m0 + id / CPRW, c = n0 + (id % CPRW) * 8;
                // The counted waits assume NST store instructions per wave and tile.  A store whose predicate fails in SOME lanes is
                // still one instruction; one that fails in all lanes of a wave is skipped -- only possible in a tile that reaches past M,
                // which is the last tile of its walker (no wait follows it), since a cout tile always starts below Cout.
                if (m < p.M && c < p.Cout) *reinterpret_cast<half8*>(dst + (size_t)m * p.ldd + c) = v[i];
            }
            ++ct_done;
        }
    }
}

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
    hipLaunchKernelGGL((conv1x1_wres_kernel<NT, STAGES, NFR>), dim3((unsigned)grid), dim3(256), 0, s, p);
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
