// Included TWICE by conv_stream1x1.hip: with BSY_K(n) = n and BSY_RELU = false it defines the kernel(s) as they always were -- identity and SiLU by
// `act`, instruction for instruction what they were before activation id 2 existed (tools/isa_diff.py) --, with BSY_K(n) = n##_relu and
// BSY_RELU = true the same text as <name>_relu, whose epilogue is ReLU whatever `act` says.  The launchers pick by `act == 2`.
// (No include guard, on purpose.)
template <int WAVES_M, int WAVES_N, int MT, int NT, int STAGES, int BK>
__global__ __launch_bounds__(512) void BSY_K(conv1x1_persist_kernel)(const ConvK p) {
    constexpr bool RELU = BSY_RELU;
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
            // park act(acc) as fp16 (the store waves finished reading the previous tile before B(ct, 0))
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
                        if constexpr (RELU) tv = relu4_f(tv);
                        else if (p.act) tv = silu4_f(tv);
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

template <int NT, int STAGES, int NFR>
__global__ __launch_bounds__(256, 2) void BSY_K(conv1x1_wres_kernel)(const ConvK p) {
    constexpr bool RELU = BSY_RELU;
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
            // bias + act -> fp16 tile in LDS (the previous tile's stores have read it: their LDS reads completed before they were issued,
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
                        if constexpr (RELU) tv = relu4_f(tv);
                        else if (p.act) tv = silu4_f(tv);
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
