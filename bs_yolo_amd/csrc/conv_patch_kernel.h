// Included TWICE by conv_patch.hip: with BSY_K(n) = n and BSY_RELU = false it defines the kernel(s) as they always were -- identity and SiLU by
// `act`, instruction for instruction what they were before activation id 2 existed (tools/isa_diff.py) --, with BSY_K(n) = n##_relu and
// BSY_RELU = true the same text as <name>_relu, whose epilogue is ReLU whatever `act` says.  The launchers pick by `act == 2`.
// (No include guard, on purpose.)
template <int NT, int STAGES, int WM, int TW_ = CP_TW, bool TAIL = false>
__global__ __launch_bounds__(128 * WM) void BSY_K(conv3x3_patch_kernel)(const ConvK p) {
    constexpr bool RELU = BSY_RELU;
    constexpr int CP_TH = TW_ == 16 ? 4 * WM : 6, NW = 2 * WM, NTHR = 64 * NW;
    constexpr int PW_ = TW_ + 2;                            // patch row length (entries)
    constexpr int NVALID = CP_TH * TW_;                     // pixels of the tile (<= TM slots)
    static_assert(TW_ == 16 || (TW_ == 20 && WM == 2), "tile shapes: 8 x 16, 16 x 16 (8 waves), 6 x 20");
    constexpr int CP_NPX = (CP_TH + 2) * PW_;               // 180 / 324 / 176 patch entries
    constexpr int PIW = (CP_NPX + 16 * NW - 1) / (16 * NW);  // patch DMA wave-instructions per wave per chunk (16 entries each)
    constexpr int CP_NPI = PIW * NW;
    constexpr int TN = 64 * NT, TM = 64 * WM;
    constexpr int PBUF = CP_NPI * 16 * 32;  // halves per patch buffer
    constexpr int WTAP = TN * 32;           // halves per tap of a weight stage
    constexpr int WST = 3 * WTAP;           // halves per weight stage (3 taps)
    constexpr int WIW = 3 * TN / 64;        // weight DMA wave-instructions per wave per step (4-wave form; counted waits)
    constexpr int OTILE = TM * (TN + 8);
    constexpr int RING = 2 * PBUF + STAGES * WST;
    constexpr int SMEM = RING > OTILE ? RING : OTILE;
    static_assert(STAGES == 2 || ((STAGES == 3 || STAGES == 4) && WM == 2), "ring depth (the 8-wave form deals the weight DMA unevenly: vmcnt(0) only)");
    // STAGES <= 4: the patch of chunk c is issued at kernel row 0 of chunk c - 1, i.e. before (or in the same step as, and then ahead
    // of) the weights of chunk c's first step as long as those are issued at most three steps ahead; a deeper ring would let that
    // step's wait pass with the patch still in flight.
    __shared__ __attribute__((aligned(16))) half_t smem[SMEM];
    half_t* sW = smem + 2 * PBUF;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;  // wave grid WM x 2: 64 pixels (4 tile rows) x NT*32 couts each
    const int lrow = lane & 31, lh = lane >> 5;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int tn_idx = wg % p.ntn;
    int t = wg / p.ntn;
    const int tx = t % p.tiles_x;
    t /= p.tiles_x;
    const int ty = t % p.tiles_y;
    const int n = t / p.tiles_y;
    const int oy0 = ty * CP_TH, ox0 = tx * TW_, n0 = tn_idx * TN;

    const bsy_rsrc_t rs0 = make_rsrc(p.src0, p.span0), rsw = make_rsrc(p.wgt, p.wspan);
    // patch DMA coordinates: instruction i of this wave fills entries 16 (wave + 4 i) .. +15; lane -> (entry, slot)
    unsigned poff[PIW];
#pragma unroll
    for (int i = 0; i < PIW; ++i) {
        const int q = 16 * (wave + NW * i) + (lane >> 2);
        const int pr = q / PW_, pc = q - pr * PW_;
        const int y = oy0 - 1 + pr, x = ox0 - 1 + pc;
        const int chunk = (lane & 3) ^ ((q >> 2) & 3);
        poff[i] = (q < CP_NPX && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W)
                      ? 2u * ((unsigned)((n * p.H + y) * p.W + x) * (unsigned)p.ld0 + 8u * chunk) : BSY_OOB;
    }
    // weight DMA coordinates: the stage is [tap kw][TN rows][64 B] = 3 * TN/16 wave-instructions of 16 rows.  Four waves:
    // wave w takes row groups w, w+4, .. of every tap.  Eight waves: row group g of tap kw goes to wave (g & 3) + 4 * (kw & 1)
    // (waves 0-3 serve taps 0 and 2, waves 4-7 tap 1).
    constexpr int WPT = TN / 64;  // row groups per wave per tap
    unsigned woff[WPT];
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
        const int r = 16 * (4 * j + (wave & 3)) + (lane >> 2);
        woff[j] = 2u * ((unsigned)(n0 + r) * (unsigned)p.Kpad + 8u * ((lane & 3) ^ ((r >> 2) & 3)));
    }
    const int Cin = p.Cin8 * 8;
    const int nchunks = Cin >> 5, nsteps = 3 * nchunks;

    auto issue_patch = [&](int chunk) {
        half_t* dst = smem + (chunk & 1) * PBUF;
#pragma unroll
        for (int i = 0; i < PIW; ++i) dma16_buf(rs0, poff[i], 64u * (unsigned)chunk, dst + (wave + NW * i) * 512);
    };
    int w_kh = 0, w_chunk = 0;  // (chunk, kernel row) of the next weight step to issue
    auto issue_weights = [&](int step) {
        half_t* dst = sW + (step % STAGES) * WST;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            if (WM == 4 && (kw & 1) != (wave >> 2)) continue;  // wave-uniform
            const unsigned koff = 2u * (unsigned)((w_kh * 3 + kw) * Cin + 32 * w_chunk);
#pragma unroll
            for (int j = 0; j < WPT; ++j) dma16_buf(rsw, woff[j], koff, dst + kw * WTAP + (4 * j + (wave & 3)) * 512);
        }
        if (++w_kh == 3) { w_kh = 0; ++w_chunk; }
    };

    f32x16 acc[NT][2];  // start at the bias of their couts (common.h acc_bias)
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc_bias(acc[a][b], p.bias + n0 + (wn * NT + a) * 32, lh);
    // lane pixel of MFMA tile b: tile row wm*4 + 2b + (lrow >> 4), column lrow & 15 -> patch entry of tap (0, 0)
    int lq[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int slot = (wm * 2 + b) * 32 + lrow;  // pixel slot -> pixel (slot / TW, slot % TW); slots past the tile read entry 0
        lq[b] = slot < NVALID ? (slot / TW_) * PW_ + slot % TW_ : 0;
    }
    int arow[NT], asw[NT];
#pragma unroll
    for (int a = 0; a < NT; ++a) {
        arow[a] = ((wn * NT + a) * 32 + lrow) * 32;
        asw[a] = (lh ^ ((lrow >> 2) & 3)) << 3;
    }

    issue_patch(0);
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s)
        if (s < nsteps) issue_weights(s);
    int kh = 0, chunk = 0;
    for (int k = 0; k < nsteps; ++k) {
        // wait for W(k) (and everything older: this chunk's patch); younger: W(k+1 .. k+STAGES-2) and, when this is the
        // kernel row after a patch issue, the next chunk's patch
        const int younger = min(STAGES - 2, nsteps - 1 - k);
        // the next chunk's patch is issued at kernel row 0, behind W(k + STAGES - 2) of that step: it is younger than W(k) during the
        // following STAGES - 2 steps
        const bool p_young = STAGES > 2 ? (kh >= 1 && kh <= STAGES - 2 && chunk + 1 < nchunks) : false;
        if (younger <= 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (STAGES > 3 && younger >= 2) {
            if (p_young) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * WIW + PIW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * WIW) : "memory");
        } else if (p_young) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WIW + PIW) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WIW) : "memory");
        }
        __builtin_amdgcn_s_barrier();  // step k visible to every wave; every wave is done reading step k-1
        if (kh == 0 && chunk + 1 < nchunks) issue_patch(chunk + 1);
        if (k + STAGES - 1 < nsteps) issue_weights(k + STAGES - 1);
        const half_t* sP = smem + (chunk & 1) * PBUF;
        const half_t* sWk = sW + (k % STAGES) * WST;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int toff = kh * PW_ + kw;
            half8 bfr[2][2], afr[2][NT];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int q = lq[b] + toff;
                const int s0 = lh ^ ((q >> 2) & 3);
                const half_t* e = sP + q * 32;
                bfr[0][b] = *reinterpret_cast<const half8*>(e + (s0 << 3));
                bfr[1][b] = *reinterpret_cast<const half8*>(e + ((s0 ^ 2) << 3));
            }
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                const half_t* e = sWk + kw * WTAP + arow[a];
                afr[0][a] = *reinterpret_cast<const half8*>(e + asw[a]);
                afr[1][a] = *reinterpret_cast<const half8*>(e + (asw[a] ^ 16));
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int a = 0; a < NT; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afr[ks][a], bfr[ks][b], acc[a][b], 0, 0, 0);
        }
        if (++kh == 3) { kh = 0; ++chunk; }
    }
    // TAIL: the 1x1 weights (A operand, [128][64] packed, k = channel; rows = box logits a * 32 + lrow) are fetched now, so that
    // their latency passes under the SiLU / LDS stage below (every DMA has drained: the loop ends on vmcnt(0))
    half8 ta[TAIL ? 4 : 1][2];
    if (TAIL) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int a = 0; a < 2; ++a)
                ta[TAIL ? ks : 0][a] = *reinterpret_cast<const half8*>(p.tail_wgt + (size_t)(a * 32 + lrow) * 64 + 16 * ks + 8 * lh);
    }
    __syncthreads();  // every wave has finished reading the last step: LDS becomes the output tile

    constexpr int LDT = TN + 8;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int prow = (wm * 2 + b) * 32 + lrow;  // = tile row * 16 + column
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const int cl = (wn * NT + a) * 32;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = cl + 8 * g + 4 * lh;
                half4 o;
                f32x4 tv = f32x4{acc[a][b][4 * g], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]};
                if constexpr (RELU) tv = relu4_f(tv);
                else if (p.act) tv = silu4_f(tv);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (half_t)tv[e];
                *reinterpret_cast<half4*>(smem + prow * LDT + c) = o;
            }
        }
    }
    __syncthreads();
    if (TAIL) {
        static_assert(!TAIL || (NT == 1 && WM == 2), "tail: 64-cout tiles, four waves");
        const int slot = wave * 32 + lrow;
        f32x16 t0, t1;  // box logits 0..31 / 32..63 of this lane's pixel, starting at the 1x1 conv's bias
        acc_bias(t0, p.tail_bias, lh);
        acc_bias(t1, p.tail_bias + 32, lh);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const half8 tb = *reinterpret_cast<const half8*>(smem + slot * LDT + 16 * ks + 8 * lh);
            t0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ta[TAIL ? ks : 0][0], tb, t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ta[TAIL ? ks : 0][1], tb, t1, 0, 0, 0);
        }
        const int oy = oy0 + slot / TW_, ox = ox0 + slot % TW_;
        const bool mv = slot < NVALID && oy < p.H && ox < p.W;
        const int pix = mv ? oy * p.W + ox : 0;
        const int hw = p.H * p.W;
        dfl_decode_store(p, t0, t1, mv, (size_t)n * p.nrows * p.A + p.a0 + pix, (size_t)n * p.rawC * hw + pix, pix, lh);
        return;
    }
    constexpr int CPRW = TN / 8, ITER = TM * CPRW / NTHR;
    half_t* dst = reinterpret_cast<half_t*>(p.dst);
#pragma unroll
    for (int i = 0; i < ITER; ++i) {
        const int id = tid + NTHR * i;
        const int prow = id / CPRW, cc = (id % CPRW) * 8;
        const int oy = oy0 + prow / TW_, ox = ox0 + prow % TW_, c = n0 + cc;
        if (prow >= NVALID || oy >= p.H || ox >= p.W || c >= p.Cout) continue;
        const size_t pix = (size_t)(n * p.H + oy) * p.W + ox;
        half8 v = *reinterpret_cast<const half8*>(smem + prow * LDT + cc);
        if (p.res) {
            const half8 r = *reinterpret_cast<const half8*>(p.res + pix * p.ldr + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] + (float)r[e]);
        }
        *reinterpret_cast<half8*>(dst + pix * p.ldd + c) = v;
    }
}
