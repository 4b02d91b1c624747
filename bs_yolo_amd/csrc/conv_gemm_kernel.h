// Included TWICE by conv_gemm.hip: with BSY_K(n) = n and BSY_RELU = false it defines the kernel(s) as they always were -- identity and SiLU by
// `act`, instruction for instruction what they were before activation id 2 existed (tools/isa_diff.py) --, with BSY_K(n) = n##_relu and
// BSY_RELU = true the same text as <name>_relu, whose epilogue is ReLU whatever `act` says.  The launchers pick by `act == 2`.
// (No include guard, on purpose.)
template <int KS, int WAVES_M, int WAVES_N, int MT, int NT, int STAGES, bool ALIGNED, int BK>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void BSY_K(conv_mfma_kernel)(const ConvK p) {
    constexpr bool RELU = BSY_RELU;
    constexpr int NW = WAVES_M * WAVES_N;   // waves per workgroup (4 or 8)
    constexpr int NTHR = 64 * NW;
    static_assert(BK == 32 || (BK == 64 && ALIGNED), "BK = 64 only for aligned layers");
    constexpr int TM = WAVES_M * MT * 32;
    constexpr int TN = WAVES_N * NT * 32;
    constexpr int TNS = TN < 64 ? 64 : TN;  // weight rows staged (>= 64 so that every wave issues the same DMA count;
                                            // the packed weights have >= 128 rows, the extra rows are simply unused)
    constexpr int CPR = BK / 8;             // 16-byte chunks per LDS row
    constexpr int RPI = 64 / CPR;           // rows filled by one DMA wave-instruction
    constexpr int PIW = TM / (RPI * NW);    // pixel-tile DMA instructions per wave
    constexpr int WIW = TNS / (RPI * NW);   // weight-tile DMA instructions per wave
    static_assert(PIW >= 1 && WIW >= 1 && (BK == 32 || (!(PIW & 1) && !(WIW & 1))), "tile too small for this wave count");
    constexpr int STAGE = (TM + TNS) * BK;  // halves per LDS stage
    constexpr int NDMA = PIW + WIW;         // DMA instructions per thread per K-step (identical for all waves)
    constexpr int SWS = BK == 32 ? 2 : 1;   // read-side swizzle: chunk ^ ((row >> SWS) & (CPR - 1))
    constexpr int OTILE = (TM > TN ? TM : TN) * ((TM > TN ? TN : TM) + 8);  // fp16 output tile staged by the coalesced epilogues:
                                                                             // [TM][TN + 8], or transposed [TN][TM + 8] (class scores)
    constexpr int SMEM = STAGES * STAGE > OTILE ? STAGES * STAGE : OTILE;
    __shared__ __attribute__((aligned(16))) half_t smem[SMEM];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    int wg = xcd_remap(blockIdx.x, gridDim.x);
    // split-K: workgroups [slice * tiles, (slice + 1) * tiles) compute slice `slice` of every tile
    const bool split = ALIGNED && p.nsl_c * p.nsl_t > 1;
    int slice = 0;
    if (split) {
        const int per = p.ntn * ((p.M + TM - 1) / TM);
        slice = wg / per;
        wg -= slice * per;
    }
    const int tap0 = split ? (slice % p.nsl_t) * p.taps_per : 0, tap1 = split ? tap0 + p.taps_per : p.ntaps;
    const int cb0 = split ? (slice / p.nsl_t) * p.cb_per : 0, cb1 = split ? cb0 + p.cb_per : p.Cin8 * 8;
    const int tn_idx = wg % p.ntn;
    const int tm_idx = wg / p.ntn;
    const int m0 = tm_idx * TM;
    const int n0 = tn_idx * TN;

    // ---- per-thread DMA coordinates: lane -> (row = lane / CPR, slot = lane % CPR) of the RPI x CPR block one
    //      wave-instruction fills; the slot holds source chunk slot ^ swizzle(row)  (== the read-side swizzle).
    //      BK = 32: swizzle(row) = (row>>2)&3 = (rsub>>2)&3.  BK = 64: (row>>1)&7 = ((q&1)<<2 | rsub>>1), q = instruction
    //      index inside the tile; PIW / WIW are even there, so the parity is that of the unrolled index.
    const int rsub = lane / CPR;
    const int slot = lane % CPR;
    const int kc0 = BK == 32 ? (slot ^ ((rsub >> 2) & 3)) : (slot ^ (rsub >> 1));  // even instructions
    const int kc1 = BK == 32 ? kc0 : (slot ^ (4 | (rsub >> 1)));                     // odd instructions (BK = 64)
    // per staged pixel row: element offset of the window origin pixel (tap 0,0 -> may be "negative" = wraps, only used
    // when the tap is valid) in each source, and a bitmask of the taps that fall inside the image
    unsigned off0[PIW], off1[PIW], vmask[PIW];
    const int ohw = p.OH * p.OW;
#pragma unroll
    for (int i = 0; i < PIW; ++i) {
        const int m = m0 + (wave * PIW + i) * RPI + rsub;
        const bool rv = m < p.M;
        const int mm = rv ? m : 0;
        int n, oh, ow;
        if (KS == 1 && p.stride == 1) {  // pixel index == m unless a source is upsampled
            n = 0; oh = 0; ow = 0;
            if (p.up0 | p.up1) { n = mm / ohw; const int rem = mm - n * ohw; oh = rem / p.OW; ow = rem - oh * p.OW; }
        } else {
            n = mm / ohw; const int rem = mm - n * ohw; oh = rem / p.OW; ow = rem - oh * p.OW;
        }
        const int iy0 = oh * p.stride - p.pad, ix0 = ow * p.stride - p.pad;
        if (KS == 1) {
            vmask[i] = rv ? 1u : 0u;
            if (p.stride == 1 && !(p.up0 | p.up1)) {
                off0[i] = (unsigned)mm * (unsigned)p.ld0;
                off1[i] = (unsigned)mm * (unsigned)p.ld1;
            } else {
                const int H0 = p.H >> p.up0, W0 = p.W >> p.up0, H1 = p.H >> p.up1, W1 = p.W >> p.up1;
                off0[i] = (unsigned)((n * H0 + (iy0 >> p.up0)) * W0 + (ix0 >> p.up0)) * (unsigned)p.ld0;
                off1[i] = (unsigned)((n * H1 + (iy0 >> p.up1)) * W1 + (ix0 >> p.up1)) * (unsigned)p.ld1;
            }
        } else {
            unsigned rb = 0, cb = 0;
#pragma unroll
            for (int t = 0; t < KS; ++t) {
                rb |= ((unsigned)(iy0 + t) < (unsigned)p.H ? 1u : 0u) << t;
                cb |= ((unsigned)(ix0 + t) < (unsigned)p.W ? 1u : 0u) << t;
            }
            unsigned vm = 0;
#pragma unroll
            for (int t = 0; t < KS; ++t) vm |= ((rb >> t) & 1u) ? (cb << (t * KS)) : 0u;
            vmask[i] = rv ? vm : 0u;
            const unsigned pix = (unsigned)((n * p.H + iy0) * p.W + ix0);  // wraps for border rows; masked there
            off0[i] = pix * (unsigned)p.ld0;
            off1[i] = pix * (unsigned)p.ld1;
        }
    }
    unsigned woff[WIW];
#pragma unroll
    for (int j = 0; j < WIW; ++j)
    {
        // rows past the packed matrix (a 32-wide cout tile stages 64 rows; the last cout tile of a 128-row matrix would read
        // rows 128..159): the descriptor path returns zeros for them, the flat-DMA (generic) path must not touch them --
        // clamp to the last packed row, the values are never used
        const int wrow = min(n0 + (wave * WIW + j) * RPI + rsub, ((p.Cout + 127) & ~127) - 1);
        woff[j] = (unsigned)wrow * (unsigned)p.Kpad + ((j & 1) ? kc1 : kc0) * 8;
    }
    const half_t* zero = reinterpret_cast<const half_t*>(bsy_zero_page);
    const bsy_rsrc_t rs0 = make_rsrc(p.src0, p.span0), rs1 = make_rsrc(p.src1 ? p.src1 : p.src0, p.src1 ? p.span1 : 0u),
                     rsw = make_rsrc(p.wgt, p.wspan);

    // K-step state.  ALIGNED: uniform (scalar) tap / channel base.  Generic: per-lane tap / 8-channel chunk index.
    int s_tap = tap0, s_cb = cb0;
    int tap = ALIGNED ? 0 : kc0 / p.Cin8;
    int c8 = ALIGNED ? 0 : kc0 - tap * p.Cin8;
    const int Cin = p.Cin8 * 8;

    // K-step state travels BY VALUE (cur_*) and is advanced by advance() below on plain locals: captured by reference and
    // mutated inside this lambda the four ints ended up in a 12-byte private (scratch) frame -- reloaded per lane and then
    // fed to the DMA's scalar offset operands through waterfall loops, in every ALIGNED instantiation (round-1 VERDICT)
    auto issue = [&](int kt, int stage, const int s_tap, const int s_cb, const int tap, const int c8) {
        half_t* sP = smem + stage * STAGE;
        half_t* sW = sP + TM * BK;
#ifdef BSY_ABLATE
        if (BSY_ABLATE & 1) return;  // no DMA
#endif
        if (ALIGNED) {
            const bool s1 = s_cb >= p.C0;
            const int ld = s1 ? p.ld1 : p.ld0;
            const int kh = (KS == 1) ? 0 : s_tap / KS;
            const int kw = (KS == 1) ? 0 : s_tap - kh * KS;
            // scalar part of the byte offset: tap displacement + channel base inside the source
            const unsigned sc = 2u * (unsigned)((kh * p.W + kw) * ld + (s1 ? s_cb - p.C0 : s_cb));
            const unsigned tbit = 1u << s_tap;
#pragma unroll
            for (int i = 0; i < PIW; ++i) {
                const unsigned kcb = 16u * (unsigned)((i & 1) ? kc1 : kc0);
                const unsigned o = (vmask[i] & tbit) ? 2u * (s1 ? off1[i] : off0[i]) + sc + kcb : BSY_OOB;
                if (s1) dma16_buf(rs1, o, 0u, sP + (wave * PIW + i) * RPI * BK);
                else dma16_buf(rs0, o, 0u, sP + (wave * PIW + i) * RPI * BK);
            }
#pragma unroll
            for (int j = 0; j < WIW; ++j)
                dma16_buf(rsw, 2u * woff[j], 2u * (unsigned)(s_tap * Cin + s_cb), sW + (wave * WIW + j) * RPI * BK);
        } else {
            const bool kvalid = tap < p.ntaps;
            const int kh = (KS == 1) ? 0 : tap / KS;
            const int kw = (KS == 1) ? 0 : tap - kh * KS;
            const int cc = c8 * 8;
            const bool s1 = cc >= p.C0;
            const half_t* base = s1 ? p.src1 : p.src0;
            const int ld = s1 ? p.ld1 : p.ld0;
            const unsigned sc = (unsigned)((kh * p.W + kw) * ld + (s1 ? cc - p.C0 : cc));
            const unsigned tbit = kvalid ? (1u << tap) : 0u;
#pragma unroll
            for (int i = 0; i < PIW; ++i) {
                const unsigned o = (s1 ? off1[i] : off0[i]) + sc;
                const half_t* g = (vmask[i] & tbit) ? base + (size_t)o : zero;
                dma16(g, sP + (wave * PIW + i) * RPI * BK);
            }
#pragma unroll
            for (int j = 0; j < WIW; ++j)
                dma16(p.wgt + (size_t)(woff[j] + (unsigned)kt * 32u), sW + (wave * WIW + j) * RPI * BK);
        }
    };
#define BSY_ADVANCE_K()                                                                                  \
    do {                                                                                                 \
        if (ALIGNED) {                                                                                   \
            if (p.korder == 1 || (p.korder == 2 && BK == 64)) { /* chunk-major, chunk = this kernel's BK */ \
                if (++s_tap >= tap1) { s_tap = tap0; s_cb += BK; }                                       \
            } else if (p.korder == 2) { /* 64-channel chunks walked by a BK-32 kernel: (tap, half) */       \
                if (s_cb & 32) { s_cb -= 32; if (++s_tap >= tap1) { s_tap = tap0; s_cb += 64; } }        \
                else s_cb += 32;                                                                         \
            } else {                                                                                     \
                s_cb += BK;                                                                              \
                if (s_cb >= cb1) { s_cb = cb0; ++s_tap; }                                                \
            }                                                                                            \
        } else {                                                                                         \
            c8 += 4;                                                                                     \
            while (c8 >= p.Cin8) { c8 -= p.Cin8; ++tap; }                                                \
        }                                                                                                \
    } while (0)

    const int lrow = lane & 31;
    const int lh = lane >> 5;
    const int nk = split ? (tap1 - tap0) * (cb1 - cb0) / BK : p.Kpad / BK;
    f32x16 acc[NT][MT];  // start at the bias of their couts (common.h acc_bias); split-K: in slice 0 only
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) {
            acc_bias(acc[a][b], p.bias + n0 + (wn * NT + a) * 32, lh);
            if (slice) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
            }
        }

    // prologue: STAGES-1 K-steps in flight
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s)
        if (s < nk) { issue(s, s, s_tap, s_cb, tap, c8); BSY_ADVANCE_K(); }

    for (int kt = 0; kt < nk; ++kt) {
        // wait for K-step kt: everything issued after it may stay in flight
        const int later = min(STAGES - 2, nk - 1 - kt);  // K-steps issued after kt that are still outstanding
        if (later >= STAGES - 2 && STAGES > 2) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 2) * NDMA) : "memory");
        } else if (STAGES > 3 && later == STAGES - 3) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES > 3 ? STAGES - 3 : 0) * NDMA) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();  // K-step kt visible to every wave; every wave is done reading stage (kt-1)%STAGES
        if (kt + STAGES - 1 < nk) { issue(kt + STAGES - 1, (kt + STAGES - 1) % STAGES, s_tap, s_cb, tap, c8); BSY_ADVANCE_K(); }
        const half_t* sP = smem + (kt % STAGES) * STAGE;
        const half_t* sW = sP + TM * BK;
        // Fragment reads run ONE 16-wide sub-step ahead of the MFMAs that use them (two register sets; the sched_barriers pin the
        // order -- left alone the scheduler reuses one set and serialises read -> wait -> MFMAs).  The workgroup's waves leave the
        // barrier together, so with all reads of the K-step in front of its MFMA burst (the round-1 form) every wave read while the
        // matrix pipes idled and then every wave multiplied while the LDS idled: 20 us of a 10-us MFMA floor on model.8.cv2 with
        // DMA and epilogue switched off.  Same MFMA order (ks, cout tile, pixel tile): same bits.
        constexpr int KSUB = BK / 16;
        half8 bfr[2][MT], afr[2][NT];
        auto rd = [&](const int ks, const int buf) {
            const int chunk = 2 * ks + lh;
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const int row = (wm * MT + b) * 32 + lrow;
                bfr[buf][b] = *reinterpret_cast<const half8*>(sP + row * BK + ((chunk ^ ((row >> SWS) & (CPR - 1))) << 3));
            }
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                const int row = (wn * NT + a) * 32 + lrow;
                afr[buf][a] = *reinterpret_cast<const half8*>(sW + row * BK + ((chunk ^ ((row >> SWS) & (CPR - 1))) << 3));
            }
        };
        rd(0, 0);
#pragma unroll
        for (int ks = 0; ks < KSUB; ++ks) {
            if (ks + 1 < KSUB) rd(ks + 1, (ks + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
                for (int b = 0; b < MT; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afr[ks & 1][a], bfr[ks & 1][b], acc[a][b], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#ifdef BSY_ABLATE
    if (BSY_ABLATE & 4) {  // no epilogue
        if (acc[0][0][0] == 12345.678f) reinterpret_cast<float*>(p.dst)[0] = 1.f;  // keep the accumulators live
        return;
    }
#endif
    if (split) {  // raw f32 sums of this slice -> its slab [pixel][ldw]; lane = pixel, registers 4 g .. 4 g + 3 = couts 8 g + 4 lh + {0..3}
        float* ws = p.split_ws + (size_t)slice * (size_t)p.slab;
#pragma unroll
        for (int b = 0; b < MT; ++b) {
            const int m = m0 + (wm * MT + b) * 32 + lrow;
            if (m >= p.M) continue;
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                const int cbase = n0 + (wn * NT + a) * 32;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = cbase + 8 * g + 4 * lh;
                    if (c < p.ldw) *reinterpret_cast<f32x4*>(ws + (size_t)m * p.ldw + c) = f32x4{acc[a][b][4 * g], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]};
                }
            }
        }
        return;
    }
    if (p.epi) {  // fused Detect decoder
        if (p.epi == 2 && !p.y_f32 && !p.raw) {
            __syncthreads();  // every wave has finished reading the last K-step: LDS becomes the transposed score tile
            conv_epilogue_cls_lds<TM, TN, MT, NT, NTHR>(p, acc, smem, m0, n0, wm, wn, lrow, lh, tid);
        } else {
            conv_epilogue_head<MT, NT>(p, acc, m0, n0, wm, wn, lrow, lh);
        }
        return;
    }
    const bool lds_epi = !p.out_f32 && !(p.Cout & 7) && !(p.ldd & 7) && !((uintptr_t)p.dst & 15) && p.dst_scale == 1 &&
                         (!p.res || (!(p.ldr & 7) && !((uintptr_t)p.res & 15)));
    if (lds_epi) {
        __syncthreads();  // every wave has finished reading the last K-step (all DMA already drained by vmcnt(0))
        conv_epilogue_lds<TM, TN, MT, NT, NTHR, RELU>(p, acc, smem, m0, n0, wm, wn, lrow, lh, tid);
    } else {
        conv_epilogue<MT, NT, RELU>(p, acc, m0, n0, wm, wn, lrow, lh);
    }
}

__global__ __launch_bounds__(256) void BSY_K(splitk_reduce_kernel)(const float* __restrict__ ws, const int nsl, const long long slab, const int ldw,
                                                           const int M, const int Cout, const int act, const half_t* __restrict__ res, const int ldr,
                                                           half_t* __restrict__ dst, const int ldd) {
    constexpr bool RELU = BSY_RELU;
    const int c8n = Cout >> 3;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)M * c8n) return;
    const int c = (int)(idx % c8n) * 8;
    const size_t m = (size_t)(idx / c8n);
    const float* wp = ws + m * ldw + c;
    f32x4 a0 = *reinterpret_cast<const f32x4*>(wp), a1 = *reinterpret_cast<const f32x4*>(wp + 4);
    for (int sl = 1; sl < nsl; ++sl) {
        const float* q = wp + (size_t)sl * (size_t)slab;
        a0 = add4_f(a0, *reinterpret_cast<const f32x4*>(q));
        a1 = add4_f(a1, *reinterpret_cast<const f32x4*>(q + 4));
    }
    float v[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    if (RELU) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = relu_f(v[e]);
    } else if (act) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = silu_f(v[e]);
    }
    if (res) {
        const half8 rv = *reinterpret_cast<const half8*>(res + m * ldr + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += (float)rv[e];
    }
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)v[e];
    *reinterpret_cast<half8*>(dst + m * ldd + c) = o;
}
