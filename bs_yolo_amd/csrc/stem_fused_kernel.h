// Included TWICE by stem_fused.hip: with BSY_K(n) = n and BSY_RELU = false it defines the kernel(s) as they always were -- identity and SiLU by
// `act`, instruction for instruction what they were before activation id 2 existed (tools/isa_diff.py) --, with BSY_K(n) = n##_relu and
// BSY_RELU = true the same text as <name>_relu, whose epilogue is ReLU whatever `act` says.  The launchers pick by `act == 2`.
// (No include guard, on purpose.)
template <typename T, int C0, int C1>
__global__ __launch_bounds__(256, sizeof(T) == 4 ? 2 : 3) void BSY_K(stem_fused_kernel)(const StemK p) {
    constexpr bool RELU = BSY_RELU;
    constexpr int NCH = C0 / 8;               // 16-byte chunks per layer-0 patch entry
    constexpr int KS1 = (9 * C0 + 15) / 16;   // layer-1 K sub-steps (16 wide)
    constexpr int NH = C1 / 32;               // layer-1 cout tiles; waves 0 .. 2*NH-1 compute layer 1
    constexpr int LDO = C1 + 8;               // padded output-tile row (halves)
    constexpr int IMG = ST_IR * ST_ROWPX * 4;
    constexpr int MID = ST_NE * C0;
    constexpr int OUT = ST_TH * ST_TW * LDO;
    static_assert(C0 == 16 || C0 == 32, "layer-0 width");
    static_assert(NH == 1 || NH == 2, "layer-1 width");
    __shared__ __attribute__((aligned(16))) half_t lds[IMG + MID + OUT + 2 * (C0 + C1)];
    half_t* simg = lds;
    half_t* smid = lds + IMG;
    half_t* sout = smid + MID;
    float* sb0 = reinterpret_cast<float*>(sout + OUT);  // biases: LDS reads instead of a global load + wait per tile
    float* sb1 = sb0 + C0;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 31, lh = lane >> 5;
    const T* img = reinterpret_cast<const T*>(p.img);

    // ---- launch-invariant operands and per-lane tables -------------------------------------------------------------
    if (tid < C0) sb0[tid] = p.b0[tid];
    if (tid < C1) sb1[tid] = p.b1[tid];
    half8 a0[IMGC_KSUB];  // layer-0 weights: rows = couts (C0 <= 32 -> one tile), [CoutPad][64] packed, k = (kh, kw, c4)
#pragma unroll
    for (int s = 0; s < IMGC_KSUB; ++s)
        a0[s] = *reinterpret_cast<const half8*>(p.w0 + (size_t)lrow * IMGC_KROW + 16 * s + 8 * lh);
    const int mt1 = wave & 1, nh1 = wave >> 1;  // layer-1 role: pixel tile (2 rows x 16) and cout tile
    const bool l1 = nh1 < NH;
    half8 a1[KS1];  // layer-1 weights, [CoutPad][Kpad1] packed, k = (kh, kw, c)
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks)
        a1[ks] = l1 ? *reinterpret_cast<const half8*>(p.w1 + (size_t)(nh1 * 32 + lrow) * p.Kpad1 + 16 * ks + 8 * lh)
                    : half8{0, 0, 0, 0, 0, 0, 0, 0};
    // load items of this thread: (image row r, group j) -> patch position; tile-independent
    int it_r[ST_NLOAD], it_j[ST_NLOAD];
#pragma unroll
    for (int i = 0; i < ST_NLOAD; ++i) {
        const int idx = tid + 256 * i;
        it_r[i] = idx / ST_NG;
        it_j[i] = idx - it_r[i] * ST_NG;
    }
    const int e1base = (2 * (2 * mt1 + (lrow >> 4))) * ST_C0W + (lrow & 15);  // layer-1 lane pixel -> patch entry of tap (0, 0)

    ImgItem<T> pre[ST_NLOAD];
    int nn = 0, noy0 = 0, nox0 = 0;  // coordinates of the tile whose patch is in `pre`
    auto fetch = [&](int tile) {
        const TileOrigin o = tile_origin<ST_TH, ST_TW>(p.grid, tile);
        nn = o.n; noy0 = o.oy0; nox0 = o.ox0;
        const int n = nn, oy0 = noy0, ox0 = nox0;
        const T* ip = img + (size_t)n * 3 * p.H * p.W;
#pragma unroll
        for (int i = 0; i < ST_NLOAD; ++i)
            pre[i] = img_item_load<T>(ip, p.H, p.W, 4 * oy0 - 3 + it_r[i], 4 * ox0 - 4 + 4 * it_j[i], tid + 256 * i < ST_NITEM);
    };

    // Retire the weight / bias loads HERE: left pending, the compiler waits for them at their first use inside the tile
    // loop with vmcnt(0) -- on every iteration, which then also waits for the prefetch issued just before.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    const TileWalk tw = xcd_tile_walk(blockIdx.x, gridDim.x, p.grid.ntiles);  // XCD-aware tile order (common.h)
    int tile = tw.tile;
    if (tile < tw.end) fetch(tile);
    for (; tile < tw.end; tile += tw.step) {
        const int n = nn, oy0 = noy0, ox0 = nox0;
#pragma unroll
        for (int i = 0; i < ST_NLOAD; ++i)
            if (tid + 256 * i < ST_NITEM) img_item_park<T>(pre[i], simg + (it_r[i] * ST_ROWPX + 4 * it_j[i]) * 4);
        lds_barrier();  // image patch visible; every wave is done with the previous tile's LDS
        if (tile + tw.step < tw.end) fetch(tile + tw.step);

        // ---- layer 0: 297 patch pixels = 10 MFMA pixel tiles, dealt round-robin to the 4 waves ----------------------
        const int r00 = 2 * oy0 - 1, c00 = 2 * ox0 - 1;  // layer-0 coordinates of patch entry (0, 0)
        for (int mt = wave; mt < ST_NMT; mt += 4) {
            const int pp = mt * 32 + lrow;
            const int pc = pp < ST_NE ? pp : ST_NE - 1;
            const int r = pc / ST_C0W, c = pc - r * ST_C0W;
            const int win = (2 * r * ST_ROWPX + 2 * c + 1) * 4;  // window origin: image-patch pixel (2r, 2c + 1)
            f32x16 acc;
            acc_bias(acc, sb0, lh);  // accumulators start at the bias (common.h acc_bias)
#pragma unroll
            for (int s = 0; s < IMGC_KSUB; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0[s], img_frag<ST_ROWPX>(simg, win, s, lh), acc, 0, 0, 0);
            // bias + SiLU -> f16; positions outside the layer-0 map are layer 1's zero padding
            const unsigned keep = ((unsigned)(r00 + r) < (unsigned)p.OH0 && (unsigned)(c00 + c) < (unsigned)p.OW0) ? 0xffffffffu : 0u;
            const int e = r * ST_C0W + (c & 1) * ST_EV + (c >> 1);
            if (pp < ST_NE) {
#pragma unroll
                for (int g = 0; g < NCH; ++g)  // couts 8g + 4lh .. +3  (C0 = 16: g < 2 only)
                    *reinterpret_cast<half4*>(smid + (e * NCH + (g ^ ((e >> 2) & (NCH - 1)))) * 8 + 4 * lh) = act_f16<RELU>(acc_group(acc, g), p.act, keep);
            }
        }
        lds_barrier();  // layer-0 patch complete

        // ---- layer 1: wave = (pixel tile of 2 rows x 16, cout tile of 32) --------------------------------------------
        if (l1) {
            f32x16 acc;
            acc_bias(acc, sb1 + nh1 * 32, lh);
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) {
                // k = 16 ks + 8 lh + (0..7) = tap * C0 + channel: one tap and one 8-channel chunk per lane half
                const int k0 = 16 * ks, k1 = k0 + 8;
                const int t0 = k0 / C0, t1 = k1 / C0;  // compile-time
                const int ch0 = (k0 % C0) / 8, ch1 = (k1 % C0) / 8;
                const int e0 = t0 < 9 ? (t0 / 3) * ST_C0W + ((t0 % 3) & 1) * ST_EV + ((t0 % 3) >> 1) : 0;
                const int e1 = t1 < 9 ? (t1 / 3) * ST_C0W + ((t1 % 3) & 1) * ST_EV + ((t1 % 3) >> 1) : 0;
                const int e = e1base + (e0 == e1 ? e0 : (lh ? e1 : e0));
                const int ch = lh ? ch1 : ch0;
                half8 bf = *reinterpret_cast<const half8*>(smid + (e * NCH + (ch ^ ((e >> 2) & (NCH - 1)))) * 8);
                if (t1 >= 9 && (t0 >= 9 || lh)) bf = half8{0, 0, 0, 0, 0, 0, 0, 0};  // K padding (C0 = 16: k >= 144)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1[ks], bf, acc, 0, 0, 0);
            }
            const int prow = mt1 * 32 + lrow;
#pragma unroll
            for (int g = 0; g < 4; ++g) *reinterpret_cast<half4*>(sout + prow * LDO + (nh1 * 32 + 8 * g + 4 * lh)) = act_f16<RELU>(acc_group(acc, g), p.act);
        }
        lds_barrier();  // output tile complete

        store_tile<ST_TH, ST_TW, C1, LDO, 256>(p.dst, p.OH1, p.OW1, p.ldd, sout, n, oy0, ox0, tid);
    }
}
