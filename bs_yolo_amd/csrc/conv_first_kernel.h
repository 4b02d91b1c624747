// Included TWICE by conv_first.hip: with BSY_K(n) = n and BSY_RELU = false it defines the kernel(s) as they always were -- identity and SiLU by
// `act`, instruction for instruction what they were before activation id 2 existed (tools/isa_diff.py) --, with BSY_K(n) = n##_relu and
// BSY_RELU = true the same text as <name>_relu, whose epilogue is ReLU whatever `act` says.  The launchers pick by `act == 2`.
// (No include guard, on purpose.)
template <typename T, int NT, int S, bool POOL>
__global__ __launch_bounds__(256) void BSY_K(conv_first_mfma_kernel)(const T* __restrict__ img, const half_t* __restrict__ wgt,
                                                              const float* __restrict__ bias, half_t* __restrict__ dst,
                                                              int H, int W, int OH, int OW, int ldd, int Cout, int act,
                                                              int tiles_x, int tiles_y) {
    constexpr bool RELU = BSY_RELU;
    static_assert((S == 1 || S == 2) && !(POOL && S != 1), "conv_first: stride 1 or 2; the pooling epilogue with stride 1");
    constexpr int CF_PR = CF_PR(S), CF_NG = CF_NG(S), CF_ROWPX = 4 * CF_NG;
    constexpr int OT = CF_TH * CF_TW * (32 * NT + 8);  // fp16 output tile of the coalesced epilogue
    constexpr int PT = CF_PR * CF_ROWPX * 4;
    constexpr int SM = PT > OT ? PT : OT;
    __shared__ __attribute__((aligned(16))) half_t stile[SM];
    half_t* patch = stile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lrow = lane & 31, lh = lane >> 5;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int n = bid / tiles_y;
    const int iy0 = ty * CF_TH * S - 1, ix0 = tx * CF_TW * S - 4;
    const T* ip = img + (size_t)n * 3 * H * W;
    const bool vec = !(W & 3) && !((uintptr_t)img & (4 * sizeof(T) - 1));
    for (int idx = tid; idx < CF_PR * CF_NG; idx += 256) {
        const int r = idx / CF_NG, j = idx - r * CF_NG;
        const ImgItem<T> it = vec ? img_item_load<T>(ip, H, W, iy0 + r, ix0 + 4 * j, true)
                                  : img_item_load_slow<T>(ip, H, W, iy0 + r, ix0 + 4 * j, true);
        img_item_park<T>(it, patch + (r * CF_ROWPX + 4 * j) * 4);
    }
    // weights: A operand, rows = output channels, [CoutPad][64] with k = (kh, kw, c4)
    half8 afr[NT][IMGC_KSUB];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int s = 0; s < IMGC_KSUB; ++s)
            afr[a][s] = *reinterpret_cast<const half8*>(wgt + (size_t)(a * 32 + lrow) * IMGC_KROW + 16 * s + 8 * lh);
    __syncthreads();

    f32x16 acc[NT][2];  // start at the bias of their couts (common.h acc_bias; the packed bias is padded to 128 values)
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc_bias(acc[a][b], bias + a * 32, lh);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        // output pixel (row `wave`, column x = 32 b + lrow): its window starts at patch pixel (S wave, S x + 3)
        const int win = ((S * wave) * CF_ROWPX + S * (b * 32 + lrow) + 3) * 4;
#pragma unroll
        for (int s = 0; s < IMGC_KSUB; ++s) {
            const half8 bf = img_frag<CF_ROWPX>(patch, win, s, lh);
#pragma unroll
            for (int a = 0; a < NT; ++a) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afr[a][s], bf, acc[a][b], 0, 0, 0);
        }
    }
    // epilogue: bias + SiLU -> fp16 tile [4 rows][64 px][32*NT ch] in LDS (the patch is dead), then coalesced 16-byte
    // stores: consecutive lanes write consecutive channels of one pixel, consecutive pixels are adjacent in NHWC
    __syncthreads();
    constexpr int CT = 32 * NT;       // channels in the tile
    constexpr int LDT = CT + 8;       // padded row (halves)
    half_t* tile = stile;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int prow = wave * CF_TW + b * 32 + lrow;
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = a * 32 + 8 * g + 4 * lh;
                half4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = acc[a][b][4 * g + e];
                    o[e] = (half_t)(RELU ? relu_f(t) : (act ? silu_f(t) : t));
                }
                *reinterpret_cast<half4*>(tile + prow * LDT + c) = o;
            }
    }
    __syncthreads();
    constexpr int CPRW = CT / 8;
    if (POOL) {  // OH x OW is the conv's extent (= H x W, even); dst is the (OH / 2) x (OW / 2) pooled map
        const int PH = OH >> 1, PW = OW >> 1;
        for (int id = tid; id < (CF_TH / 2) * (CF_TW / 2) * CPRW; id += 256) {
            const int pp = id / CPRW, cc = (id % CPRW) * 8;
            const int pr = pp / (CF_TW / 2), pc = pp % (CF_TW / 2);
            const int oy = ty * (CF_TH / 2) + pr, ox = tx * (CF_TW / 2) + pc;
            if (oy >= PH || ox >= PW || cc >= Cout) continue;
            const half_t* t0 = tile + ((2 * pr) * CF_TW + 2 * pc) * LDT + cc;
            *reinterpret_cast<half8*>(dst + ((size_t)(n * PH + oy) * PW + ox) * ldd + cc) =
                pool_max4<half_t>(*reinterpret_cast<const half8*>(t0), *reinterpret_cast<const half8*>(t0 + LDT),
                                  *reinterpret_cast<const half8*>(t0 + CF_TW * LDT), *reinterpret_cast<const half8*>(t0 + (CF_TW + 1) * LDT));
        }
        return;
    }
    for (int id = tid; id < CF_TH * CF_TW * CPRW; id += 256) {
        const int prow = id / CPRW, cc = (id % CPRW) * 8;
        const int oy = ty * CF_TH + prow / CF_TW, ox = tx * CF_TW + prow % CF_TW;
        if (oy >= OH || ox >= OW || cc >= Cout) continue;
        *reinterpret_cast<half8*>(dst + ((size_t)(n * OH + oy) * OW + ox) * ldd + cc) =
            *reinterpret_cast<const half8*>(tile + prow * LDT + cc);
    }
}
