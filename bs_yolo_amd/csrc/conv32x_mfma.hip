// Dense convolution of the "fp32x" engine mode: fp32 storage, fp32-class accuracy, fp16 matrix pipe.
//
// Replaces Conv.forward_fuse (nn/modules/conv.py:149-151) for fp32 callers at ~22 significant bits instead of the exact fp32
// chain of conv32_mfma.hip: every f32 operand is split into an f16 pair  v = hi + lo  (hi = f16(v), lo = f16(v - hi): v - hi is
// exact in f32, lo carries its leading 11 bits, so hi + lo reproduces v to ~2^-21 relative) and the product is taken as
//     w x  ~=  hi_w hi_x + hi_w lo_x + lo_w hi_x            (the dropped lo_w lo_x term is 2^-22 of the product)
// = THREE v_mfma_f32_32x32x16_f16 into ONE f32 accumulator tile per 16-deep K sub-step.  Products of two f16 values are exact in
// f32 and the pipe accumulates in f32, so what is lost against conv32_mfma is the 2^-21 representation error of the operands and the
// summation order -- far inside the north-star's 1e-3 (measured: tests/test_gpu_parity.py, fp32x cases).  Matrix-pipe roof:
// 2.5 PFLOP/s / 3 = 833 TFLOP/s of useful work against 157 TFLOP/s for v_mfma_f32_32x32x2_f32.
//
// Storage stays the fp32 mode's (NHWC f32 views, so every non-conv kernel of ref32.hip serves this mode unchanged); the split is
// done where it is cheapest:
//   weights : once, on the host (weights.py pack_record: two f16 planes [Cout][Kpad], K = (kh, kw, cin) padded to 32, behind the
//             f32 matrix the exact kernels read);
//   pixels  : in the staging path -- global_load_dwordx4 (f32) -> registers -> v_cvt_pkrtz_f16_f32 / subtract / convert ->
//             ds_write_b128 into an f16 hi tile and an f16 lo tile.  (Round-toward-zero for hi is as good as round-to-nearest here:
//             v - hi stays exact, lo picks up the difference; and it never produces an infinity from a finite input.)
// GEMM view as in conv32_mfma.hip: D[cout][pixel], A = weights (rows = cout), B = pixels => lane = pixel, registers = couts.
// Workgroup = 4 waves, tile 128 pixels x (64 NT | 32 THIN) couts, K-step 32; LDS rows of 32 halfs + 8 of padding (80 bytes: the
// 16 lanes of a ds_read_b128 group land on 16 distinct 16-byte bank slots).  Double-buffered stages, one barrier per K-step.
// The image conv (3 channels) and shapes this kernel does not take stay on the exact kernels (launch_conv32).
#include <stdlib.h>

#include "common.h"

namespace {
typedef __fp16 pk2_t __attribute__((ext_vector_type(2)));
union H8 {
    half8 h;
    pk2_t p[4];
    f32x4 f;
};

// 8 consecutive f32 (two 16-byte pieces) -> hi / lo f16 pieces
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, H8& hi, H8& lo) {
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        hi.p[j] = __builtin_amdgcn_cvt_pkrtz(v[2 * j], v[2 * j + 1]);
        const float r0 = v[2 * j] - (float)hi.p[j][0], r1 = v[2 * j + 1] - (float)hi.p[j][1];
        lo.p[j] = __builtin_amdgcn_cvt_pkrtz(r0, r1);
    }
}

// Epilogue of one 32-pixel block of a wave's accumulator tiles (lane = pixel, registers = couts) through a WAVE-PRIVATE LDS tile
// [32 pixels][NT * 32 + 4] floats: each lane parks its pixel's activated couts, then the wave reads the tile back row-wise, so that a
// store instruction writes whole rows (NT * 128 contiguous bytes per pixel, 64 / (NT * 8) pixels per instruction) instead of 32 pieces
// of 32 bytes, and the shortcut is read the same way.  The fp32 modes' 160 x 160 / 80 x 80 layers are HBM-bound (fp32 storage): the
// direct form ran them at ~75 % of a streaming copy.  (Round 4, measured: it pays on the image conv only, 406 -> 313 us -- a pixel's 32 couts
// are ONE 128-byte row there; on the other kernels the direct 32-byte pieces were already merged in L2 and the extra LDS round trip
// cost 0-8 %: they keep the direct form.)  No workgroup barrier: the tile belongs to one wave, whose LDS operations
// complete in issue order.  rowfn(r, pix, dp): source-geometry pixel index (shortcut) and destination pixel index of row r, false
// if the row lies outside the output.  Same arithmetic per element as the direct form (activation, then + shortcut).
template <int NT, int PB, typename RowFn>
__device__ __forceinline__ void epilogue_block(f32x16 (&acc)[NT][PB], const int b, float* wl, const int lane, const int cw0, const Conv32Args& a, RowFn rowfn) {
    constexpr int RS = NT * 32 + 4, PPR = NT * 8;
    const int lj = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int an = 0; an < NT; ++an)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = acc[an][b][4 * q + e];
                v[e] = act32(t, a.act, silu_rcp);
            }
            *reinterpret_cast<f32x4*>(wl + lj * RS + an * 32 + 8 * q + 4 * lh) = v;
        }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < NT * 4; ++j) {
        const int id = lane + 64 * j, r = id / PPR, c4 = (id % PPR) * 4, c = cw0 + c4;
        size_t pix = 0, dp = 0;
        if (rowfn(r, pix, dp) && c < a.Cout) {  // Cout % 4 == 0: a piece is inside or outside as a whole
            f32x4 v = *reinterpret_cast<const f32x4*>(wl + r * RS + c4);
            if (a.res) {
                const f32x4 rv = *reinterpret_cast<const f32x4*>(a.res + pix * a.ldr + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += rv[e];
            }
            *reinterpret_cast<f32x4*>(a.dst + dp * a.ldd + c) = v;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the rows are in registers before the next block overwrites the tile
}
#define CX_EPI_BYTES(NT_, WAVES_) ((WAVES_) * 32 * ((NT_) * 32 + 4) * 4)

template <int NT, bool THIN = false>
__global__ __launch_bounds__(256, 2) void conv32x_mfma_kernel(const Conv32Args a, const int M, const int ntn) {
    static_assert(!THIN || NT == 1, "thin tile: one 32-cout accumulator tile per wave");
    constexpr int TM = 128, TN = THIN ? 32 : 64 * NT, BK = 32, LDH = 40, PB = THIN ? 1 : 2;
    constexpr int WPIECES = TN * 4;                       // 16-byte pieces of one weight plane per K-step
    constexpr int WPT = (WPIECES + 255) / 256;            // per thread (the thin tile: threads 0..127 only)
    __shared__ __attribute__((aligned(16))) half_t sP[2][2][TM * LDH];  // [stage][hi | lo]
    __shared__ __attribute__((aligned(16))) half_t sW[2][2][TN * LDH];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = THIN ? wave : wave >> 1, wn = THIN ? 0 : wave & 1;
    const int prow0 = THIN ? wm * 32 : wm * 64;
    const int lj = lane & 31, lh = lane >> 5;
    const int tn_idx = blockIdx.x % ntn, tm_idx = blockIdx.x / ntn;
    const int m0 = tm_idx * TM, n0 = tn_idx * TN;
    const int Cin = a.C0 + a.C1, Cin8 = Cin >> 3;
    const int K = a.ks * a.ks * Cin, nk = (K + BK - 1) / BK;
    const int ohw = a.OH * a.OW;

    // ---- pixel items of this thread: pixels (tid >> 2) and (tid >> 2) + 64, 8-channel group (tid & 3) of every K-step ----
    const int gq = tid & 3;
    int pn[2], piy[2], pix_[2];
    bool pok[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int m = m0 + (tid >> 2) + 64 * it;
        pok[it] = m < M;
        const int mm = pok[it] ? m : 0;
        pn[it] = mm / ohw;
        const int rem = mm - pn[it] * ohw;
        const int oh = rem / a.OW;
        piy[it] = oh * a.stride - a.pad;
        pix_[it] = (rem - oh * a.OW) * a.stride - a.pad;
    }
    int tap = 0, c8 = gq, tkh = 0, tkw = 0;
    while (c8 >= Cin8) { c8 -= Cin8; ++tap; if (++tkw == a.ks) { tkw = 0; ++tkh; } }
    const int H0 = a.H >> a.up0, W0 = a.W >> a.up0, H1 = a.H >> a.up1, W1 = a.W >> a.up1;
    const bsy_rsrc_t rs0 = make_rsrc(a.src0, (unsigned)((((long long)a.B * H0 * W0 - 1) * a.ld0 + a.C0) * 4));
    const unsigned plane_bytes = (unsigned)a.Cout * (unsigned)a.wx_kpad * 2u;
    const bsy_rsrc_t rwh = make_rsrc(a.wx_hi, plane_bytes), rwl = make_rsrc(a.wx_lo, plane_bytes);

    f32x4 pv[2][2], wvh[WPT], wvl[WPT];
    auto load_step = [&](int kt) {
        const int kh = tkh, kw = tkw;
        const int c = c8 * 8;
        const bool s1 = c >= a.C0, kvalid = tap < a.ks * a.ks;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int iy = piy[it] + kh, ix = pix_[it] + kw;
            const bool ok = kvalid && pok[it] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            if (a.C1) {  // (uniform) two concat operands: the piece's source differs from lane to lane -> plain pointers
                pv[it][0] = f32x4{0.f, 0.f, 0.f, 0.f};
                pv[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (ok) {
                    const float* p = s1 ? reinterpret_cast<const float*>(a.src1) + ((size_t)(pn[it] * H1 + (iy >> a.up1)) * W1 + (ix >> a.up1)) * a.ld1 + (c - a.C0)
                                        : reinterpret_cast<const float*>(a.src0) + ((size_t)(pn[it] * H0 + (iy >> a.up0)) * W0 + (ix >> a.up0)) * a.ld0 + c;
                    pv[it][0] = *reinterpret_cast<const f32x4*>(p);
                    pv[it][1] = *reinterpret_cast<const f32x4*>(p + 4);
                }
            } else {
                const unsigned o0 = ok ? 4u * ((unsigned)((pn[it] * H0 + (iy >> a.up0)) * W0 + (ix >> a.up0)) * (unsigned)a.ld0 + (unsigned)c) : BSY_OOB_PAIR;
                pv[it][0] = buf_load16<f32x4>(rs0, o0);
                pv[it][1] = buf_load16<f32x4>(rs0, o0 + 16u);
            }
        }
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int id = tid + 256 * j;
            const int row = id >> 2, q = id & 3;  // cout row of the tile, 8-k piece of the K-step
            const bool ok = (WPIECES >= 256 || id < WPIECES) && n0 + row < a.Cout;  // k < Kpad always: the planes are padded to 32
            const unsigned off = ok ? 2u * ((unsigned)(n0 + row) * (unsigned)a.wx_kpad + (unsigned)(kt * BK + 8 * q)) : BSY_OOB_PAIR;
            wvh[j] = buf_load16<f32x4>(rwh, off);
            wvl[j] = buf_load16<f32x4>(rwl, off);
        }
        c8 += 4;
        while (c8 >= Cin8) { c8 -= Cin8; ++tap; if (++tkw == a.ks) { tkw = 0; ++tkh; } }
    };
    auto store_step = [&](int st) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            H8 hi, lo;
            split8(pv[it][0], pv[it][1], hi, lo);
            const int o = ((tid >> 2) + 64 * it) * LDH + 8 * gq;
            *reinterpret_cast<half8*>(&sP[st][0][o]) = hi.h;
            *reinterpret_cast<half8*>(&sP[st][1][o]) = lo.h;
        }
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int id = tid + 256 * j;
            if (WPIECES >= 256 || id < WPIECES) {
                const int o = (id >> 2) * LDH + 8 * (id & 3);
                H8 t;
                t.f = wvh[j];
                *reinterpret_cast<half8*>(&sW[st][0][o]) = t.h;
                t.f = wvl[j];
                *reinterpret_cast<half8*>(&sW[st][1][o]) = t.h;
            }
        }
    };

    // accumulators start at the bias, as in every conv kernel of the library
    f32x16 acc[NT][PB];
#pragma unroll
    for (int an = 0; an < NT; ++an)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = n0 + (wn * NT + an) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const float bv = c < a.Cout ? a.bias[c] : 0.f;
#pragma unroll
            for (int b = 0; b < PB; ++b) acc[an][b][r] = bv;
        }

    load_step(0);
    store_step(0);
    if (nk > 1) load_step(1);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int st = kt & 1;
        // step kt + 1 goes to LDS before this step's MFMAs (its loads are a step old; stage st ^ 1 was last read in step kt - 1), the
        // loads of step kt + 2 fly during them: split, ds_writes and MFMAs share one block for the scheduler to interleave
        if (kt + 1 < nk) store_step(st ^ 1);
        if (kt + 2 < nk) load_step(kt + 2);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            half8 bh[PB], bl[PB], ah[NT], al[NT];
#pragma unroll
            for (int b = 0; b < PB; ++b) {
                const int o = (prow0 + b * 32 + lj) * LDH + 16 * s + 8 * lh;
                bh[b] = *reinterpret_cast<const half8*>(&sP[st][0][o]);
                bl[b] = *reinterpret_cast<const half8*>(&sP[st][1][o]);
            }
#pragma unroll
            for (int an = 0; an < NT; ++an) {
                const int o = ((wn * NT + an) * 32 + lj) * LDH + 16 * s + 8 * lh;
                ah[an] = *reinterpret_cast<const half8*>(&sW[st][0][o]);
                al[an] = *reinterpret_cast<const half8*>(&sW[st][1][o]);
            }
#pragma unroll
            for (int an = 0; an < NT; ++an)
#pragma unroll
                for (int b = 0; b < PB; ++b) {
                    acc[an][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[an], bh[b], acc[an][b], 0, 0, 0);
                    acc[an][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[an], bl[b], acc[an][b], 0, 0, 0);
                    acc[an][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[an], bh[b], acc[an][b], 0, 0, 0);
                }
        }
        __syncthreads();
    }

    // ---- epilogue: lane = pixel, registers 4 q .. 4 q + 3 = couts 8 q + 4 lh + {0..3} of the 32-cout tile ----
#pragma unroll
    for (int b = 0; b < PB; ++b) {
        const int m = m0 + prow0 + b * 32 + lj;
        if (m >= M) continue;
        const int n = m / ohw, rem = m - n * ohw, oh = rem / a.OW, ow = rem - oh * a.OW;
        const size_t pix = (size_t)(n * a.OH + oh) * a.OW + ow;
        size_t dp = pix;
        if (a.dst_scale != 1)
            dp = ((size_t)n * (a.OH * a.dst_scale) + (oh * a.dst_scale + a.dst_dy)) * (size_t)(a.OW * a.dst_scale) + (ow * a.dst_scale + a.dst_dx);
#pragma unroll
        for (int an = 0; an < NT; ++an)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = n0 + (wn * NT + an) * 32 + 8 * q + 4 * lh;
                if (c >= a.Cout) continue;  // Cout % 4 == 0: a group of four is inside or outside as a whole
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = acc[an][b][4 * q + e];
                    v[e] = act32(t, a.act, silu_rcp);
                }
                if (a.res) {
                    const f32x4 rv = *reinterpret_cast<const f32x4*>(a.res + pix * a.ldr + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += rv[e];
                }
                *reinterpret_cast<f32x4*>(a.dst + dp * a.ldd + c) = v;
            }
    }
}

// ---- big tiles (round 4): 256 pixels x (256 | 128) couts, 8 waves, one workgroup per CU -------------------------------------
// The 128 x 128 tile above stages (128 + 128) x 4 bytes per k for 2 x 128 x 128 FLOP = 31 KB per MFLOP, and the layers that carry
// the FLOPs run at the rate a CU takes bytes in from L2 / Infinity Cache (~12.5 B/clk: 207-217 TFLOP/s on model.3 / model.5).
// 256 x 256 stages 15.6 KB per MFLOP, 256 x 128 23 KB.  Same arithmetic, same staging path (f32 pixels split in registers, f16
// weight planes through registers), K-step BK (16: 48-byte LDS rows; 32: 80-byte rows), two LDS stages + the staging registers.
template <int TN, int BK>
__global__ __launch_bounds__(512, 2) void conv32x_big_kernel(const Conv32Args a, const int M, const int ntn) {
    static_assert((TN == 256 || TN == 128) && (BK == 16 || BK == 32), "tile");
    constexpr int TM = 256, LDH = BK + 8, CPR = BK / 8, NST = 2;
    constexpr int PPT = TM * CPR / 512;        // pixel pieces (8 consecutive k of one pixel) per thread per K-step
    constexpr int WPT = TN * CPR / 512;        // weight pieces per thread per plane (TN 128, BK 16: threads 0..255 only)
    constexpr int WPIECES = TN * CPR;
    constexpr int WPTR = WPT > 0 ? WPT : 1;
    constexpr int WN = TN / 64, WM = 8 / WN;   // wave grid: WM pixel rows x WN cout columns; wave tile (TM / WM) px x 64 couts
    constexpr int PB = TM / WM / 32, NT = 2;
    constexpr int STAGE = (TM + TN) * LDH;     // halves per plane per stage
    __shared__ __attribute__((aligned(16))) half_t sm[NST * 2 * STAGE];  // [stage][hi | lo][pixel rows, then weight rows]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int prow0 = wm * (TM / WM);
    const int lj = lane & 31, lh = lane >> 5;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);  // XCD-aware (common.h)
    const int tn_idx = wg % ntn, tm_idx = wg / ntn;
    const int m0 = tm_idx * TM, n0 = tn_idx * TN;
    const int Cin = a.C0 + a.C1, Cin8 = Cin >> 3;
    const int K = a.ks * a.ks * Cin, nk = (K + BK - 1) / BK;
    const int ohw = a.OH * a.OW;

    const int gq = tid % CPR;
    int pn[PPT], piy[PPT], pix_[PPT];
    bool pok[PPT];
#pragma unroll
    for (int it = 0; it < PPT; ++it) {
        const int m = m0 + tid / CPR + (512 / CPR) * it;
        pok[it] = m < M;
        const int mm = pok[it] ? m : 0;
        pn[it] = mm / ohw;
        const int rem = mm - pn[it] * ohw;
        const int oh = rem / a.OW;
        piy[it] = oh * a.stride - a.pad;
        pix_[it] = (rem - oh * a.OW) * a.stride - a.pad;
    }
    int tap = 0, c8 = gq, tkh = 0, tkw = 0;
    while (c8 >= Cin8) { c8 -= Cin8; ++tap; if (++tkw == a.ks) { tkw = 0; ++tkh; } }
    const int H0 = a.H >> a.up0, W0 = a.W >> a.up0, H1 = a.H >> a.up1, W1 = a.W >> a.up1;
    const bsy_rsrc_t rs0 = make_rsrc(a.src0, (unsigned)((((long long)a.B * H0 * W0 - 1) * a.ld0 + a.C0) * 4));
    const bsy_rsrc_t rs1 = make_rsrc(a.C1 ? a.src1 : a.src0, a.C1 ? (unsigned)((((long long)a.B * H1 * W1 - 1) * a.ld1 + a.C1) * 4) : 0u);
    const unsigned plane_bytes = (unsigned)a.Cout * (unsigned)a.wx_kpad * 2u;
    const bsy_rsrc_t rwh = make_rsrc(a.wx_hi, plane_bytes), rwl = make_rsrc(a.wx_lo, plane_bytes);

    f32x4 pv[PPT][2], wvh[WPTR], wvl[WPTR];
    auto load_step = [&](int kt) {
        const int c = c8 * 8;
        const bool s1 = c >= a.C0, kvalid = tap < a.ks * a.ks;
#pragma unroll
        for (int it = 0; it < PPT; ++it) {
            const int iy = piy[it] + tkh, ix = pix_[it] + tkw;
            const bool ok = kvalid && pok[it] && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            // two concat operands: the piece's source differs from lane to lane -> one load from each descriptor, the other out of range
            const unsigned o0 = (ok && !s1) ? 4u * ((unsigned)((pn[it] * H0 + (iy >> a.up0)) * W0 + (ix >> a.up0)) * (unsigned)a.ld0 + (unsigned)c) : BSY_OOB_PAIR;
            pv[it][0] = buf_load16<f32x4>(rs0, o0);
            pv[it][1] = buf_load16<f32x4>(rs0, o0 + 16u);
            if (a.C1) {  // uniform
                const unsigned o1 = (ok && s1) ? 4u * ((unsigned)((pn[it] * H1 + (iy >> a.up1)) * W1 + (ix >> a.up1)) * (unsigned)a.ld1 + (unsigned)(c - a.C0)) : BSY_OOB_PAIR;
                const f32x4 q0 = buf_load16<f32x4>(rs1, o1), q1 = buf_load16<f32x4>(rs1, o1 + 16u);
                if (s1) { pv[it][0] = q0; pv[it][1] = q1; }
            }
        }
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int id = tid + 512 * j;
            const int row = id / CPR, q = id % CPR;
            const bool ok = n0 + row < a.Cout;
            const unsigned off = ok ? 2u * ((unsigned)(n0 + row) * (unsigned)a.wx_kpad + (unsigned)(kt * BK + 8 * q)) : BSY_OOB_PAIR;
            wvh[j] = buf_load16<f32x4>(rwh, off);
            wvl[j] = buf_load16<f32x4>(rwl, off);
        }
        if (WPT == 0) {  // TN 128, BK 16: 256 pieces per plane
            const int row = tid / CPR, q = tid % CPR;
            const bool ok = tid < WPIECES && n0 + row < a.Cout;
            const unsigned off = ok ? 2u * ((unsigned)(n0 + row) * (unsigned)a.wx_kpad + (unsigned)(kt * BK + 8 * q)) : BSY_OOB_PAIR;
            wvh[0] = buf_load16<f32x4>(rwh, off);
            wvl[0] = buf_load16<f32x4>(rwl, off);
        }
        c8 += CPR;
        while (c8 >= Cin8) { c8 -= Cin8; ++tap; if (++tkw == a.ks) { tkw = 0; ++tkh; } }
    };
    auto store_step = [&](int st) {
        half_t* hi_p = sm + (size_t)st * 2 * STAGE;
        half_t* lo_p = hi_p + STAGE;
#pragma unroll
        for (int it = 0; it < PPT; ++it) {
            H8 hi, lo;
            split8(pv[it][0], pv[it][1], hi, lo);
            const int o = (tid / CPR + (512 / CPR) * it) * LDH + 8 * gq;
            *reinterpret_cast<half8*>(hi_p + o) = hi.h;
            *reinterpret_cast<half8*>(lo_p + o) = lo.h;
        }
#pragma unroll
        for (int j = 0; j < WPTR; ++j) {
            const int id = tid + 512 * j;
            if (WPT > 0 || id < WPIECES) {
                const int o = (TM + id / CPR) * LDH + 8 * (id % CPR);
                H8 t;
                t.f = wvh[j];
                *reinterpret_cast<half8*>(hi_p + o) = t.h;
                t.f = wvl[j];
                *reinterpret_cast<half8*>(lo_p + o) = t.h;
            }
        }
    };

    f32x16 acc[NT][PB];
#pragma unroll
    for (int an = 0; an < NT; ++an)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = n0 + (wn * NT + an) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const float bv = c < a.Cout ? a.bias[c] : 0.f;
#pragma unroll
            for (int b = 0; b < PB; ++b) acc[an][b][r] = bv;
        }

    load_step(0);
    store_step(0);
    if (nk > 1) load_step(1);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int st = kt & 1;
        // Step kt + 1 goes to LDS BEFORE this step's MFMAs: its loads were issued a whole step ago, the stage it overwrites was last
        // read in step kt - 1 (behind that step's barrier), and the split's VALU work and ds_writes sit in one block with the MFMAs, so
        // the scheduler interleaves them instead of leaving the matrix pipe idle behind a store phase; the loads of step kt + 2 fly
        // during the MFMAs (the registers are the third stage).
        if (kt + 1 < nk) store_step(st ^ 1);
        if (kt + 2 < nk) load_step(kt + 2);
        const half_t* hi_p = sm + (size_t)st * 2 * STAGE;
        const half_t* lo_p = hi_p + STAGE;
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
            half8 ah[NT], al[NT];
#pragma unroll
            for (int an = 0; an < NT; ++an) {
                const int o = (TM + (wn * NT + an) * 32 + lj) * LDH + 16 * s + 8 * lh;
                ah[an] = *reinterpret_cast<const half8*>(hi_p + o);
                al[an] = *reinterpret_cast<const half8*>(lo_p + o);
            }
#pragma unroll
            for (int b = 0; b < PB; ++b) {
                const int o = (prow0 + b * 32 + lj) * LDH + 16 * s + 8 * lh;
                const half8 bh = *reinterpret_cast<const half8*>(hi_p + o);
                const half8 bl = *reinterpret_cast<const half8*>(lo_p + o);
#pragma unroll
                for (int an = 0; an < NT; ++an) {
                    acc[an][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[an], bh, acc[an][b], 0, 0, 0);
                    acc[an][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[an], bl, acc[an][b], 0, 0, 0);
                    acc[an][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[an], bh, acc[an][b], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int b = 0; b < PB; ++b) {
        const int m = m0 + prow0 + b * 32 + lj;
        if (m >= M) continue;
        const int n = m / ohw, rem = m - n * ohw, oh = rem / a.OW, ow = rem - oh * a.OW;
        const size_t pix = (size_t)(n * a.OH + oh) * a.OW + ow;
        size_t dp = pix;
        if (a.dst_scale != 1)
            dp = ((size_t)n * (a.OH * a.dst_scale) + (oh * a.dst_scale + a.dst_dy)) * (size_t)(a.OW * a.dst_scale) + (ow * a.dst_scale + a.dst_dx);
#pragma unroll
        for (int an = 0; an < NT; ++an)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = n0 + (wn * NT + an) * 32 + 8 * q + 4 * lh;
                if (c >= a.Cout) continue;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = acc[an][b][4 * q + e];
                    v[e] = act32(t, a.act, silu_rcp);
                }
                if (a.res) {
                    const f32x4 rv = *reinterpret_cast<const f32x4*>(a.res + pix * a.ldr + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += rv[e];
                }
                *reinterpret_cast<f32x4*>(a.dst + dp * a.ldd + c) = v;
            }
    }
}

// ---- patch kernel (round 4): 3 x 3, stride 1, one source -----------------------------------------------------------------------
// The implicit-GEMM kernels above fetch AND split every input pixel once per tap (nine times); thin layers (Cout <= 64 at 80 x 80 /
// 160 x 160: the Bottlenecks inside C3k2, Detect's box branch) were bound by exactly that -- 47 KB staged per MFLOP.  Here the 10 x 18
// input patch of an 8 x 16 output tile is fetched and split ONCE per CK-channel chunk into an f16 hi / lo patch in LDS and serves all
// nine taps (a tap = a shifted window of the patch: the B fragment of pixel (y, x) for tap (kh, kw) is patch row (y + kh) * 18 + x + kw);
// only the weights -- TPS taps x TN couts x CK per step, both planes -- stream through a double-buffered stage.  K walks chunk-major:
// (chunk, kh, kw, channel in chunk).  CK = 32 (Cin % 32 == 0) or 16; TN = 128 / 64 (wave grid 2 x 2) or 32 (4 x 1).
// TW = 16: 8 x 16 output tile; TW = 20: 6 x 20 (120 of the 128 MFMA pixel slots) for maps whose width is a multiple of 20 and not of 16
// -- a 20 x 20 map is 4 such tiles (83 % of their area inside the map) instead of 6 tiles of 8 x 16 (52 %).
template <int NT, bool THIN, int CK, int TPS, int TW>
__global__ __launch_bounds__(256, 2) void conv32x_patch_kernel(const Conv32Args a, const int tiles_y, const int tiles_x, const int ntn) {
    static_assert((CK == 16 || CK == 32) && (TPS == 1 || TPS == 3) && (!THIN || NT == 1) && (TW == 16 || TW == 20), "configuration");
    constexpr int TH = TW == 16 ? 8 : 6, PH = TH + 2, PW = TW + 2, NPP = PH * PW;  // 180 / 176 patch pixels
    constexpr int TN = THIN ? 32 : 64 * NT, LDH = CK + 8, CPR = CK / 8, PB = THIN ? 1 : 2, KS = CK / 16;
    constexpr int PPT = (NPP * CPR + 255) / 256;          // patch pieces per thread
    constexpr int WPIECES = TPS * TN * CPR;               // weight pieces per plane per step
    constexpr int WPT = (WPIECES + 255) / 256;
    constexpr int NSTEP = 9 / TPS;                        // steps per chunk
    __shared__ __attribute__((aligned(16))) half_t sPat[2][NPP * LDH];           // [hi | lo]
    __shared__ __attribute__((aligned(16))) half_t sWt[2][2][TPS * TN * LDH];    // [stage][hi | lo][tap][cout][k]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = THIN ? wave : wave >> 1, wn = THIN ? 0 : wave & 1;
    const int prow0 = THIN ? wm * 32 : wm * 64;
    const int lj = lane & 31, lh = lane >> 5;
    const int nb = gridDim.x, bq = nb >> 3, br = nb & 7, bx = blockIdx.x & 7;
    const int wg = (bx < br ? bx * (bq + 1) : br * (bq + 1) + (bx - br) * bq) + (blockIdx.x >> 3);
    const int tn_idx = wg % ntn;
    int t = wg / ntn;
    const int txi = t % tiles_x; t /= tiles_x;
    const int tyi = t % tiles_y;
    const int img = t / tiles_y;
    const int y0 = tyi * TH, x0 = txi * TW, n0 = tn_idx * TN;
    const int Cin = a.C0, nchunk = Cin / CK;
    const bsy_rsrc_t rs0 = make_rsrc(a.src0, (unsigned)((((long long)a.B * a.H * a.W - 1) * a.ld0 + a.C0) * 4));
    const unsigned plane_bytes = (unsigned)a.Cout * (unsigned)a.wx_kpad * 2u;
    const bsy_rsrc_t rwh = make_rsrc(a.wx_hi, plane_bytes), rwl = make_rsrc(a.wx_lo, plane_bytes);

    // patch pieces of this thread: piece id -> (patch pixel, 8-channel group); offset of the pixel in the source (or out of range)
    unsigned poff[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int id = tid + 256 * j, pp = id / CPR, q = id % CPR;
        const int iy = y0 - 1 + pp / PW, ix = x0 - 1 + pp % PW;
        const bool ok = pp < NPP && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        poff[j] = ok ? 4u * ((unsigned)((img * a.H + iy) * a.W + ix) * (unsigned)a.ld0 + 8u * q) : BSY_OOB_PAIR;
    }
    f32x4 pv[PPT][2], wvh[WPT], wvl[WPT];
    auto load_patch = [&](int c) {
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const unsigned o = poff[j] == BSY_OOB_PAIR ? BSY_OOB_PAIR : poff[j] + 4u * (unsigned)(c * CK);
            pv[j][0] = buf_load16<f32x4>(rs0, o);
            pv[j][1] = buf_load16<f32x4>(rs0, o + 16u);
        }
    };
    auto store_patch = [&]() {
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int id = tid + 256 * j;
            if (id < NPP * CPR) {
                H8 hi, lo;
                split8(pv[j][0], pv[j][1], hi, lo);
                const int o = (id / CPR) * LDH + 8 * (id % CPR);
                *reinterpret_cast<half8*>(&sPat[0][o]) = hi.h;
                *reinterpret_cast<half8*>(&sPat[1][o]) = lo.h;
            }
        }
    };
    // weights of step g = chunk * NSTEP + j: taps TPS j .. TPS j + TPS - 1 of the chunk, k = tap * Cin + chunk * CK + ..
    auto load_w = [&](int g) {
        const int c = g / NSTEP, tap0 = (g % NSTEP) * TPS;
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int id = tid + 256 * j;
            const int q = id % CPR, row = (id / CPR) % TN, tp = id / (CPR * TN);
            const bool ok = id < WPIECES && n0 + row < a.Cout;
            const unsigned off = ok ? 2u * ((unsigned)(n0 + row) * (unsigned)a.wx_kpad + (unsigned)((tap0 + tp) * Cin + c * CK + 8 * q)) : BSY_OOB_PAIR;
            wvh[j] = buf_load16<f32x4>(rwh, off);
            wvl[j] = buf_load16<f32x4>(rwl, off);
        }
    };
    auto store_w = [&](int st) {
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int id = tid + 256 * j;
            if (id < WPIECES) {
                const int o = (id / CPR) * LDH + 8 * (id % CPR);  // row = tap * TN + cout
                H8 t2;
                t2.f = wvh[j];
                *reinterpret_cast<half8*>(&sWt[st][0][o]) = t2.h;
                t2.f = wvl[j];
                *reinterpret_cast<half8*>(&sWt[st][1][o]) = t2.h;
            }
        }
    };

    f32x16 acc[NT][PB];
#pragma unroll
    for (int an = 0; an < NT; ++an)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = n0 + (wn * NT + an) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const float bv = c < a.Cout ? a.bias[c] : 0.f;
#pragma unroll
            for (int b = 0; b < PB; ++b) acc[an][b][r] = bv;
        }
    // patch row (pixel index) of this lane's pixel of block b for tap (0, 0): (y + kh) * PW + x + kw is added per tap
    int prow[PB];
#pragma unroll
    for (int b = 0; b < PB; ++b) {
        const int p = prow0 + b * 32 + lj;
        prow[b] = p < TH * TW ? (p / TW) * PW + p % TW : 0;  // (6 x 20: slots 120..127 compute on pixel 0 and are not stored)
    }

    const int nsteps = nchunk * NSTEP;
    load_patch(0);
    load_w(0);
    store_w(0);
    if (nsteps > 1) load_w(1);
    int g = 0;
    for (int c = 0; c < nchunk; ++c) {
        store_patch();            // (every wave is done with the previous chunk's patch: the barrier that ended its last step)
        if (c + 1 < nchunk) load_patch(c + 1);  // in flight during this chunk's nine taps
        __syncthreads();
        for (int j = 0; j < NSTEP; ++j, ++g) {
            const int st = g & 1;
            if (g + 1 < nsteps) store_w(st ^ 1);
            if (g + 2 < nsteps) load_w(g + 2);
#pragma unroll
            for (int tp = 0; tp < TPS; ++tp) {
                const int tap = j * TPS + tp, kh = tap / 3, kw = tap - 3 * kh;
                const int shift = kh * PW + kw;
#pragma unroll
                for (int s2 = 0; s2 < KS; ++s2) {
                    half8 ah[NT], al[NT];
#pragma unroll
                    for (int an = 0; an < NT; ++an) {
                        const int o = (tp * TN + (wn * NT + an) * 32 + lj) * LDH + 16 * s2 + 8 * lh;
                        ah[an] = *reinterpret_cast<const half8*>(&sWt[st][0][o]);
                        al[an] = *reinterpret_cast<const half8*>(&sWt[st][1][o]);
                    }
#pragma unroll
                    for (int b = 0; b < PB; ++b) {
                        const int o = (prow[b] + shift) * LDH + 16 * s2 + 8 * lh;
                        const half8 bh = *reinterpret_cast<const half8*>(&sPat[0][o]);
                        const half8 bl = *reinterpret_cast<const half8*>(&sPat[1][o]);
#pragma unroll
                        for (int an = 0; an < NT; ++an) {
                            acc[an][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[an], bh, acc[an][b], 0, 0, 0);
                            acc[an][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[an], bl, acc[an][b], 0, 0, 0);
                            acc[an][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[an], bh, acc[an][b], 0, 0, 0);
                        }
                    }
                }
            }
            __syncthreads();
        }
    }

#pragma unroll
    for (int b = 0; b < PB; ++b) {
        const int p = prow0 + b * 32 + lj;
        const int oy = y0 + p / TW, ox = x0 + p % TW;
        if (p >= TH * TW || oy >= a.H || ox >= a.W) continue;
        const size_t pix = (size_t)(img * a.H + oy) * a.W + ox;
#pragma unroll
        for (int an = 0; an < NT; ++an)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = n0 + (wn * NT + an) * 32 + 8 * q + 4 * lh;
                if (c >= a.Cout) continue;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float tt = acc[an][b][4 * q + e];
                    v[e] = act32(tt, a.act, silu_rcp);
                }
                if (a.res) {
                    const f32x4 rv = *reinterpret_cast<const f32x4*>(a.res + pix * a.ldr + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += rv[e];
                }
                *reinterpret_cast<f32x4*>(a.dst + pix * a.ldd + c) = v;
            }
    }
}

template <int NT, bool THIN, int TPS>
int launch_patch(const Conv32Args& a, hipStream_t s) {
    const bool w20 = a.W % 20 == 0 && a.W % 16 != 0;
    const int ty = ceil_div(a.H, w20 ? 6 : 8), tx = ceil_div(a.W, w20 ? 20 : 16), ntn = ceil_div(a.Cout, THIN ? 32 : 64 * NT);
    const long long nb = (long long)a.B * ty * tx * ntn;
    if (nb > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "conv32x_patch: grid out of range");
    const dim3 grid((unsigned)nb), blk(256);
    if (a.C0 % 32 == 0) {
        if (w20) hipLaunchKernelGGL((conv32x_patch_kernel<NT, THIN, 32, TPS, 20>), grid, blk, 0, s, a, ty, tx, ntn);
        else hipLaunchKernelGGL((conv32x_patch_kernel<NT, THIN, 32, TPS, 16>), grid, blk, 0, s, a, ty, tx, ntn);
    } else {
        if (w20) hipLaunchKernelGGL((conv32x_patch_kernel<NT, THIN, 16, TPS, 20>), grid, blk, 0, s, a, ty, tx, ntn);
        else hipLaunchKernelGGL((conv32x_patch_kernel<NT, THIN, 16, TPS, 16>), grid, blk, 0, s, a, ty, tx, ntn);
    }
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

// ---- image conv (round 4): BCHW image (f16 / f32, 3 channels), 3 x 3, stride 1 or 2 -> NHWC f32 --------------------------------
// K = (kh, kw, c) = 27, padded to 32 with zeros: ONE K-step of two 16-deep sub-steps, so no loop and no ring -- a workgroup gathers
// the 27 taps of its 128 output pixels straight from the three image planes (thread = (pixel, half of the K range)), splits them, and
// every wave multiplies its 32 pixels with all NT 32-cout tiles of the layer (weights: the layer's two planes [Cout][32] parked in
// LDS).  HBM-bound by design: B x 3 x H x W in, B x OH x OW x Cout x 4 bytes out (0.84 GB for YOLO11s at 64 x 640 x 640; the exact
// kernel took 0.63 ms over it on the fp32 matrix pipe).
template <int NT, typename TI>
__global__ __launch_bounds__(256) void conv32x_first_kernel(const Conv32Args a, const int M) {
    constexpr int TM = 128, LDH = 40;
    struct Stages {
        half_t sP[2][TM * LDH];
        half_t sW[2][NT * 32 * LDH];
    };
    constexpr int EPI = CX_EPI_BYTES(1, 4), SMEM = (int)sizeof(Stages) > EPI ? (int)sizeof(Stages) : EPI;  // epilogue: one 32-cout tile at a time
    __shared__ __attribute__((aligned(16))) unsigned char smem_raw[SMEM];
    auto& sP = reinterpret_cast<Stages*>(smem_raw)->sP;
    auto& sW = reinterpret_cast<Stages*>(smem_raw)->sW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lj = lane & 31, lh = lane >> 5;
    const int m0 = blockIdx.x * TM;
    const int ohw = a.OH * a.OW;
    // weights: NT * 32 rows x 4 pieces per plane
    for (int id = tid; id < NT * 32 * 4; id += 256) {
        const int row = id >> 2, q = id & 3;
        H8 h, l;
        h.f = f32x4{0.f, 0.f, 0.f, 0.f};
        l.f = h.f;
        if (row < a.Cout) {
            h.f = *reinterpret_cast<const f32x4*>(a.wx_hi + (size_t)row * a.wx_kpad + 8 * q);
            l.f = *reinterpret_cast<const f32x4*>(a.wx_lo + (size_t)row * a.wx_kpad + 8 * q);
        }
        *reinterpret_cast<half8*>(&sW[0][row * LDH + 8 * q]) = h.h;
        *reinterpret_cast<half8*>(&sW[1][row * LDH + 8 * q]) = l.h;
    }
    {   // pixels: thread = (pixel tid >> 1, k half tid & 1): k = 16 half .. 16 half + 15, k = (kh * 3 + kw) * 3 + c
        const int pl = tid >> 1, k0 = 16 * (tid & 1);
        const int m = m0 + pl;
        const bool pok = m < M;
        const int mm = pok ? m : 0;
        const int n = mm / ohw, rem = mm - n * ohw, oh = rem / a.OW, ow = rem - oh * a.OW;
        const int iy0 = oh * a.stride - a.pad, ix0 = ow * a.stride - a.pad;
        const size_t hw = (size_t)a.H * a.W;
        const TI* img = reinterpret_cast<const TI*>(a.src0) + (size_t)n * 3 * hw;
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = k0 + j, tap = k / 3, c = k - 3 * tap, kh = tap / 3, kw = tap - 3 * kh;
            const int iy = iy0 + kh, ix = ix0 + kw;
            v[j] = (pok && k < 27 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) ? (float)img[(size_t)c * hw + (size_t)iy * a.W + ix] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            H8 hi, lo;
            split8(f32x4{v[8 * g], v[8 * g + 1], v[8 * g + 2], v[8 * g + 3]}, f32x4{v[8 * g + 4], v[8 * g + 5], v[8 * g + 6], v[8 * g + 7]}, hi, lo);
            *reinterpret_cast<half8*>(&sP[0][pl * LDH + k0 + 8 * g]) = hi.h;
            *reinterpret_cast<half8*>(&sP[1][pl * LDH + k0 + 8 * g]) = lo.h;
        }
    }
    __syncthreads();
    f32x16 acc[NT];
#pragma unroll
    for (int an = 0; an < NT; ++an)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = an * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            acc[an][r] = c < a.Cout ? a.bias[c] : 0.f;
        }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        const int o = (wave * 32 + lj) * LDH + 16 * s2 + 8 * lh;
        const half8 bh = *reinterpret_cast<const half8*>(&sP[0][o]);
        const half8 bl = *reinterpret_cast<const half8*>(&sP[1][o]);
#pragma unroll
        for (int an = 0; an < NT; ++an) {
            const int ow_ = (an * 32 + lj) * LDH + 16 * s2 + 8 * lh;
            const half8 ah = *reinterpret_cast<const half8*>(&sW[0][ow_]);
            const half8 al = *reinterpret_cast<const half8*>(&sW[1][ow_]);
            acc[an] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[an], 0, 0, 0);
            acc[an] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[an], 0, 0, 0);
            acc[an] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[an], 0, 0, 0);
        }
    }
    __syncthreads();  // every wave has read its fragments: the stages become the waves' output tiles
    // one 32-cout tile at a time through the wave's LDS tile [32 pixels][36]: a pixel's Cout floats are contiguous in the output, so a
    // store instruction then writes 8 pixels x 128 bytes instead of 32 pieces of 32 bytes
    float* wl = reinterpret_cast<float*>(smem_raw) + wave * 32 * 36;
    const int mb = m0 + wave * 32;
#pragma unroll
    for (int an = 0; an < NT; ++an) {
        f32x16 one[1][1] = {{acc[an]}};
        epilogue_block<1, 1>(one, 0, wl, lane, an * 32, a, [&](int r, size_t& pix, size_t& dp) {
            if (mb + r >= M) return false;
            pix = dp = (size_t)(mb + r);
            return true;
        });
    }
}

template <typename TI>
int launch_first(const Conv32Args& a, int M, hipStream_t s) {
    const dim3 grid((unsigned)ceil_div(M, 128));
    switch (ceil_div(a.Cout, 32)) {
        case 1: hipLaunchKernelGGL((conv32x_first_kernel<1, TI>), grid, dim3(256), 0, s, a, M); break;
        case 2: hipLaunchKernelGGL((conv32x_first_kernel<2, TI>), grid, dim3(256), 0, s, a, M); break;
        case 3: hipLaunchKernelGGL((conv32x_first_kernel<3, TI>), grid, dim3(256), 0, s, a, M); break;
        default: hipLaunchKernelGGL((conv32x_first_kernel<4, TI>), grid, dim3(256), 0, s, a, M); break;
    }
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
}  // namespace

bool conv32x_mfma_supported(const Conv32Args& a) {
    if (!a.wx_hi || !a.wx_lo || a.wx_kpad <= 0 || (a.wx_kpad & 31)) return false;
    if (a.first)  // the image conv: 3 x 3 over 3 channels (K = 27 -> one 32-deep step), up to 128 couts, NHWC f32 output in 16-byte pieces
        return a.ks == 3 && a.C0 == 3 && !a.C1 && !a.up0 && a.wx_kpad == 32 && a.Cout > 0 && a.Cout <= 128 && !(a.Cout & 3) && !(a.ldd & 3) && !a.res &&
               a.dst_scale == 1 && (a.src_dtype == BSY_F16 || a.src_dtype == BSY_F32) && !(((uintptr_t)a.wx_hi | (uintptr_t)a.wx_lo | (uintptr_t)a.dst) & 15);
    if (!conv32_mfma_supported(a)) return false;  // the same view / alignment rules as the exact MFMA kernel
    if (((uintptr_t)a.wx_hi | (uintptr_t)a.wx_lo) & 15) return false;
    if (a.wx_kpad < a.ks * a.ks * (a.C0 + a.C1)) return false;
    if ((long long)a.Cout * a.wx_kpad * 2 >= 0xFFFFFFC0LL) return false;
    return true;
}

int launch_conv32x_mfma(const Conv32Args& a, hipStream_t s) {
    if (!conv32x_mfma_supported(a)) BSY_FAIL(BSY_ERR_ARG, "conv32x_mfma: unsupported shape / alignment");
    const long long M = (long long)a.B * a.OH * a.OW;
    if (M <= 0 || M > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "conv32x_mfma: M out of range");
    if (a.first) return a.src_dtype == BSY_F16 ? launch_first<half_t>(a, (int)M, s) : launch_first<float>(a, (int)M, s);
    // tile choice (BSY_CONV32X_TILE=0 / 1 / 2 forces the 128-pixel tiles / 256 x 128 / 256 x 256 where they apply; _BK=16 / 32):
    // 256 x 256 from 256 couts and 256 x 128 from 128, when the grid still gives every CU a workgroup or the layer is deep enough
    // that staged bytes, not tile quantisation, set its time
    const char* ef = getenv("BSY_CONV32X_TILE");   // (read per call: the tests switch it between launches)
    const char* eb = getenv("BSY_CONV32X_BK");
    const char* ep = getenv("BSY_CONV32X_PATCH");
    const int force = ef ? atoi(ef) : -1, bk = eb ? atoi(eb) : 32;
    // 3 x 3 stride-1 layers with one source: the patch kernel (faster than the implicit-GEMM tiles on every such layer of the YOLO
    // graphs, 20 x 20 maps included: cv2.2.0 166 -> 105 us with 8 x 16 tiles at 52 % fill; 6 x 20 tiles since).  BSY_CONV32X_PATCH=0
    // switches it off (tests / A-B).
    const bool patch_ok = a.ks == 3 && a.stride == 1 && a.pad == 1 && !a.C1 && !a.up0 && a.dst_scale == 1 && a.C0 % 16 == 0 && a.OH == a.H && a.OW == a.W;
    if (patch_ok && force < 0 && (ep ? atoi(ep) != 0 : true)) {
        if (a.Cout > 64) return launch_patch<2, false, 1>(a, s);
        if (a.Cout > 32) return launch_patch<1, false, 1>(a, s);
        return launch_patch<1, true, 3>(a, s);
    }
    int big = 0;
    const long long ptiles = (M + 255) / 256;
    if (a.Cout >= 256 && ptiles * ceil_div(a.Cout, 256) >= 128) big = 2;
    else if (a.Cout >= 128 && ptiles * ceil_div(a.Cout, 128) >= 128) big = 1;
    if (force >= 0) big = force == 2 ? (a.Cout >= 256 ? 2 : (a.Cout >= 128 ? 1 : 0)) : (force == 1 ? (a.Cout >= 128 ? 1 : 0) : 0);
    if (big) {
        const int tn = big == 2 ? 256 : 128, ntn_b = ceil_div(a.Cout, tn);
        const long long nb = (long long)ceil_div((int)M, 256) * ntn_b;
        if (nb > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "conv32x_mfma: grid out of range");
        if (big == 2 && bk == 16) hipLaunchKernelGGL((conv32x_big_kernel<256, 16>), dim3((unsigned)nb), dim3(512), 0, s, a, (int)M, ntn_b);
        else if (big == 2) hipLaunchKernelGGL((conv32x_big_kernel<256, 32>), dim3((unsigned)nb), dim3(512), 0, s, a, (int)M, ntn_b);
        else if (bk == 16) hipLaunchKernelGGL((conv32x_big_kernel<128, 16>), dim3((unsigned)nb), dim3(512), 0, s, a, (int)M, ntn_b);
        else hipLaunchKernelGGL((conv32x_big_kernel<128, 32>), dim3((unsigned)nb), dim3(512), 0, s, a, (int)M, ntn_b);
        HIP_TRY(hipGetLastError());
        return BSY_OK;
    }
    const bool wide = a.Cout > 64, thin = a.Cout <= 32;
    const int ntn = ceil_div(a.Cout, wide ? 128 : (thin ? 32 : 64));
    const long long nblk = (long long)ceil_div((int)M, 128) * ntn;
    if (nblk > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "conv32x_mfma: grid out of range");
    if (thin) hipLaunchKernelGGL((conv32x_mfma_kernel<1, true>), dim3((unsigned)nblk), dim3(256), 0, s, a, (int)M, ntn);
    else if (wide) hipLaunchKernelGGL((conv32x_mfma_kernel<2>), dim3((unsigned)nblk), dim3(256), 0, s, a, (int)M, ntn);
    else hipLaunchKernelGGL((conv32x_mfma_kernel<1>), dim3((unsigned)nblk), dim3(256), 0, s, a, (int)M, ntn);
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
