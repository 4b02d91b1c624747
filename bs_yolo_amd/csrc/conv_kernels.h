#pragma once
// What the fp16 conv translation units share -- header only: the library is not built with relocatable device code, so no
// __device__ variable crosses a unit (the zero page of the generic implicit-GEMM variant is file-local in conv_gemm.hip).
//   conv_select.hip    (host only) packed dims, conv_korder, the configuration table kConvCfgs, conv_cfg_valid, conv_candidates,
//                      launch_conv: fills a ConvK and hands it to the family launcher of the chosen id
//   conv_gemm.hip      conv_mfma_kernel (implicit GEMM, ksize 1 / 3), splitk_reduce_kernel; launch_gemm_cfg
//   conv_stream1x1.hip conv1x1_persist_kernel, conv1x1_wres_kernel (streaming 1x1 layers); launch_stream1x1_cfg
//   conv_patch.hip     conv3x3_patch_kernel (+ box-branch tail); launch_patch_cfg
//   dwpw_fused.hip     a different op (BSY_OP_DWPW): borrows dma16_buf only
// From here: ConvK (the kernels' argument block), the LDS-DMA wrappers, the epilogues of the implicit-GEMM kernel and the DFL
// decoder the patch kernel's tail shares with them (all templates / __forceinline__), the family launchers' declarations.
#include "common.h"

struct ConvK {
    const half_t* src0;
    const half_t* src1;
    int ld0, ld1, C0, C1, up0, up1;
    int H, W, OH, OW, stride, pad;
    int M;            // B*OH*OW
    int Cin8;         // (C0+C1)/8
    int ntaps;        // ks*ks
    int nk;           // Kpad/32 (informational; the kernel uses Kpad / BK)
    int Kpad;
    const half_t* wgt;
    const float* bias;
    void* dst;
    int ldd, Cout, out_f32;
    const half_t* res;
    int ldr;
    int act;
    int dst_scale, dst_dy, dst_dx;
    int ntn;  // number of cout tiles
    int ntm;  // number of pixel tiles (streaming 1x1 kernels)
    int tiles_x, tiles_y, B;  // patch kernel: 8 x 16 output tiles per image
    int epi, y_f32, A, a0, nrows, raw_f32, rawC;  // fused Detect decoder (ConvArgs::epi)
    float lvl_stride;
    int xyxy;  // box rows as corners (ConvArgs::xyxy)
    void* y;
    void* raw;
    const half_t* tail_wgt;  // box-branch tail (ConvArgs::tail_wgt): packed [128][64] 1x1 weights, f32 bias
    const float* tail_bias;
    unsigned span0, span1, wspan;  // bytes addressable from src0 / src1 / wgt (buffer-descriptor num_records)
    // Split-K (latency mode, round 4; implicit-GEMM kernel, ALIGNED variants): the K walk is cut into nsl_c x nsl_t slices -- slice
    // (sc, st) sums channels [sc * cb_per, (sc + 1) * cb_per) of taps [st * taps_per, (st + 1) * taps_per) in the layer's own order --
    // each computed by its own workgroups of ONE launch into an f32 slab of split_ws ([slice][pixel][ldw] raw sums; the bias enters in
    // slice 0); splitk_reduce_kernel adds the slabs in slice order and applies activation / shortcut.  nsl_c * nsl_t <= 1: off.
    int nsl_c, nsl_t, cb_per, taps_per, ldw;
    float* split_ws;
    long long slab;   // floats per slice
    int korder;  // the layer's K walk (conv_select.hip conv_korder: a function of the layer's SHAPE, never of the configuration): 0 = the packed
                 // order (taps outer, channels inner), 1 = chunk-major with 32-channel chunks (32 channels of all ntaps taps, then
                 // the next 32), 2 = chunk-major with 64-channel chunks (a BK-32 kernel visits the two halves of a chunk tap by tap).
                 // Chunk-major: a stride-2 3x3 tile re-reads its input lines within ntaps K-steps -- from the XCD's L2 -- instead
                 // of once per tap, Cin / BK K-steps apart; and it is the order the patch kernel sums in.
};

// 16-byte LDS-DMA: the wave's 64 lanes land at lds_wave_base + 16*lane (lds_wave_base must be wave-uniform).
// Guarded so that the host pass (which only needs the launch stub) never type-checks the LDS address-space builtin.
__device__ __forceinline__ void dma16(const void* g, half_t* lds_wave_base) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_global_load_lds(g, lds_wave_base, 16, 0, 0);
#else
    (void)g;
    (void)lds_wave_base;
#endif
}

// Same through a buffer descriptor: address = base(rsrc) + voff + soff, lanes whose voff is out of range (>= num_records)
// write ZEROS to LDS -- that is how padded taps / rows past M / K padding are filled, with no zero page and no 64-bit
// per-lane pointer arithmetic (the scalar K-step displacement rides in soff).
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void dma16_buf(bsy_rsrc_t r, unsigned voff, unsigned soff, half_t* lds_wave_base) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, lds_wave_base, 16, (int)voff, (int)soff, 0, 0);
}
#else
__device__ __forceinline__ void dma16_buf(bsy_rsrc_t, unsigned, unsigned, half_t*) {}
#endif

template <int MT, int NT, bool RELU = false>
__device__ __forceinline__ void conv_epilogue(const ConvK& p, f32x16 (&acc)[NT][MT], int m0, int n0, int wm, int wn,
                                              int lrow, int lh) {
    const int ohw = p.OH * p.OW;
    const bool wide = !p.out_f32 && !(p.Cout & 15) && !(p.ldd & 7) && !((uintptr_t)p.dst & 15);
#pragma unroll
    for (int b = 0; b < MT; ++b) {
        const int m = m0 + (wm * MT + b) * 32 + lrow;
        const bool mvalid = m < p.M;
        size_t dpix = (size_t)(mvalid ? m : 0);
        if (p.dst_scale != 1) {
            const int mm = mvalid ? m : 0;
            const int n = mm / ohw;
            const int rem = mm - n * ohw;
            const int oh = rem / p.OW;
            const int ow = rem - oh * p.OW;
            dpix = ((size_t)n * (p.OH * p.dst_scale) + (oh * p.dst_scale + p.dst_dy)) * (size_t)(p.OW * p.dst_scale) +
                   (ow * p.dst_scale + p.dst_dx);
        }
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const int cbase = n0 + (wn * NT + a) * 32;
            if (cbase >= p.Cout) continue;  // wave-uniform
            if (wide) {
                // all 32 couts of this MFMA tile exist (Cout % 16 == 0 and cbase + 16 <= Cout; second half checked below)
                unsigned pk[4][2];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = cbase + 8 * g + 4 * lh;
                    float v[4] = {0.f, 0.f, 0.f, 0.f};
                    if (c < p.Cout) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float t = acc[a][b][4 * g + e];  // (the accumulators started at the bias)
                            v[e] = RELU ? relu_f(t) : (p.act ? silu_f(t) : t);
                        }
                        if (p.res && mvalid) {
                            const half4 rv = *reinterpret_cast<const half4*>(p.res + dpix * p.ldr + c);
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
                        }
                    }
                    half2v h0 = {(half_t)v[0], (half_t)v[1]}, h1 = {(half_t)v[2], (half_t)v[3]};
                    pk[g][0] = __builtin_bit_cast(unsigned, h0);
                    pk[g][1] = __builtin_bit_cast(unsigned, h1);
                }
#pragma unroll
                for (int g = 0; g < 4; g += 2) {
                    // lanes l / l+32 hold couts 8g+{0..3} / 8g+{4..7}: swap so each lane owns 8 consecutive couts
                    const auto r0 = __builtin_amdgcn_permlane32_swap(pk[g][0], pk[g + 1][0], false, false);
                    const auto r1 = __builtin_amdgcn_permlane32_swap(pk[g][1], pk[g + 1][1], false, false);
                    const int c = cbase + 8 * (g + lh);
                    if (mvalid && c < p.Cout) {
                        uint4 o = {r0[0], r1[0], r0[1], r1[1]};
                        *reinterpret_cast<uint4*>(reinterpret_cast<half_t*>(p.dst) + dpix * p.ldd + c) = o;
                    }
                }
                continue;
            }
            if (!mvalid) continue;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = cbase + 8 * g + 4 * lh;
                if (c >= p.Cout) continue;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = acc[a][b][4 * g + e];
                    if constexpr (RELU) t = relu_f(t);
                    else if (p.act) t = silu_f(t);
                    v[e] = t;
                }
                const bool full = c + 3 < p.Cout;
                if (p.res) {
                    const half_t* rp = p.res + dpix * p.ldr + c;
                    if (full) {
                        const half4 rv = *reinterpret_cast<const half4*>(rp);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (c + e < p.Cout) v[e] += (float)rp[e];
                    }
                }
                if (p.out_f32) {
                    float* dp = reinterpret_cast<float*>(p.dst) + dpix * p.ldd + c;
                    if (full) {
                        f32x4 o = {v[0], v[1], v[2], v[3]};
                        *reinterpret_cast<f32x4*>(dp) = o;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (c + e < p.Cout) dp[e] = v[e];
                    }
                } else {
                    half_t* dp = reinterpret_cast<half_t*>(p.dst) + dpix * p.ldd + c;
                    if (full) {
                        half4 o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
                        *reinterpret_cast<half4*>(dp) = o;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (c + e < p.Cout) dp[e] = (half_t)v[e];
                    }
                }
            }
        }
    }
}

// Fused Detect decoder (ConvArgs::epi): the last conv of a head branch turns its accumulators straight into rows of the
// prediction tensor y (B, 4 + nc, A) -- what Detect._inference (head.py:113-148) computes from the concatenated logit
// maps -- instead of storing f32 logits for a separate decode kernel to read back (0.3 GB per batch of 64, and the
// decode launch itself).  In the accumulator layout a lane owns ONE pixel (= anchor), so for a fixed register the 32
// lanes of a half-wave write 32 consecutive anchors of one y row: coalesced without staging.
//   epi 2 (class logits): sigmoid, rows 4 + c.
//   epi 3 (box logits, 4 sides x 16 DFL bins = 64 couts in one wave: WAVES_N == 1, NT == 2): a side's 16 bins sit in
//          8 registers of this lane and 8 of lane ^ 32 -> softmax expectation with three cross-lane exchanges, then
//          dist2bbox (xywh; xyxy where ConvK::xyxy is set) * stride, rows 0..3.
// The raw logits go to the level's raw map (B, 64 + nc, h, w) when the caller bound one.
template <typename T>
__device__ __forceinline__ void head_store(void* base, size_t idx, float v) { reinterpret_cast<T*>(base)[idx] = (T)v; }

// DFL + dist2bbox of one pixel per lane pair (head.py:141-146, block.py:58-77): lo / hi = the 32 x 32 accumulators of couts 0..31 /
// 32..63 of this lane's pixel; side sd's 16 bins sit in 8 registers of this lane and 8 of lane ^ 32.  Writes rows 0..3 of y (and the
// raw logits when a raw map is bound).
__device__ __forceinline__ void dfl_decode_store(const ConvK& p, const f32x16& lo, const f32x16& hi, bool mv,
                                                 size_t ybase, size_t rbase, int pix, int lh) {
    const int hw = p.OH * p.OW;
    float dist[4];
#pragma unroll
    for (int sd = 0; sd < 4; ++sd) {
        const int rb = 8 * (sd & 1);
        float v[8];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * g + e] = ((sd >> 1) ? hi : lo)[rb + 4 * g + e];  // logits incl. bias (accumulator start)
        if (p.raw && mv) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const size_t ri = rbase + (size_t)(16 * sd + (i & 3) + 8 * (i >> 2) + 4 * lh) * hw;
                if (p.raw_f32) head_store<float>(p.raw, ri, v[i]); else head_store<half_t>(p.raw, ri, v[i]);
            }
        }
        float mx = v[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) mx = fmaxf(mx, v[i]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float den = 0.f, num = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float ex = __expf(v[i] - mx);
            den += ex;
            num += ex * (float)((i & 3) + 8 * (i >> 2) + 4 * lh);  // bin index of this register
        }
        den += __shfl_xor(den, 32, 64);
        num += __shfl_xor(num, 32, 64);
        dist[sd] = num / den;
    }
    if (mv && lh == 0) {
        const int ay_i = pix / p.OW, ax_i = pix - ay_i * p.OW;
        const float ax = (float)ax_i + 0.5f, ay = (float)ay_i + 0.5f;
        const float x1 = ax - dist[0], y1 = ay - dist[1], x2 = ax + dist[2], y2 = ay + dist[3];
        // xyxy (an end2end head): (anchor - lt) * stride, (anchor + rb) * stride, as tal.py:385-395 with xywh=False then head.py:129
        const float o[4] = {(p.xyxy ? x1 : (x1 + x2) * 0.5f) * p.lvl_stride, (p.xyxy ? y1 : (y1 + y2) * 0.5f) * p.lvl_stride,
                            (p.xyxy ? x2 : x2 - x1) * p.lvl_stride, (p.xyxy ? y2 : y2 - y1) * p.lvl_stride};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t yi = ybase + (size_t)r * p.A;
            if (p.y_f32) head_store<float>(p.y, yi, o[r]); else head_store<half_t>(p.y, yi, o[r]);
        }
    }
}

template <int MT, int NT>
__device__ __forceinline__ void conv_epilogue_head(const ConvK& p, f32x16 (&acc)[NT][MT], int m0, int n0, int wm, int wn,
                                                   int lrow, int lh) {
    const int hw = p.OH * p.OW;
#pragma unroll
    for (int b = 0; b < MT; ++b) {
        const int m = m0 + (wm * MT + b) * 32 + lrow;
        const bool mv = m < p.M;
        const int mm = mv ? m : 0;
        const int n = mm / hw, pix = mm - n * hw;
        const size_t ybase = (size_t)n * p.nrows * p.A + p.a0 + pix;
        const size_t rbase = (size_t)n * p.rawC * hw + pix;
        if (p.epi == 2) {
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                const int cl = n0 + (wn * NT + a) * 32;
                if (cl >= p.Cout) continue;  // wave-uniform
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c0 = cl + 8 * g + 4 * lh;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = c0 + e;
                        if (!mv || c >= p.Cout) continue;
                        const float v = acc[a][b][4 * g + e];
                        const float sg = sigmoid_f(v);
                        const size_t yi = ybase + (size_t)(4 + c) * p.A;
                        if (p.y_f32) head_store<float>(p.y, yi, sg); else head_store<half_t>(p.y, yi, sg);
                        if (p.raw) {
                            const size_t ri = rbase + (size_t)(64 + c) * hw;
                            if (p.raw_f32) head_store<float>(p.raw, ri, v); else head_store<half_t>(p.raw, ri, v);
                        }
                    }
                }
            }
        } else if (NT == 2) {  // epi 3; host guarantees WAVES_N == 1, n0 == 0, Cout == 64
            dfl_decode_store(p, acc[0][b], acc[NT - 1][b], mv, ybase, rbase, pix, lh);
        }
    }
}

// Class-score epilogue through LDS (f16 y, no raw map requested): the direct form above writes 64-byte pieces (32 lanes x
// one f16 anchor) -- the class conv of the 80 x 80 level ran at 2.6 TB/s.  Here sigmoid(logit) is parked transposed,
// [cout][TM + 8] f16, and leaves as 16-byte pieces of 8 consecutive anchors of one y row (falling back to single
// elements for a piece that straddles two images or starts on an odd boundary).
template <int TM, int TN, int MT, int NT, int NTHR>
__device__ __forceinline__ void conv_epilogue_cls_lds(const ConvK& p, f32x16 (&acc)[NT][MT], half_t* stile, int m0, int n0,
                                                      int wm, int wn, int lrow, int lh, int tid) {
    constexpr int LDP = TM + 8;  // padded row of the transposed tile (halves)
#pragma unroll
    for (int b = 0; b < MT; ++b) {
        const int prow = (wm * MT + b) * 32 + lrow;
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const int cl = (wn * NT + a) * 32;
            if (n0 + cl >= p.Cout) continue;  // wave-uniform; bias is padded to CoutPad only
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = cl + 8 * g + 4 * lh;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = acc[a][b][4 * g + e];
                    stile[(c + e) * LDP + prow] = (half_t)sigmoid_f(v);
                }
            }
        }
    }
    __syncthreads();
    const int hw = p.OH * p.OW;
    half_t* y = reinterpret_cast<half_t*>(p.y);
    constexpr int GPR = TM / 8;  // 8-anchor pieces per cout row
    for (int id = tid; id < TN * GPR; id += NTHR) {
        const int cr = id / GPR, g8 = (id - cr * GPR) * 8;
        const int c = n0 + cr, m = m0 + g8;
        if (c >= p.Cout || m >= p.M) continue;
        const int n = m / hw, pix = m - n * hw;
        const size_t yi = ((size_t)n * p.nrows + 4 + c) * p.A + p.a0 + pix;
        if (pix + 8 <= hw && m + 8 <= p.M && !(yi & 7)) {
            *reinterpret_cast<half8*>(y + yi) = *reinterpret_cast<const half8*>(stile + cr * LDP + g8);
        } else {
            for (int e = 0; e < 8 && m + e < p.M; ++e) {
                const int me = m + e, ne = me / hw, pe = me - ne * hw;
                y[((size_t)ne * p.nrows + 4 + c) * p.A + p.a0 + pe] = stile[cr * LDP + g8 + e];
            }
        }
    }
}

// Coalesced epilogue (fp16 outputs, Cout % 8 == 0): the accumulator layout (lane = pixel, 4 channels per register
// group) makes every direct store touch 32 different pixel rows; for the HBM-bound 1x1 layers that store pattern was
// the whole kernel (3x).  Instead: bias + SiLU in registers -> fp16 tile [TM][TN] in LDS (the DMA ring is free after
// the K loop) -> every thread moves 16-byte pieces with consecutive lanes on consecutive channels of one pixel row,
// adding the residual (also read coalesced) on the way.
template <int TM, int TN, int MT, int NT, int NTHR, bool RELU = false>
__device__ __forceinline__ void conv_epilogue_lds(const ConvK& p, f32x16 (&acc)[NT][MT], half_t* stile, int m0, int n0,
                                                  int wm, int wn, int lrow, int lh, int tid) {
    constexpr int LDT = TN + 8;  // padded tile row (halves)
#pragma unroll
    for (int b = 0; b < MT; ++b) {
        const int prow = (wm * MT + b) * 32 + lrow;
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const int cl = (wn * NT + a) * 32;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = cl + 8 * g + 4 * lh;
                half4 o;
                f32x4 t = f32x4{acc[a][b][4 * g], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]};
                if constexpr (RELU) t = relu4_f(t);
                else if (p.act) t = silu4_f(t);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (half_t)t[e];
                *reinterpret_cast<half4*>(stile + prow * LDT + c) = o;
            }
        }
    }
    __syncthreads();
    constexpr int CPRW = TN / 8;                 // 16-byte pieces per tile row
    constexpr int ITER = TM * CPRW / NTHR;
    half_t* dst = reinterpret_cast<half_t*>(p.dst);
#pragma unroll
    for (int i = 0; i < ITER; ++i) {
        const int id = tid + NTHR * i;
        const int row = id / CPRW, cc = (id % CPRW) * 8;
        const int m = m0 + row, c = n0 + cc;
        if (m >= p.M || c >= p.Cout) continue;
        half8 v = *reinterpret_cast<const half8*>(stile + row * LDT + cc);
        if (p.res) {
            const half8 r = *reinterpret_cast<const half8*>(p.res + (size_t)m * p.ldr + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] + (float)r[e]);
        }
        *reinterpret_cast<half8*>(dst + (size_t)m * p.ldd + c) = v;
    }
}

// Family launchers: `id` is a row id of kConvCfgs (conv_select.hip) without the chunk-major bit.  Each unit switches over the ids IT
// instantiates; an id it does not know is BSY_ERR_ARG (the configuration sweep of tests/test_gpu_parity.py meets it then).
int launch_gemm_cfg(int id, int ksize, const ConvK& k, hipStream_t s);
int launch_stream1x1_cfg(int id, const ConvK& k, hipStream_t s);
int launch_patch_cfg(int id, bool tail, const ConvK& k, hipStream_t s);

constexpr int PERSIST_MAX_COUT = 1024;  // persistent 1x1 kernel: the whole bias vector stays in LDS (conv_cfg_valid checks it)
