// Attention core of C2PSA for gfx950: out = softmax(q^T k * scale) applied to v, per (image, head), optionally + pe(v).
//
// Replaces the matmul/softmax/matmul lines of Attention.forward (nn/modules/block.py:4279-4286):
//     attn = (q.transpose(-2,-1) @ k) * scale ; attn = attn.softmax(-1) ; x = v @ attn.transpose(-2,-1)
// and, with pe weights, the `+ self.pe(v)` of :4286 (depthwise 3x3 + bias on v, no activation).
// The reference materialises the (B, heads, N, N) matrix in HBM; here it never leaves registers (flash-style online
// softmax).  qkv is NHWC fp16 with the channel order [q(all heads) | k(all heads) | v(all heads)] (the host permutes
// the rows of the qkv 1x1-conv weight accordingly, bs_yolo_amd/weights.py), so v is a plain channel slice for `pe`.
//
// A wave owns 32 queries and walks all keys in tiles of 32.  Both products run on v_mfma_f32_32x32x16_f16 with the QUERY on the
// lane:
//     S^T[key][q]  = sum_c K[key][c] Q[q][c]     A = K rows (LDS), B = Q (registers, loaded once per query block)
//     O^T[d][q]   += sum_key V^T[d][key] P^T[key][q]   A = V^T, B = P^T = the S^T accumulator itself converted to fp16
// (guide: "an accumulator tile as the next MFMA's operand": element j of lane half h of k-step s is key 16s + 8(j>>2) + 4h + (j&3);
// the V^T fragment is read in the same permuted order).  V lies in LDS as it lies in HBM, [key][d], written with 16-byte stores;
// the V^T fragment comes out of it with the transposing read ds_read_b64_tr_b16 (4 keys x 16 channels per 16-lane group).
// Row statistics are per lane; the two lane halves of a query exchange their tile maximum and tile row sum (v_permlane32_swap).
//
// Two forms of the same tile step:
//   resident  (N <= attn_res_rows): one workgroup of 8 waves (4 at head_dim > 64) stages ALL keys of its (image, head) once, one barrier, then its waves
//             loop over 32-query blocks with no barrier inside.  A 20 x 20 map is 13 blocks: no padding of N to 128, K / V fetched
//             once per head instead of once per 128 queries.  With few (image, head) pairs the query blocks of a head are dealt to
//             several workgroups (each stages the head again); a query's arithmetic does not depend on who computes it.
//   streaming (larger N): 4 waves = 128 queries, key chunks of 128 through two LDS buffers, the next chunk fetched into registers
//             while the current one is multiplied: one barrier per 128 keys.
//
// pe epilogue: after normalisation a lane holds 4-channel groups of its query's output.  It rounds them to fp16 (what the unfused
// path stores), then evaluates dwconv3x3_kernel<false, true> (elementwise.hip) for those channels at its own pixel: accumulator =
// bias, taps in that kernel's order (for kw: top, mid, bot), one v_fma_mix_f32 per tap with zeros for taps outside the map, result
// f16(acc + f32(att)) with the sum rounded to f32 first -- the same bits as the two launches.  v around the pixel comes from the
// resident LDS image, or from global memory / L2 in the streaming form.
#include <type_traits>

#include "common.h"

// V image: row `key` holds HD halves; its 64-byte (32-channel) chunks are XOR-swizzled by the key so that the four rows a
// transposing read touches per lane half fall into four different 64-byte bank groups of the 256-byte bank period
// (HD = 32 / 96: rows 64 / 192 bytes apart do that already).  Swizzle bits come from key & 3 only -> a lane constant in the tile loop.
template <int HD>
__device__ __forceinline__ int v_off(int key, int d) {
    const int swz = HD == 64 ? ((key >> 1) & 1) : HD == 128 ? (key & 3) : 0;
    return key * HD + ((((d >> 5) ^ swz)) << 5) + (d & 31);
}

__device__ __forceinline__ half4 lds_read_tr(const half_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __fp16 fp16x4 __attribute__((__vector_size__(8)));
    typedef fp16x4 __attribute__((address_space(3))) * lds_ptr;
    const fp16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_ptr)p);
    half4 r;
    __builtin_memcpy(&r, &t, 8);
    return r;
#else
    return half4{};
#endif
}

// max / sum of x with the other lane half's (lane ^ 32) value: v_permlane32_swap instead of a trip through LDS (ds_bpermute)
__device__ __forceinline__ void swap_halves(float x, float& lo, float& hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned u = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);  // r[0]: lanes 0-31 of x in both halves, r[1]: lanes 32-63
    lo = __builtin_bit_cast(float, (unsigned)r[0]);
    hi = __builtin_bit_cast(float, (unsigned)r[1]);
#else
    lo = hi = x;
#endif
}

// keys the resident form can hold: 128 KB of the CU's 160 KB, at most 512 rows (K rows are KD + 8 halves: 16 x odd bytes, conflict-free
// 16-byte reads), a multiple of the 32-key tile
constexpr int attn_res_rows(int kd, int hd) {
    const int r = (128 * 1024 / ((kd + 8 + hd) * 2)) & ~31;
    return r < 512 ? r : 512;
}
// waves per workgroup: 8 in the resident form (two per SIMD: one wave's softmax under the other's MFMAs) while the accumulators of two
// waves fit a SIMD's registers (head_dim <= 64), else 4
constexpr int attn_waves(int hd, bool res) { return res && hd <= 64 ? 8 : 4; }
#define ATTN_CHUNK 128  // keys per LDS buffer of the streaming form

struct AttnKArgs {
    const half_t* qkv;
    half_t* out;
    const float* pe_w;  // [9][heads * HD] or null
    const float* pe_b;
    int ld, ldo, N, heads, W;
    float scale;
};

// KD = key_dim (channels of q and k per head), HD = head_dim (channels of v per head).  The stock scales give 32 / 64 (block.py:4253-4258:
// num_heads = dim // 64, key_dim = head_dim / 2); other width multiples give other pairs (0.1875: one head of 48 / 96) -- instantiated for
// KD in {16, 32, 48, 64} and HD in {32, 64, 96, 128}.
template <int KD, int HD, bool RES>
__global__ __launch_bounds__(attn_waves(HD, RES) * 64) void attention_kernel(const AttnKArgs p) {
    constexpr int NW = attn_waves(HD, RES), NT = NW * 64;
    constexpr int KS = KD / 16, DT = HD / 32, NCK = KD / 8, NCV = HD / 8, KLD = KD + 8;
    constexpr int ROWS = RES ? attn_res_rows(KD, HD) : ATTN_CHUNK;
    constexpr int BUF = ROWS * (KLD + HD);  // halves: [ROWS][KLD] K rows, then the V image
    static_assert(KD % 16 == 0 && KD <= 64 && HD % 32 == 0 && HD <= 128, "head shape");
    __shared__ __attribute__((aligned(16))) half_t lds[(RES ? 1 : 2) * BUF];
    __shared__ __attribute__((aligned(16))) float sPE[10 * HD];  // this head's pe weights [9][HD] and bias [HD]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 31, lh = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int N = p.N, ld = p.ld;
    const int qoff = head * KD, koff = p.heads * KD + head * KD, voff = p.heads * 2 * KD + head * HD;
    const half_t* base = p.qkv + (size_t)b * N * ld;
    const float scale = p.scale;
    constexpr float LOG2E = 1.4426950408889634f;
    const int ntiles = (N + 31) / 32, nfull = N / 32;
    const half8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};

    if (p.pe_w)  // (visible after the first barrier of either form)
        for (int i = tid; i < 10 * HD; i += NT)
            sPE[i] = i < 9 * HD ? p.pe_w[(i / HD) * (p.heads * HD) + head * HD + i % HD] : p.pe_b[head * HD + i - 9 * HD];

    // lane constants of the LDS reads: K row fragment, and the transposing read's address (lane 4q + p of a 16-lane group
    // supplies row q, columns 4p .. 4p + 3 of the group's 4-key x 16-channel block; it receives column (lane & 15) of the 4 rows)
    const int krd = lrow * KLD + 8 * lh;
    int vtr[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) vtr[dt] = v_off<HD>(4 * lh + ((lane >> 2) & 3), dt * 32 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3));

    half8 qf[KS];
    f32x16 o[DT];
    float m_run, l_run;  // running maximum of s * scale and row sum, both shared by the lane pair

    // one 32-key tile at rows kb .. kb + 31 of (sK, sV); k0 = its first key.  RAG: the tile holds keys >= N (last tile only).
    auto tile = [&](const half_t* sK, const half_t* sV, const int kb, const int k0, auto rag) {
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const half8 a = *reinterpret_cast<const half8*>(sK + kb * KLD + krd + 16 * ks);
            s = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qf[ks], s, 0, 0, 0);
        }
        // From here to the fp16 P the arithmetic is the kernel's of before, operation for operation (s * scale, the difference to the
        // maximum, times log2 e, v_exp_f32; row sum in key order, the two lane halves added per tile, l = fma(l, alpha, sum)): the forward
        // returns the bits it returned.  The empty asm keeps the product from contracting into the subtraction.
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] *= scale;
            asm("" : "+v"(s[r]));
        }
        if constexpr (decltype(rag)::value) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (k0 + (r & 3) + 8 * (r >> 2) + 4 * lh >= N) s[r] = -INFINITY;
        }
        float mt = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, s[r]);
        float mlo, mhi;
        swap_halves(mt, mlo, mhi);
        const float m_new = fmaxf(m_run, fmaxf(mlo, mhi));
        float alpha = 1.0f;
        if (__any(m_new > m_run)) {  // wave-uniform: where no lane's maximum moved every lane's factor is 2^0 = 1, exactly
            alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
            m_run = m_new;
        }
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f((s[r] - m_run) * LOG2E);
            rs += s[r];
        }
        float rlo, rhi;
        swap_halves(rs, rlo, rhi);
        l_run = __builtin_fmaf(l_run, alpha, rlo + rhi);
        // O^T += V^T P^T
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            half8 pb;
#pragma unroll
            for (int j = 0; j < 8; ++j) pb[j] = (half_t)s[8 * ks + j];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const half_t* vp = sV + (kb + 16 * ks) * HD + vtr[dt];
                const half4 v0 = lds_read_tr(vp), v1 = lds_read_tr(vp + 8 * HD);
                const half8 a = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pb, o[dt], 0, 0, 0);
            }
        }
    };
    const std::false_type full_tile;
    const std::true_type ragged_tile;

    auto begin_block = [&](const int qb) {
        const int q = qb * 32 + lrow;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            qf[ks] = q < N ? *reinterpret_cast<const half8*>(base + (size_t)q * ld + qoff + 16 * ks + 8 * lh) : z8;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
        m_run = -INFINITY;
        l_run = 0.f;
    };

    // normalise, (pe,) store.  sV: the resident V image (RES) -- the streaming form reads v from global memory.
    auto finish_block = [&](const int qb, const half_t* sV) {
        const int q = qb * 32 + lrow;
        if (q >= N) return;
        const float inv = 1.0f / l_run;
        half_t* op = p.out + ((size_t)b * N + q) * p.ldo + head * HD;
        const bool pe = p.pe_w != nullptr;
        // pe: the nine taps of this query's pixel -- row of v (clamped into the map, so every read is in bounds) and whether the tap
        // lies inside; a tap outside contributes fma(0, w, acc), as the depthwise kernel's zero-filled loads do
        int tn[9];
        bool tin[9];
        if (pe) {
            const int W = p.W, H = N / W, y = q / W, x = q - y * W;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
                tin[k] = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
                tn[k] = tin[k] ? yy * W + xx : q;
            }
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = dt * 32 + 8 * g + 4 * lh;
                half4 att;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = o[dt][4 * g + e] * inv;
                    asm("" : "+v"(t));  // the product rounds to f32, then to f16, in every instantiation
                    att[e] = (half_t)t;
                }
                if (pe) {
                    const f32x4 bs = *reinterpret_cast<const f32x4*>(sPE + 9 * HD + d);
                    float acc[4] = {bs[0], bs[1], bs[2], bs[3]};
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                        for (int kh = 0; kh < 3; ++kh) {
                            const int k = kh * 3 + kw;
                            union { half4 h; unsigned u[2]; } v;
                            v.h = RES ? *reinterpret_cast<const half4*>(sV + v_off<HD>(tn[k], d))
                                      : *reinterpret_cast<const half4*>(base + (size_t)tn[k] * ld + voff + d);
                            v.u[0] = tin[k] ? v.u[0] : 0u;
                            v.u[1] = tin[k] ? v.u[1] : 0u;
                            const f32x4 w = *reinterpret_cast<const f32x4*>(sPE + k * HD + d);
                            acc[0] = fma_mix_lo(v.u[0], w[0], acc[0]);
                            acc[1] = fma_mix_hi(v.u[0], w[1], acc[1]);
                            acc[2] = fma_mix_lo(v.u[1], w[2], acc[2]);
                            acc[3] = fma_mix_hi(v.u[1], w[3], acc[3]);
                        }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float t = acc[e] + (float)att[e];
                        asm("" : "+v"(t));  // f32 sum, then f16: dwconv3x3_kernel's two roundings (never one fused v_fma_mixlo_f16)
                        att[e] = (half_t)t;
                    }
                }
                *reinterpret_cast<half4*>(op + d) = att;
            }
    };

    if constexpr (RES) {
        half_t* sK = lds;
        half_t* sV = lds + ROWS * KLD;
        const int npad = ntiles * 32;  // <= ROWS (launcher); rows N .. npad - 1 are zeros
        // 16-byte pieces, K and V alike (piece < NCK of a row: K), 8 loads in flight per thread before their stores
        constexpr int NCR = NCK + NCV, U = 8;
        const int total = npad * NCR;
        for (int i0 = tid; i0 < total; i0 += NT * U) {
            half8 r[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int id = i0 + u * NT, key = id / NCR, ch = id % NCR;
                r[u] = (id < total && key < N) ? *reinterpret_cast<const half8*>(base + (size_t)key * ld + (ch < NCK ? koff + ch * 8 : voff + (ch - NCK) * 8)) : z8;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int id = i0 + u * NT, key = id / NCR, ch = id % NCR;
                if (id < total) *reinterpret_cast<half8*>(ch < NCK ? sK + key * KLD + ch * 8 : sV + v_off<HD>(key, (ch - NCK) * 8)) = r[u];
            }
        }
        __syncthreads();
        // the head's 32-query blocks, dealt round-robin to the waves of all workgroups of this (image, head)
        for (int qb = blockIdx.x * NW + wave; qb < ntiles; qb += gridDim.x * NW) {
            begin_block(qb);
            for (int t = 0; t < nfull; ++t) tile(sK, sV, t * 32, t * 32, full_tile);
            if (nfull < ntiles) tile(sK, sV, nfull * 32, nfull * 32, ragged_tile);
            finish_block(qb, sV);
        }
    } else {
        constexpr int PK = ATTN_CHUNK * NCK / NT, PV = ATTN_CHUNK * NCV / NT;  // 16-byte pieces per thread and chunk
        static_assert(PK * NT == ATTN_CHUNK * NCK && PV * NT == ATTN_CHUNK * NCV, "chunk staging");
        const int qb = blockIdx.x * NW + wave;  // may lie past the last block: the wave still stages and keeps the barriers
        begin_block(qb);
        half8 kreg[PK], vreg[PV];
        auto fetch = [&](const int k0) {
#pragma unroll
            for (int i = 0; i < PK; ++i) {
                const int id = tid + NT * i, key = k0 + id / NCK;
                kreg[i] = key < N ? *reinterpret_cast<const half8*>(base + (size_t)key * ld + koff + (id % NCK) * 8) : z8;
            }
#pragma unroll
            for (int i = 0; i < PV; ++i) {
                const int id = tid + NT * i, key = k0 + id / NCV;
                vreg[i] = key < N ? *reinterpret_cast<const half8*>(base + (size_t)key * ld + voff + (id % NCV) * 8) : z8;
            }
        };
        const int nchunks = (N + ATTN_CHUNK - 1) / ATTN_CHUNK;
        fetch(0);
        for (int ck = 0; ck < nchunks; ++ck) {
            half_t* sK = lds + (ck & 1) * BUF;
            half_t* sV = sK + ROWS * KLD;
            // buffer (ck & 1) was last read for chunk ck - 2; every wave finished that before it passed the barrier of chunk ck - 1
#pragma unroll
            for (int i = 0; i < PK; ++i) {
                const int id = tid + NT * i;
                *reinterpret_cast<half8*>(sK + (id / NCK) * KLD + (id % NCK) * 8) = kreg[i];
            }
#pragma unroll
            for (int i = 0; i < PV; ++i) {
                const int id = tid + NT * i;
                *reinterpret_cast<half8*>(sV + v_off<HD>(id / NCV, (id % NCV) * 8)) = vreg[i];
            }
            __syncthreads();
            if (ck + 1 < nchunks) fetch((ck + 1) * ATTN_CHUNK);  // in flight while this chunk is multiplied
            const int t0 = ck * (ATTN_CHUNK / 32);
            const int tend = min(t0 + ATTN_CHUNK / 32, ntiles), fend = min(tend, nfull);
            for (int t = t0; t < fend; ++t) tile(sK, sV, (t - t0) * 32, t * 32, full_tile);
            if (fend < tend) tile(sK, sV, (fend - t0) * 32, fend * 32, ragged_tile);
        }
        finish_block(qb, nullptr);
    }
}

bool attention_supported(int key_dim, int head_dim) {
    return key_dim > 0 && key_dim <= 64 && !(key_dim & 15) && head_dim > 0 && head_dim <= 128 && !(head_dim & 31);
}

// impl 0: resident where one head's keys fit LDS, else streaming; 1: resident (BSY_ERR_ARG where it does not fit); 2: streaming
int launch_attention(const AttnArgs& a, hipStream_t s, int impl) {
    if (!attention_supported(a.key_dim, a.head_dim))
        BSY_FAIL(BSY_ERR_ARG, "attention: key_dim must be 16 / 32 / 48 / 64 and head_dim 32 / 64 / 96 / 128 (got %d / %d)", a.key_dim, a.head_dim);
    if ((a.ld & 7) || (a.ldo & 3) || ((uintptr_t)a.qkv & 15) || ((uintptr_t)a.out & 7) || a.N <= 0 || a.heads <= 0 || a.B <= 0)
        BSY_FAIL(BSY_ERR_ARG, "attention: bad layout");
    if (a.ld < a.heads * (2 * a.key_dim + a.head_dim) || a.ldo < a.heads * a.head_dim) BSY_FAIL(BSY_ERR_ARG, "attention: row stride too small");
    if (impl < 0 || impl > 2) BSY_FAIL(BSY_ERR_ARG, "attention: impl must be 0 (auto), 1 (resident) or 2 (streaming)");
    if (a.pe_w) {
        if (!a.pe_b || a.H <= 0 || a.W <= 0 || (long long)a.H * a.W != a.N) BSY_FAIL(BSY_ERR_ARG, "attention: pe needs its bias and H * W == N");
        if (((uintptr_t)a.pe_w & 15) || ((uintptr_t)a.pe_b & 15)) BSY_FAIL(BSY_ERR_ARG, "attention: pe weights must be 16-byte aligned");
    }
    if ((long long)a.B * a.N * (a.ld > a.ldo ? a.ld : a.ldo) >= (1LL << 40)) BSY_FAIL(BSY_ERR_ARG, "attention: view too large");
    const int nblk = (a.N + 31) / 32;
    const bool fits = nblk * 32 <= attn_res_rows(a.key_dim, a.head_dim);
    if (impl == 1 && !fits) BSY_FAIL(BSY_ERR_ARG, "attention: %d keys of %d + %d channels do not fit the resident form", a.N, a.key_dim, a.head_dim);
    const bool res = impl == 1 || (impl == 0 && fits);
    AttnKArgs k;
    k.qkv = a.qkv; k.out = a.out; k.pe_w = a.pe_w; k.pe_b = a.pe_w ? a.pe_b : nullptr;
    k.ld = a.ld; k.ldo = a.ldo; k.N = a.N; k.heads = a.heads; k.W = a.pe_w ? a.W : 1;
    k.scale = a.scale;
    // resident: one workgroup per (image, head); where those alone leave CUs of the 256 empty (an 8-image shard: 32 pairs), the query
    // blocks of a head go to several workgroups, at most one per block of every wave.  Shape and batch decide, nothing else.
    int nsplit = 1;
    if (res) {
        const long long pairs = (long long)a.B * a.heads;
        const int nw = attn_waves(a.head_dim, true);
        const int want = pairs >= 256 ? 1 : (int)((256 + pairs - 1) / pairs), cap = (nblk + nw - 1) / nw;
        nsplit = want < cap ? want : cap;
    }
    const dim3 grid(res ? nsplit : (nblk + 3) / 4, a.heads, a.B);
#define ATT_GO(KD_, HD_)                                                                                \
    if (a.key_dim == KD_ && a.head_dim == HD_) {                                                        \
        if (res) hipLaunchKernelGGL((attention_kernel<KD_, HD_, true>), grid, dim3(attn_waves(HD_, true) * 64), 0, s, k); \
        else hipLaunchKernelGGL((attention_kernel<KD_, HD_, false>), grid, dim3(256), 0, s, k);         \
    }
#define ATT_ROW(KD_) ATT_GO(KD_, 32) ATT_GO(KD_, 64) ATT_GO(KD_, 96) ATT_GO(KD_, 128)
    ATT_ROW(16) ATT_ROW(32) ATT_ROW(48) ATT_ROW(64)
#undef ATT_ROW
#undef ATT_GO
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}
