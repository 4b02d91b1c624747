// Building blocks of the persistent fused block kernels (stem_fused.hip, bneck_fused.hip, c3k2_fused.hip; pmsfa_fused.hip uses the
// weight staging and the plain epilogue): a workgroup owns a TH x TW output tile, keeps its weights on chip, parks intermediate
// maps in LDS with padded pitches and runs every conv on v_mfma_f32_32x32x16_f16 (A = 32 couts x 16 k, B = 16 k x 32 pixels,
// lane = pixel, lane half lh = k .. k + 7 of the step; accumulator register r = cout (r & 3) + 8 (r >> 2) + 4 lh).
// Every shape is a template parameter and everything is force-inlined.  The epilogues and the tap walk compile to what the
// hand-written copies compiled to; the two helpers that hold a loop over threads (stage_rows, store_tile) are optimised before
// they are inlined and reorder a few hundred instructions around them, registers and LDS unchanged (tools/isa_diff.py; docs/experiments.md,
// "Fused block kernels on shared tile helpers").  A new fused kernel starts from these, not from a copy.
#pragma once
#include "common.h"

// ---- weights --------------------------------------------------------------------------------------------------------------------
// Rows [0, ROWS) of a packed weight matrix ([CoutPad][kpad] halves) -> LDS rows of PITCH halves, CHUNKS 16-byte pieces per row, by
// the NT threads of the workgroup.  PITCH = K + 8: a pitch of 16 x odd bytes makes the lanes' ds_read_b128 of an A fragment (lane =
// row) conflict-free.  Visible after the next barrier.  The global loads are retired by the s_waitcnt vmcnt(0) every kernel places
// in front of its tile loop: left pending, the compiler waits for them at their first use INSIDE the loop with vmcnt(0) -- on every
// iteration, which then also waits for the tile prefetch issued just before.
template <int NT, int ROWS, int CHUNKS, int PITCH>
__device__ __forceinline__ void stage_rows(half_t* dst, const half_t* src, int kpad, int tid) {
    for (int i = tid; i < ROWS * CHUNKS; i += NT) {
        const int row = i / CHUNKS, ch = i - row * CHUNKS;
        *reinterpret_cast<half8*>(dst + row * PITCH + ch * 8) = *reinterpret_cast<const half8*>(src + (size_t)row * kpad + ch * 8);
    }
}

// The same where the shape is known at launch only (ghost_fused.hip: one instantiation per accumulator count serves every width).
template <int NT>
__device__ __forceinline__ void stage_rows(half_t* dst, const half_t* src, int kpad, int tid, int rows, int chunks, int pitch) {
    for (int i = tid; i < rows * chunks; i += NT) {
        const int row = i / chunks, ch = i - row * chunks;
        *reinterpret_cast<half8*>(dst + row * pitch + ch * 8) = *reinterpret_cast<const half8*>(src + (size_t)row * kpad + ch * 8);
    }
}

// ---- epilogues --------------------------------------------------------------------------------------------------------------------
// Group g of an accumulator tile: couts 8g + 4lh .. + 3 of this lane's pixel
__device__ __forceinline__ f32x4 acc_group(const f32x16& acc, int g) {
    return f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
}

// Activation, rounded to f16: the four values a lane stores to an LDS tile as one 8-byte piece.  RELU = false: SiLU if act, the form
// every fused block kernel had; RELU = true (stem_fused_kernel_relu alone): ReLU, whatever act says.  The epilogues
// return the piece and the caller stores it (`*reinterpret_cast<half4*>(dst) = act_f16(..)`): the address is then evaluated after
// the arithmetic, as in the loops these replace -- with `dst` as an argument the register allocation of every caller moved.
template <bool RELU = false>
__device__ __forceinline__ half4 act_f16(f32x4 t, int act) {
    half4 o;
    if constexpr (RELU) t = relu4_f(t);
    else if (act) t = silu4_f(t);
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = (half_t)t[q];
    return o;
}
// The same for a pixel of an intermediate patch that may lie outside the map, where the next conv's zero padding belongs:
// keep = all ones inside, 0 outside.  An AND with the word, not a select on `inside`: the select makes the compiler branch
// around each SiLU.
template <bool RELU = false>
__device__ __forceinline__ half4 act_f16(f32x4 t, int act, unsigned keep) {
    union { half4 h; unsigned u[2]; } o;
    if constexpr (RELU) t = relu4_f(t);
    else if (act) t = silu4_f(t);
#pragma unroll
    for (int q = 0; q < 4; ++q) o.h[q] = (half_t)t[q];
    o.u[0] &= keep;
    o.u[1] &= keep;
    return o.h;
}
// Shortcut epilogue: activation + rv.  The activation is rounded to f16 BEFORE the add and the sum is taken in f32, as
// conv_kernels.h conv_epilogue_lds does for a conv with a residual operand: the unfused launch stores nothing wider.
__device__ __forceinline__ half4 act_res_f16(half4 rv, f32x4 t, int act) {
    half4 o;
    if (act) t = silu4_f(t);
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = (half_t)((float)(half_t)t[q] + (float)rv[q]);
    return o;
}

// ---- 3x3 conv over a padded LDS patch -------------------------------------------------------------------------------------------
// K order of a 3x3 conv's MFMA steps (conv_select.hip conv_korder: a fused kernel walks K as the conv kernels walk that layer).
enum class KOrder {
    TapMajor,      // k = (tap, channel): step ks covers k0 = 16 ks
    Chunk32Major,  // CIN % 32 == 0: (32-channel chunk, tap, 16-wide half of the chunk)
};
// acc += W (32 couts x 9 CIN) . patch, KSTEPS steps of 16.  The patch holds PITCH halves per pixel and ROWPX pixels per row; bbase =
// this lane's pixel at tap (0, 0) + 8 lh, so every B fragment is ONE ds_read_b128 at a compile-time offset.  afrag(k0) returns the
// A fragment of columns k0 .. k0 + 15 of the weight matrix (k = tap * CIN + channel): from a register array or from LDS.
template <int CIN, int ROWPX, int PITCH, int KSTEPS, KOrder ORDER = KOrder::TapMajor, typename AFrag>
__device__ __forceinline__ void mfma_taps3x3(f32x16& acc, AFrag afrag, const half_t* bbase) {
    static_assert(ORDER == KOrder::TapMajor || CIN % 32 == 0, "chunk-major walk: 32-channel chunks");
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
        // compile-time; lane half 1 = the next 8-channel piece
        const int k0 = ORDER == KOrder::TapMajor ? 16 * ks : ((ks % 18) >> 1) * CIN + 32 * (ks / 18) + 16 * (ks & 1);
        const int tap = k0 / CIN, ch0 = (k0 % CIN) / 8;
        const half8 bf = *reinterpret_cast<const half8*>(bbase + ((tap / 3) * ROWPX + tap % 3) * PITCH + ch0 * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(afrag(k0), bf, acc, 0, 0, 0);
    }
}

// ---- tiles ------------------------------------------------------------------------------------------------------------------------
struct TileOrigin {
    int n, oy0, ox0;  // image, first output row and column
};
template <int TH, int TW>
__device__ __forceinline__ TileOrigin tile_origin(const TileGrid& grid, int tile) {
    const TileIdx t = tile_index(grid, tile);
    return TileOrigin{t.n, t.ty * TH, t.tx * TW};
}

// Output tile in LDS ([TH * TW pixels][LDO halves], C channels used) -> NHWC view dst (B x H x W, pixel pitch ldd), 16-byte pieces,
// consecutive threads on consecutive pieces of a pixel; pixels outside the map are skipped.
template <int TH, int TW, int C, int LDO, int NT>
__device__ __forceinline__ void store_tile(half_t* dst, int H, int W, int ldd, const half_t* sout, int n, int oy0, int ox0, int tid) {
    constexpr int CPRW = C / 8;
#pragma unroll
    for (int id = tid; id < TH * TW * CPRW; id += NT) {
        const int prow = id / CPRW, cc = (id % CPRW) * 8;
        const int oy = oy0 + prow / TW, ox = ox0 + prow % TW;
        if (oy < H && ox < W)
            *reinterpret_cast<half8*>(dst + ((size_t)(n * H + oy) * W + ox) * ldd + cc) = *reinterpret_cast<const half8*>(sout + prow * LDO + cc);
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
// Grid of a persistent kernel: every tile its own workgroup up to `slots`, the number resident at once (256 CUs x workgroups per CU)
static inline int persistent_grid(int ntiles, int slots) { return ntiles < slots ? ntiles : slots; }
template <typename... P>
static inline bool all_aligned16(const P*... ptrs) {
    return !((... | (uintptr_t)ptrs) & 15);
}
