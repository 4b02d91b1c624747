// Host side of the fp16 conv op: which kernel configuration runs a layer.  The table kConvCfgs is the one place that says which
// configuration ids exist; the kernels live in conv_gemm.hip, conv_stream1x1.hip and conv_patch.hip (map: conv_kernels.h).
#include <stdlib.h>

#include "conv_kernels.h"

extern "C" int bsy_conv_packed_dims(int C2, int C1, int ksize, int* cout_pad, int* k_pad) {
    if (C2 <= 0 || C1 <= 0 || (ksize != 1 && ksize != 3)) BSY_FAIL(BSY_ERR_ARG, "conv_packed_dims: bad shape");
    if (cout_pad) *cout_pad = round_up(C2, 128);
    if (C1 == 3) C1 = 4;  // image convs are packed with a zero 4th input channel (image_conv.h)
    if (k_pad) *k_pad = round_up(ksize * ksize * C1, 32);
    return BSY_OK;
}

// The K walk of a layer -- the order in which its products enter the fp32 accumulators, hence its result's bits -- is a function of
// the layer's SHAPE alone; every kernel configuration that is valid for the layer sums in that order (round 3: a tuned plan
// returns bit for bit what the heuristic plan returns, on any box).
//   0: the packed order (taps outer, channels inner): 1x1 convs (one tap) and unaligned channel counts (generic variant only);
//   1: chunk-major, 32-channel chunks: aligned 3x3 layers -- the patch kernel's order; implicit-GEMM tiles walk it with BK 32;
//   2: chunk-major, 64-channel chunks: aligned 3x3 STRIDE-2 layers with Cin % 64 == 0 (no patch kernel there; the BK-64 tiles
//      these layers run fastest on sum in this order, BK-32 tiles visit the two halves of a chunk tap by tap).
int conv_korder(const ConvArgs& a) {
    const int Cin = a.C0 + a.C1;
    if (a.ksize != 3 || (Cin & 31) || (a.C0 & 31)) return 0;
    return (a.stride == 2 && !(Cin & 63) && !(a.C0 & 63)) ? 2 : 1;
}

// Kernel configuration id: tile << 4 | variant, + 4 (the chunk-major bit) on an implicit-GEMM tile of a layer whose K walk is chunk-major
// (conv_korder != 0), so that ids recorded before round 3 for the packed order on such a layer are recognised as stale (invalid ->
// heuristic).  kConvCfgs has one row per id the library launches (a 64-cout patch id has a second one with the box-branch tail):
// conv_cfg_valid, conv_candidates and launch_conv read what an id is from there.
enum ConvFam { CONV_GEMM, CONV_PERSIST, CONV_WRES, CONV_PATCH, CONV_TAIL };
struct ConvCfg {
    int id; ConvFam fam;     // id without the chunk-major bit
    int tm, tn, stages, bk;  // pixel tile x cout tile, DMA ring depth (K-steps), K-step (channels)
    bool aligned;            // 32-channel-aligned operands; false: generic (per-lane K bookkeeping, flat DMA)
    int tw, nfr;             // patch tile width: 16 (8 x 16 px) or 20 (6 x 20 px); weights-resident: most A fragments per wave built for
};
// The rows name the template arguments of the instantiation an id stands for; the instantiations themselves are the cases of the
// owning unit's launcher (conv_kernels.h: launch_gemm_cfg, launch_stream1x1_cfg, launch_patch_cfg), same arguments, same id.
template <int WM, int WN, int MT, int NT, int S, bool AL, int BK> constexpr ConvCfg gemm_row(int id) {
    return {id, CONV_GEMM, WM * MT * 32, WN * NT * 32, S, BK, AL, 0, 0};
}
template <int WM, int WN, int MT, int NT, int S, int BK> constexpr ConvCfg persist_row(int id) {
    return {id, CONV_PERSIST, WM * MT * 32, WN * NT * 32, S, BK, true, 0, 0};
}
template <int NT, int S, int NFR> constexpr ConvCfg wres_row(int id) {
    return {id, CONV_WRES, 128, 64 * NT, S, 32, true, 0, NFR};
}
template <int NT, int S, int TW, bool TAIL = false> constexpr ConvCfg patch_row(int id) {
    return {id, TAIL ? CONV_TAIL : CONV_PATCH, TW == 16 ? 8 * 16 : 6 * 20, 64 * NT, S, 32, true, TW, 0};
}
// gemm_row<WM, WN, MT, NT, STAGES, ALIGNED, BK>(id), variant 0 = generic (BK 32, 3 stages), 1 = aligned BK 32 / 3 stages, 2 = aligned
// BK 32 / 2 stages, 3 = aligned BK 64 / 2 stages.  conv_candidates' sweep walks the implicit-GEMM and persistent rows in this order.
static const ConvCfg kConvCfgs[] = {
    gemm_row<4, 1, 2, 1, 3, false, 32>(0x00),  // 256 px x 32 couts (4 waves)
    gemm_row<4, 1, 2, 1, 3, true, 32>(0x01),
    gemm_row<4, 1, 2, 1, 2, true, 32>(0x02),
    gemm_row<4, 1, 2, 1, 2, true, 64>(0x03),
    gemm_row<4, 1, 2, 2, 3, false, 32>(0x10),  // 256 x 64 (4 x 1 waves: all 64 couts in one wave, what the DFL decoder needs)
    gemm_row<4, 1, 2, 2, 3, true, 32>(0x11),
    gemm_row<4, 1, 2, 2, 2, true, 32>(0x12),
    gemm_row<4, 1, 2, 2, 2, true, 64>(0x13),
    gemm_row<2, 2, 2, 2, 3, false, 32>(0x20),  // 128 x 128
    gemm_row<2, 2, 2, 2, 3, true, 32>(0x21),
    gemm_row<2, 2, 2, 2, 2, true, 32>(0x22),
    gemm_row<2, 2, 2, 2, 2, true, 64>(0x23),
    gemm_row<2, 2, 2, 1, 3, false, 32>(0x30),  // 128 x 64
    gemm_row<2, 2, 2, 1, 3, true, 32>(0x31),
    gemm_row<2, 2, 2, 1, 2, true, 32>(0x32),
    gemm_row<2, 2, 2, 1, 2, true, 64>(0x33),
    gemm_row<4, 2, 2, 2, 3, true, 32>(0x41),   // 256 x 128 (8 waves), aligned variants only
    gemm_row<4, 2, 2, 2, 2, true, 32>(0x42),
    gemm_row<4, 2, 2, 2, 2, true, 64>(0x43),   //   (96 KiB of LDS)
    gemm_row<1, 4, 2, 1, 3, false, 32>(0x50),  // 64 x 128: small tiles = many resident workgroups for the latency-bound thin-K layers
    gemm_row<1, 4, 2, 1, 3, true, 32>(0x51),
    gemm_row<1, 4, 2, 1, 2, true, 32>(0x52),
    gemm_row<1, 4, 2, 1, 2, true, 64>(0x53),
    gemm_row<2, 2, 1, 1, 3, false, 32>(0x60),  // 64 x 64, likewise
    gemm_row<2, 2, 1, 1, 3, true, 32>(0x61),
    gemm_row<2, 2, 1, 1, 2, true, 32>(0x62),
    gemm_row<2, 2, 1, 1, 2, true, 64>(0x63),
    gemm_row<4, 2, 2, 4, 3, true, 32>(0x71),   // 256 x 256 (8 waves, wave tile 64 x 128: half the L2->LDS bytes per FLOP of 128 x 128)
    gemm_row<4, 2, 2, 4, 2, true, 32>(0x72),
    gemm_row<4, 2, 2, 4, 2, true, 64>(0x73),   //   (128 KiB of LDS)
    persist_row<2, 2, 2, 2, 3, 32>(0x81),      // persistent 1x1 kernel (4 compute + 4 store waves, tiles walked per workgroup): 128 x 128
    persist_row<2, 2, 2, 2, 2, 32>(0x82),
    persist_row<2, 2, 2, 2, 2, 64>(0x83),
    persist_row<2, 2, 2, 1, 3, 32>(0x91),      // 128 x 64
    persist_row<2, 2, 2, 1, 2, 32>(0x92),
    persist_row<2, 2, 2, 1, 2, 64>(0x93),
    patch_row<2, 2, 16>(0xA1),                 // patch-based 3x3 stride-1 kernel <NT, STAGES, TW>: 8 x 16 px x 128 couts
    patch_row<1, 3, 16>(0xB1),                 // 64 couts
    patch_row<1, 2, 16>(0xB2),
    patch_row<1, 4, 16>(0xB3),
    patch_row<2, 2, 20>(0xC1),                 // 6 x 20 px x 128 couts
    patch_row<1, 3, 20>(0xD1),
    patch_row<1, 2, 20>(0xD2),
    patch_row<1, 4, 20>(0xD3),
    patch_row<1, 3, 16, true>(0xB1),           // + box-branch tail (ConvArgs::tail_wgt: the 1x1 conv and DFL decoder after the 3x3 conv)
    patch_row<1, 2, 16, true>(0xB2),
    patch_row<1, 4, 16, true>(0xB3),
    patch_row<1, 3, 20, true>(0xD1),
    patch_row<1, 2, 20, true>(0xD2),
    patch_row<1, 4, 20, true>(0xD3),
    wres_row<2, 4, 24>(0xE1),                  // weights-resident streaming 1x1 kernel <NT, STAGES, NFR>: 128 px x 128 couts (NFR 32 would spill)
    wres_row<2, 3, 24>(0xE2),
    wres_row<1, 4, 32>(0xF1),                  // 128 px x 64 couts
    wres_row<1, 3, 32>(0xF2),
};

static const ConvCfg* conv_cfg_row(int cfg, bool tail) {
    for (const ConvCfg& r : kConvCfgs) if (r.id == (cfg & ~4) && (r.fam == CONV_TAIL) == tail) return &r;
    return nullptr;
}

bool conv_cfg_valid(const ConvArgs& a, int cfg) {
    const ConvCfg* r = conv_cfg_row(cfg, a.tail_wgt != nullptr);
    if (!r) return false;
    const int Cin = a.C0 + a.C1, ko = conv_korder(a), nsl = a.nsl_c * a.nsl_t;
    const bool aligned = !(Cin & 31) && !(a.C0 & 31), aligned64 = !(Cin & 63) && !(a.C0 & 63);
    if ((r->aligned && !aligned) || (r->bk == 64 && !aligned64)) return false;
    if (r->fam == CONV_GEMM) {
        if (!(cfg & 4) != !ko) return false;  // the id's chunk-major bit must say what the layer's shape says
        // a chunk-major walk needs aligned operands; on 32-channel chunks a 64-deep K-step would pair the halves of two chunks
        if (ko && (!r->aligned || (ko == 1 && r->bk == 64))) return false;
        if (nsl > 1 && (!r->aligned || (Cin / (a.nsl_c > 0 ? a.nsl_c : 1)) % r->bk)) return false;  // split-K: K-steps within a slice
        if (a.epi == 3 && (r->tm != 256 || r->tn != 64)) return false;  // DFL needs all 64 box couts in one wave
        return r->tn != 256 || !(a.Cout & 255);                          // whole 256-cout tiles only
    }
    // the other kernels: one K walk each (no chunk-major bit), no split-K, no fused decoder but the tail's, fp16 output in 16-byte stores
    if ((cfg & 4) || nsl > 1 || (r->fam == CONV_TAIL ? (a.epi != 3 || a.Cout != 64 || a.res) : a.epi != 0)) return false;
    if (a.out_f32 || (a.Cout & 7) || (a.ldd & 7) || ((uintptr_t)a.dst & 15) || a.dst_scale > 1) return false;
    if (r->fam == CONV_PERSIST || r->fam == CONV_WRES) {  // the streaming 1x1 kernels
        if (a.ksize != 1 || a.stride != 1 || a.res) return false;
        if (r->fam == CONV_PERSIST) return a.Cout <= PERSIST_MAX_COUT;  // the bias vector stays in LDS
        // weights-resident: K fits the row's register fragments and the pixel ring; 128-cout tiles only past 64 couts
        return (r->tn / 64) * (Cin / 16) <= r->nfr && Cin / 32 >= r->stages - 1 && (r->tn != 128 || a.Cout > 64);
    }
    // patch (+ tail): 3x3 stride 1, one source, no upsample; sums chunk-major over 32-channel chunks = K walk 1
    return ko == 1 && a.ksize == 3 && a.stride == 1 && a.pad == 1 && !a.C1 && !a.up0 && (!a.res || (!(a.ldr & 7) && !((uintptr_t)a.res & 15))) &&
           (r->tn != 128 || a.Cout > 64);
}

// Selection aids of the tests and tools: BSY_NO_PATCH / BSY_NO_PERSIST / BSY_NO_WRES keep a family out of the candidate lists (an
// explicit ConvArgs::cfg still runs it).  Read at every call: the tests set and clear them within one process.
static bool family_off(const char* env) { return getenv(env) != nullptr; }

int conv_candidates(const ConvArgs& a, int* out, int max_out) {
    const int Cin = a.C0 + a.C1;
    const bool aligned = !(Cin & 31) && !(a.C0 & 31), aligned64 = !(Cin & 63) && !(a.C0 & 63);
    const long long M = (long long)a.B * a.OH * a.OW;
    const int tile = a.epi == 3 ? 1 : (a.Cout > 64 ? 2 : (a.Cout > 32 ? 1 : 0));  // heuristic default: widest cout tile that is not wasted
    const int ko = conv_korder(a), km = ko ? 4 : 0;
    // 6x20 tiles where they need fewer tiles than 8x16 ones (20 x 20 maps: 4 instead of 6 per image)
    const bool t20 = ceil_div(a.W, 20) * ceil_div(a.H, 6) < ceil_div(a.W, 16) * ceil_div(a.H, 8);
    int n = 0;
    auto add = [&](int c) {
        for (int i = 0; i < n; ++i) if (out[i] == c) return;
        if (n < max_out && conv_cfg_valid(a, c)) out[n++] = c;
    };
    if (a.tail_wgt) {  // 3x3 conv + 1x1 + DFL: the 64-cout patch configurations
        if (t20) { add(0xD2); add(0xD1); add(0xD3); }
        add(0xB2); add(0xB1); add(0xB3); add(0xD2); add(0xD1); add(0xD3);
        return n;
    }
    if (!aligned) {
        add(tile << 4);
        if (a.Cout > 32) { add(0x30); add(0x60); }
        if (a.Cout > 64) add(0x50);
        return n;
    }
    // heuristic first (what an un-tuned plan runs: the r01 measurements' usual winners), then the exhaustive
    // (tile x variant) sweep the autotuner times.  Every candidate of a layer sums in the layer's K walk (conv_cfg_valid).
    const bool patch_ok = !family_off("BSY_NO_PATCH");
    if (!a.epi && a.ksize == 3 && a.stride == 1 && a.H >= 16 && a.W >= 16 && patch_ok) add(t20 ? 0xD2 : 0xB2);  // patch kernel
    const int vbest = (aligned64 && ko != 1) ? 3 : 1;  // 64-deep K-steps where the K walk allows them
    if (!a.epi && !(a.Cout & 255) && aligned64 && ko != 1 && M >= 16384) add(0x73 | km);  // 256 x 256, 64-deep K-steps
    add(tile << 4 | vbest | km);
    for (const ConvCfg& r : kConvCfgs) {
        if ((r.fam != CONV_GEMM && r.fam != CONV_PERSIST) || !r.aligned) continue;
        if (r.tn >= 2 * round_up(a.Cout, 32)) continue;                           // more than half of the cout tile would be padding
        if (r.tn == 32 && a.Cout > 32) continue;                                    // 32-wide tiles re-read the pixels once per 32 couts
        if (r.tm == 256 && r.tn == 128 && (a.Cout < 128 || M < 32768)) continue;    // 8-wave 256x128 only for wide, large layers
        if (r.tn == 256 && M < 16384) continue;
        if (r.fam == CONV_PERSIST && (M < 65536 || family_off("BSY_NO_PERSIST"))) continue;  // persistent tiles need several tiles per workgroup
        add(r.id | (r.fam == CONV_GEMM ? km : 0));
    }
    if (a.ksize == 1 && M >= 65536 && !family_off("BSY_NO_WRES"))  // HBM-bound 1x1 layers
        for (const ConvCfg& r : kConvCfgs) if (r.fam == CONV_WRES) add(r.id);
    if (a.H >= 16 && a.W >= 16 && patch_ok)  // 3x3 s1 patch kernel
        for (const ConvCfg& r : kConvCfgs) if (r.fam == CONV_PATCH && (r.tw == 16 || t20)) add(r.id);
    return n;
}

int launch_conv(const ConvArgs& a, hipStream_t s) {
    const int Cin = a.C0 + a.C1;
    if (a.ksize != 1 && a.ksize != 3) BSY_FAIL(BSY_ERR_ARG, "conv: ksize %d unsupported", a.ksize);
    if (a.stride != 1 && a.stride != 2) BSY_FAIL(BSY_ERR_ARG, "conv: stride %d unsupported", a.stride);
    if ((a.C0 & 7) || (a.C1 & 7) || (a.ld0 & 7) || (a.C1 && (a.ld1 & 7)))
        BSY_FAIL(BSY_ERR_ARG, "conv: channel counts/strides must be multiples of 8 (C0=%d C1=%d ld0=%d ld1=%d)", a.C0,
                 a.C1, a.ld0, a.ld1);
    if ((a.ldd & 3) || (a.res && (a.ldr & 3))) BSY_FAIL(BSY_ERR_ARG, "conv: dst/res row stride must be a multiple of 4");
    if (((uintptr_t)a.src0 & 15) || ((uintptr_t)a.src1 & 15) || ((uintptr_t)a.wgt & 15) || ((uintptr_t)a.bias & 15) ||
        ((uintptr_t)a.dst & 7) || ((uintptr_t)a.res & 7))
        BSY_FAIL(BSY_ERR_ARG, "conv: misaligned pointer");
    if (a.C1 && !a.src1) BSY_FAIL(BSY_ERR_ARG, "conv: src1 missing");
    if ((a.up0 && ((a.H | a.W) & 1)) || (a.up1 && ((a.H | a.W) & 1))) BSY_FAIL(BSY_ERR_ARG, "conv: odd size with upsample");
    if (a.OH != (a.H + 2 * a.pad - a.ksize) / a.stride + 1 || a.OW != (a.W + 2 * a.pad - a.ksize) / a.stride + 1)
        BSY_FAIL(BSY_ERR_ARG, "conv: output extent mismatch");
    const long long M = (long long)a.B * a.OH * a.OW;
    if (M <= 0 || M > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "conv: M out of range");
    if (a.epi) {
        if ((a.epi != 2 && a.epi != 3) || !a.y || a.A <= 0 || a.a0 < 0 || a.a0 + a.OH * a.OW > a.A || a.dst_scale > 1 || a.res)
            BSY_FAIL(BSY_ERR_ARG, "conv: bad fused-decoder arguments (epi %d)", a.epi);
        if (a.epi == 3 && (a.Cout != 64 || a.nrows < 4)) BSY_FAIL(BSY_ERR_ARG, "conv: DFL epilogue needs 64 box channels");
        if (a.tail_wgt && (a.epi != 3 || !a.tail_bias || a.ksize != 3 || ((uintptr_t)a.tail_wgt & 15) || ((uintptr_t)a.tail_bias & 15)))
            BSY_FAIL(BSY_ERR_ARG, "conv: bad box-branch tail arguments");
        if (a.epi == 2 && a.nrows < 4 + a.Cout) BSY_FAIL(BSY_ERR_ARG, "conv: y has %d rows, class epilogue needs %d", a.nrows, 4 + a.Cout);
        if (a.raw && a.rawC < (a.epi == 3 ? 64 : 64 + a.Cout)) BSY_FAIL(BSY_ERR_ARG, "conv: raw map has too few channels");
    }
    ConvK k;
    k.src0 = a.src0; k.src1 = a.src1; k.ld0 = a.ld0; k.ld1 = a.ld1; k.C0 = a.C0; k.C1 = a.C1;
    k.up0 = a.up0; k.up1 = a.up1; k.H = a.H; k.W = a.W; k.OH = a.OH; k.OW = a.OW; k.stride = a.stride; k.pad = a.pad;
    k.M = (int)M; k.Cin8 = Cin / 8; k.ntaps = a.ksize * a.ksize;
    k.Kpad = round_up(a.ksize * a.ksize * Cin, 32); k.nk = k.Kpad / 32;
    k.wgt = a.wgt; k.bias = a.bias; k.dst = a.dst; k.ldd = a.ldd; k.Cout = a.Cout; k.out_f32 = a.out_f32;
    k.res = a.res; k.ldr = a.ldr; k.act = a.act; k.B = a.B; k.tiles_x = k.tiles_y = 0;
    k.epi = a.epi; k.y = a.y; k.y_f32 = a.y_f32; k.A = a.A; k.a0 = a.a0; k.nrows = a.nrows; k.lvl_stride = a.lvl_stride;
    k.xyxy = a.epi == 3 && a.xyxy;
    k.raw = a.raw; k.raw_f32 = a.raw_f32; k.rawC = a.rawC;
    k.tail_wgt = a.tail_wgt; k.tail_bias = a.tail_bias;
    if (a.tail_wgt && !a.epi) BSY_FAIL(BSY_ERR_ARG, "conv: a box-branch tail needs the decoder arguments (epi 3)");
    k.dst_scale = a.dst_scale > 0 ? a.dst_scale : 1; k.dst_dy = a.dst_dy; k.dst_dx = a.dst_dx; k.ntn = 1;
    k.nsl_c = k.nsl_t = 1; k.cb_per = Cin; k.taps_per = a.ksize * a.ksize; k.split_ws = nullptr; k.slab = 0; k.ldw = 0;
    if (a.nsl_c * a.nsl_t > 1) {
        const int nt = a.ksize * a.ksize;
        if (a.nsl_c < 1 || a.nsl_t < 1 || !a.split_ws || a.epi || a.out_f32 || a.tail_wgt || (a.dst_scale > 1) || (Cin % a.nsl_c) || ((Cin / a.nsl_c) & 31) || (a.C0 & 31) ||
            (nt % a.nsl_t) || (a.Cout & 7) || (a.ldd & 7) || ((uintptr_t)a.dst & 15) || (a.res && ((a.ldr & 7) || ((uintptr_t)a.res & 15))) || ((uintptr_t)a.split_ws & 15))
            BSY_FAIL(BSY_ERR_ARG, "conv: bad split-K arguments (%d x %d slices)", a.nsl_c, a.nsl_t);
        if (conv_korder(a) == 2 && ((Cin / a.nsl_c) & 63)) BSY_FAIL(BSY_ERR_ARG, "conv: split-K slices of a 64-channel-chunk layer must be multiples of 64 channels");
        k.nsl_c = a.nsl_c; k.nsl_t = a.nsl_t; k.cb_per = Cin / a.nsl_c; k.taps_per = nt / a.nsl_t; k.split_ws = a.split_ws;
        k.ldw = round_up(a.Cout, 32);               // whole 32-cout MFMA tiles: the slab rows take every accumulator group unconditionally
        k.slab = (long long)M * k.ldw;
    }
    // ---- configuration: explicit (autotuned, ConvArgs::cfg) or heuristic -----------------------------------------
    if (a.ksize == 3 && (a.up0 || a.up1)) BSY_FAIL(BSY_ERR_ARG, "conv: upsampled source only with ksize 1");
    // element offsets are kept in 32 bits inside the kernel
    if ((long long)a.B * a.H * a.W * (long long)(a.ld0 > a.ld1 ? a.ld0 : a.ld1) >= (1LL << 31))
        BSY_FAIL(BSY_ERR_ARG, "conv: source view exceeds 2^31 elements (split the batch)");
    {   // bytes addressable from each view's first element up to its last element (descriptor range check)
        const long long px0 = (long long)a.B * (a.H >> a.up0) * (a.W >> a.up0), px1 = (long long)a.B * (a.H >> a.up1) * (a.W >> a.up1);
        k.span0 = (unsigned)(((px0 - 1) * a.ld0 + a.C0) * 2);
        k.span1 = a.C1 ? (unsigned)(((px1 - 1) * a.ld1 + a.C1) * 2) : 0u;
        k.wspan = (unsigned)((long long)round_up(a.Cout, 128) * k.Kpad * 2);
    }
    int cfg = a.cfg;
    if (cfg < 0 || !conv_cfg_valid(a, cfg)) {
        int list[BSY_CONV_MAX_CFG];
        if (conv_candidates(a, list, BSY_CONV_MAX_CFG) <= 0) BSY_FAIL(BSY_ERR_ARG, "conv: no kernel configuration for this shape");
        cfg = list[0];
    }
    k.korder = conv_korder(a);
    const ConvCfg* r = conv_cfg_row(cfg, a.tail_wgt != nullptr);
    switch (r->fam) {
        case CONV_GEMM: return launch_gemm_cfg(r->id, a.ksize, k, s);
        case CONV_PERSIST:
        case CONV_WRES: return launch_stream1x1_cfg(r->id, k, s);
        case CONV_PATCH:
        case CONV_TAIL: return launch_patch_cfg(r->id, r->fam == CONV_TAIL, k, s);
    }
    BSY_FAIL(BSY_ERR_ARG, "conv: configuration 0x%02x has no kernel family", cfg);
}
