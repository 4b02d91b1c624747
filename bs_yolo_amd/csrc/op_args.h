// What a bsy_op record MEANS: one builder per op kind and storage type turns a record (include/bsyolo.h) into the launch arguments of
// its kernel family (common.h).  This is the one place where the record's overloaded fields are read -- `heads` as a weight row length,
// `pad` as a kernel width, `lvl_h[1]` as a first anchor, `act` as a DFL order, `level` as a pooling mode (POOL_DOWN, MAXPOOL) -- for plan_ops.hip (the two
// dispatch switches) and for the tuners of engine.hip, which need a conv's arguments without a launch.  A builder takes the record, the
// resolver and the base of the weight blob, and returns false on refusal with the error text set.  Nothing here launches, allocates or
// needs a device or a plan object: tools/op_args_check.cpp drives the builders over a host vector.
#pragma once
#include "common.h"

// Views -> pointers.  Workspace buffers are offsets behind `ws`, external slots are the caller's pointers.
struct Resolver {
    char* ws;            // base of the plan's workspace (or of the engine's arena)
    const size_t* off;   // byte offset of every workspace buffer
    size_t n_bufs;
    void* const* ext;
    int n_ext;
    bool ok = true;      // false once a required view did not resolve (the error text says which)
    // a present workspace view or a bound external slot; never records an error: the test for OPTIONAL outputs
    bool bound(const bsy_view& v) const {
        if (v.buf >= BSY_EXT_BASE) return v.buf - BSY_EXT_BASE < n_ext && ext[v.buf - BSY_EXT_BASE];
        return v.buf >= 0 && (size_t)v.buf < n_bufs;
    }
    // base pointer of the buffer (no channel offset), nullptr when the view is absent; anything else unbound is an error
    char* base(const bsy_view& v) {
        if (v.buf < 0) return nullptr;
        if (bound(v)) return v.buf >= BSY_EXT_BASE ? (char*)ext[v.buf - BSY_EXT_BASE] : ws + off[v.buf];
        ok = false;
        if (v.buf >= BSY_EXT_BASE) bsy_set_error("plan_run: external slot %d not bound", v.buf - BSY_EXT_BASE);
        else bsy_set_error("plan_run: buffer %d out of range", v.buf);
        return nullptr;
    }
    template <typename T>
    T* at(const bsy_view& v) { char* b = base(v); return b ? (T*)b + v.coff : nullptr; }
    half_t* h(const bsy_view& v) { return at<half_t>(v); }
    float* f(const bsy_view& v) { return at<float>(v); }
    // an optional output pointer: null when the caller left its slot out
    char* optional(const bsy_view& v) { return bound(v) ? base(v) : nullptr; }
    // an optional output that is a whole op (RAW_NCHW, NHWC2NCHW): its external slot is unbound, the op is skipped
    bool left_out(const bsy_view& v) const { return v.buf >= BSY_EXT_BASE && !bound(v); }
};

// ---- decoding shared by the fp16 and the fp32 storage builders -------------------------------------------------------------------
// ELA: w_off -> f32 blob [spatial_conv C*k][ch_att conv C*k][gn.weight C][gn.bias C]; scale, lvl_stride[0..1] = the three sigmoid
// coefficients; res = the f32 scratch buffer.  Everything but src / dst, whose type is the storage's.
inline void ela_fields(ElaArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.lds = op.src0.ld; a.B = op.B; a.H = op.H; a.W = op.W; a.C = op.src0.C; a.k = op.ksize;
    const float* blob = (const float*)(wb + op.w_off);
    a.wsp = blob; a.wch = blob + (size_t)a.C * a.k; a.gnw = a.wch + (size_t)a.C * a.k; a.gnb = a.gnw + a.C;
    a.ch_coef = op.scale; a.sp_coef = op.lvl_stride[0]; a.res_coef = op.lvl_stride[1];
    a.scratch = R.f(op.res); a.ldd = op.dst.ld;
}
// MSCA_SPATIAL / MSCA_MIX: branch i of four is box[i], the fourth res; its mean / logit map is cls[i], the fourth msk[0]
inline const bsy_view& msca_branch(const bsy_op& op, int i) { return i < 3 ? op.box[i] : op.res; }
inline const bsy_view& msca_stat(const bsy_op& op, int i) { return i < 3 ? op.cls[i] : op.msk[0]; }
// MSCA_MIX (MixArgs of T = half_t, Mix32Args of T = float): the branches are of the storage type, the logits f32 in both
template <typename T, typename Args>
inline bool build_mix(Args& a, const bsy_op& op, Resolver& R, const char*) {
    for (int i = 0; i < 4; ++i) {
        const bsy_view &bv = msca_branch(op, i), &lv = msca_stat(op, i);
        a.br[i] = R.at<T>(bv); a.ldb[i] = bv.ld; a.lg[i] = R.f(lv); a.ldl[i] = lv.ld;
    }
    a.B = op.B; a.HW = op.H * op.W; a.C = op.dst.C; a.dst = R.at<T>(op.dst); a.ldd = op.dst.ld;
    return R.ok;
}
// DWCONV_G (DwGenArgs / Dw32Args): ksize = kernel HEIGHT, pad = kernel WIDTH (padding is always k / 2), heads = row length of the f32
// [kh*kw][heads] weights, key_dim = first channel of this launch inside them, act = number of leading channels with SiLU
template <typename Args>
inline void dwg_fields(Args& a, const bsy_op& op, const char* wb) {
    a.kh = op.ksize; a.kw = op.pad; a.stride = op.stride; a.wld = op.heads;
    a.w = (const float*)(wb + op.w_off) + op.key_dim; a.b = (const float*)(wb + op.b_off) + op.key_dim;
    a.act_c = op.act;
}
// Ops whose launchers take scalars (SPPF_POOL, COPY, GAP, fp32 ATTN, MUL, ADD): only their views are resolved, the first n of src0 (the
// buffer SPPF_POOL works in), dst, src1.  T = the storage type.
template <typename T>
struct Views {
    T* src0 = nullptr;
    T* dst = nullptr;
    const T* src1 = nullptr;
};
template <typename T>
inline bool build_views(Views<T>& v, const bsy_op& op, Resolver& R, int n) {
    v.src0 = R.at<T>(op.src0);
    if (n > 1) v.dst = R.at<T>(op.dst);
    if (n > 2) v.src1 = R.at<T>(op.src1);
    return R.ok;
}
// POOL_DOWN (both storage types): the launcher takes the buffers' first elements and the views' first channels separately
inline bool build_pool_down(const char*& src, char*& dst, const bsy_op& op, Resolver& R) {
    src = R.base(op.src0); dst = R.base(op.dst);
    if (R.ok && op.src0.C != op.dst.C) { R.ok = false; bsy_set_error("pool_down: %d channels in, %d out", op.src0.C, op.dst.C); }
    return R.ok;
}
// MAXPOOL (both storage types): POOL_DOWN's calling convention; `level` = the mode, (H, W) the source's extent, (OH, OW) the destination's
inline bool build_maxpool(const char*& src, char*& dst, const bsy_op& op, Resolver& R) {
    src = R.base(op.src0); dst = R.base(op.dst);
    const int oh = op.level ? op.H : op.H / 2, ow = op.level ? op.W : op.W / 2;
    if (R.ok && (op.src0.C != op.dst.C || op.OH != oh || op.OW != ow)) {
        R.ok = false;
        bsy_set_error("maxpool: %d channels in, %d out; mode %d on %d x %d gives %d x %d, the record says %d x %d", op.src0.C, op.dst.C, op.level, op.H,
                      op.W, oh, ow, op.OH, op.OW);
    }
    return R.ok;
}
// MAXSIG (both storage types): src0 = the embedding, src1 = the projection, dst = its gated copy (may be src1's view); heads x head_dim
// channels each, nc guide rows at w_off, [bias | scale] at b_off.  What needs no pointer is checked here, so that bsy_plan_create can ask
// with an unbound resolver (maxsig_record_ok); the launcher checks the rest
inline bool maxsig_record_ok(const bsy_op& op) {
    const int C = op.heads * op.head_dim;
    if (op.src0.buf < 0 || op.src1.buf < 0 || op.dst.buf < 0) { bsy_set_error("maxsig: null pointer (src0, src1 and dst are all needed)"); return false; }
    if (op.nc < 1) { bsy_set_error("maxsig: nc = %d (at least one guide row)", op.nc); return false; }
    if (op.heads < 1 || op.head_dim < 1 || op.src0.C != C || op.src1.C != C || op.dst.C != C) {
        bsy_set_error("maxsig: %d heads of %d channels on views of %d / %d / %d channels", op.heads, op.head_dim, op.src0.C, op.src1.C, op.dst.C);
        return false;
    }
    if (!op.prec && !maxsig_supported(op.head_dim)) {
        bsy_set_error("maxsig: heads of hc = %d channels are not on the fp16 path (16 to 128 in steps of 16)", op.head_dim);
        return false;
    }
    if (op.src0.buf == op.dst.buf && op.src0.coff < op.dst.coff + C && op.dst.coff < op.src0.coff + C) {
        bsy_set_error("maxsig: the destination overlaps the embedding view (src0)");
        return false;
    }
    return true;
}
inline bool build_maxsig(MaxSigArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    if (!maxsig_record_ok(op)) { R.ok = false; return false; }
    a.dtype = op.prec ? BSY_F32 : BSY_F16;
    if (op.prec) { a.embed = R.f(op.src0); a.proj = R.f(op.src1); a.dst = R.f(op.dst); }
    else { a.embed = R.h(op.src0); a.proj = R.h(op.src1); a.dst = R.h(op.dst); }
    a.lde = op.src0.ld; a.ldp = op.src1.ld; a.ldd = op.dst.ld;
    a.B = op.B; a.HW = op.H * op.W; a.heads = op.heads; a.hc = op.head_dim; a.nc = op.nc;
    a.G = wb + op.w_off; a.bias_scale = (const float*)(wb + op.b_off);
    return R.ok;
}
// CBFUSE (both storage types): src0 = the last input, dst = the sum (may be src0's view); nl taps, tap i = box[i] (i < 4) / cls[0] (i = 4)
// with its shift in lvl_h[i] / lvl_w[0].  What needs no pointer is checked in cbfuse_record_ok, which bsy_plan_create asks as well; the
// launcher checks the rest (alignment, overlap of the resolved addresses)
inline const bsy_view& cbfuse_tap(const bsy_op& op, int i) { return i < BSY_MAX_LEVELS ? op.box[i] : op.cls[i - BSY_MAX_LEVELS]; }
inline int cbfuse_shift(const bsy_op& op, int i) { return i < BSY_MAX_LEVELS ? op.lvl_h[i] : op.lvl_w[i - BSY_MAX_LEVELS]; }
inline bool cbfuse_record_ok(const bsy_op& op) {
    int shift[BSY_CBFUSE_MAX_TAPS] = {};
    for (int i = 0; i < BSY_CBFUSE_MAX_TAPS && i < op.nl; ++i) shift[i] = cbfuse_shift(op, i);
    if (!cbfuse_shape_ok(op.nl, shift, op.H, op.W)) return false;
    const int C = op.dst.C;
    if (op.src0.buf < 0 || op.dst.buf < 0 || C < 1) { bsy_set_error("cbfuse: null pointer (src0 and dst are both needed)"); return false; }
    if (op.src0.C < C) { bsy_set_error("cbfuse: the last input has %d channels, dst %d", op.src0.C, C); return false; }
    if (op.src0.buf == op.dst.buf && (op.src0.coff != op.dst.coff || op.src0.ld != op.dst.ld) && op.src0.coff < op.dst.coff + C &&
        op.dst.coff < op.src0.coff + C) {
        bsy_set_error("cbfuse: the destination overlaps the last input without being its view (in place: the same view)");
        return false;
    }
    for (int i = 0; i < op.nl; ++i) {
        const bsy_view& t = cbfuse_tap(op, i);
        if (t.buf < 0) { bsy_set_error("cbfuse: null pointer (tap %d of %d is absent)", i, op.nl); return false; }
        if (t.C < C) { bsy_set_error("cbfuse: tap %d is narrower (%d channels) than dst (%d)", i, t.C, C); return false; }
        if (t.buf == op.dst.buf && t.coff < op.dst.coff + C && op.dst.coff < t.coff + C) {
            bsy_set_error("cbfuse: the destination overlaps tap %d", i);
            return false;
        }
    }
    return true;
}
inline bool build_cbfuse(CbFuseArgs& a, const bsy_op& op, Resolver& R, const char*) {
    if (!cbfuse_record_ok(op)) { R.ok = false; return false; }
    const bool f32 = op.prec != 0;
    a.dtype = f32 ? BSY_F32 : BSY_F16;
    a.n = op.nl;
    for (int i = 0; i < op.nl; ++i) {
        const bsy_view& t = cbfuse_tap(op, i);
        a.tap[i] = f32 ? (const void*)R.f(t) : (const void*)R.h(t);
        a.ldt[i] = t.ld; a.shift[i] = cbfuse_shift(op, i);
    }
    a.last = f32 ? (const void*)R.f(op.src0) : (const void*)R.h(op.src0);
    a.dst = f32 ? (void*)R.f(op.dst) : (void*)R.h(op.dst);
    a.ldl = op.src0.ld; a.ldd = op.dst.ld; a.B = op.B; a.H = op.H; a.W = op.W; a.C = op.dst.C;
    return R.ok;
}
// NHWC2NCHW: dst = the whole BCHW tensor, an optional output -- `skip`: its slot is unbound, nothing is resolved or launched
template <typename T>
inline bool build_nhwc2nchw(const T*& src, void*& out, bool& skip, const bsy_op& op, Resolver& R) {
    skip = R.left_out(op.dst);
    if (skip) return true;
    src = R.at<T>(op.src0); out = R.base(op.dst);
    return R.ok;
}
// RAW_NCHW: level `level` of the per-level arrays -> the level's raw BCHW map, an optional output like NHWC2NCHW's
struct RawNchwArgs {
    const float *box = nullptr, *cls = nullptr;
    int ldb = 0, ldc = 0, h = 0, w = 0;
    void* out = nullptr;
    bool skip = false;
};
inline bool build_raw_nchw(RawNchwArgs& a, const bsy_op& op, Resolver& R) {
    const int l = op.level;
    if (l < 0 || l >= BSY_MAX_LEVELS) { bsy_set_error("raw_nchw: level %d", l); return false; }
    a.skip = R.left_out(op.dst);
    if (a.skip) return true;
    a.box = R.f(op.box[l]); a.ldb = op.box[l].ld; a.cls = R.f(op.cls[l]); a.ldc = op.cls[l].ld;
    a.h = op.lvl_h[l]; a.w = op.lvl_w[l]; a.out = R.base(op.dst);
    return R.ok;
}
// CLASSIFY_TAIL (csrc/classify.hip): the logit map is f32 in every precision mode.  res = x and box[0] / cls[0] = the top-k index /
// value rows are optional outputs: an unbound slot leaves them out, the rows only together (k is then passed as 0).
struct ClassifyArgs {
    const float* logits = nullptr;
    void *y = nullptr, *x = nullptr;
    int k = 0;
    int32_t* idx = nullptr;
    float* val = nullptr;
};
inline bool build_classify_tail(ClassifyArgs& a, const bsy_op& op, Resolver& R) {
    a.logits = R.f(op.src0); a.y = R.base(op.dst); a.x = R.optional(op.res);
    if (op.ksize > 0 && R.bound(op.box[0]) && R.bound(op.cls[0])) {
        a.k = op.ksize; a.idx = (int32_t*)R.base(op.box[0]); a.val = (float*)R.base(op.cls[0]);
    }
    return R.ok;
}
// E2E_TOPK (csrc/topk.hip, every precision mode): src0 = the pre-top-k tensor (B, 4 + nc, A) of out_dtype, dst = the rows (B, min(ksize, A), 6)
// f32, res = the scratch of bsy_end2end_topk_workspace_bytes(B, A, nc, ksize) bytes (the planner sizes the buffer with the same call)
struct TopkArgs {
    const void* pred = nullptr;
    float* rows = nullptr;
    void* ws = nullptr;
    size_t ws_bytes = 0;
};
inline bool build_e2e_topk(TopkArgs& a, const bsy_op& op, Resolver& R) {
    a.pred = R.base(op.src0); a.rows = (float*)R.base(op.dst); a.ws = R.base(op.res);
    a.ws_bytes = bsy_end2end_topk_workspace_bytes(op.B, op.A, op.nc, op.ksize);
    if (R.ok && (!a.pred || !a.rows || !a.ws || !a.ws_bytes || op.src0.C != 4 + op.nc)) {
        R.ok = false;
        bsy_set_error("e2e_topk: src0 (%d rows, nc = %d), dst and the res scratch are all needed; B = %d, A = %d, max_det = %d", op.src0.C, op.nc, op.B, op.A, op.ksize);
    }
    return R.ok;
}
// DECODE (f32 logit maps in every precision mode).  act bit 0 = the fused head epilogue's DFL order, bit 1 = xyxy boxes; the msk slots hold mask coefficients
// (Segment), angle (OBB) or keypoint (Pose) logits; Pose: res = the raw keypoint tensor, an optional output
inline bool build_decode(DecodeArgs& a, const bsy_op& op, Resolver& R, const char*) {
    a.nl = op.nl; a.B = op.B; a.nc = op.nc; a.nm = op.nm; a.A = op.A; a.ne = op.ne;
    a.halves = (op.act & 1) && !op.nm && !op.ne;
    a.xyxy = (op.act >> 1) & 1;
    a.nk = op.nk; a.kdim = op.kdim;
    const bool extra = op.nm || op.ne || op.nk;
    for (int l = 0; l < op.nl && l < BSY_MAX_LEVELS; ++l) {
        a.box[l] = R.f(op.box[l]); a.cls[l] = R.f(op.cls[l]); a.msk[l] = extra ? R.f(op.msk[l]) : nullptr;
        a.ldb[l] = op.box[l].ld; a.ldc[l] = op.cls[l].ld; a.ldm[l] = extra ? op.msk[l].ld : 0;
        a.h[l] = op.lvl_h[l]; a.w[l] = op.lvl_w[l]; a.stride[l] = op.lvl_stride[l];
    }
    a.y = R.base(op.dst); a.y_dtype = op.out_dtype;
    if (op.nk) a.kraw = R.optional(op.res);
    return R.ok;
}

// ---- fp32 storage (bsy_op.prec 1 / 2): f32 views, kernels of ref32.hip ----------------------------------------------------------
// CONV and CONV_FIRST (src0 = the BCHW image of in_dtype).  prec 2 (fp32x) adds the split-f16 planes behind the f32 matrix.
inline bool build_conv32(Conv32Args& a, const bsy_op& op, Resolver& R, const char* wb) {
    if (op.out_f32 >= 2) { bsy_set_error("fp32 mode: fused Detect decoder ops are not part of fp32 plans"); return false; }
    a.first = op.kind == BSY_OP_CONV_FIRST;
    a.src0 = a.first ? (const void*)R.base(op.src0) : (const void*)R.f(op.src0);
    a.src_dtype = op.in_dtype;
    a.src1 = R.f(op.src1);
    a.ld0 = op.src0.ld; a.ld1 = op.src1.buf >= 0 ? op.src1.ld : 0;
    a.C0 = op.src0.C; a.C1 = op.src1.buf >= 0 ? op.src1.C : 0;
    a.up0 = op.up0; a.up1 = op.up1;
    a.B = op.B; a.H = op.H; a.W = op.W; a.OH = op.OH; a.OW = op.OW; a.ks = op.ksize; a.stride = op.stride; a.pad = op.pad;
    a.w = (const float*)(wb + op.w_off); a.bias = (const float*)(wb + op.b_off);
    a.dst = R.f(op.dst); a.ldd = op.dst.ld; a.Cout = op.dst.C;
    a.res = R.f(op.res); a.ldr = op.res.buf >= 0 ? op.res.ld : 0;
    a.act = op.act; a.dst_scale = op.dst_scale > 0 ? op.dst_scale : 1; a.dst_dy = op.dst_dy; a.dst_dx = op.dst_dx;
    if (op.prec == 2) {
        // byte offsets of the two f16 weight planes the record carries behind its f32 matrix (weights.py pack_record):
        // [f32 K x Cout][pad to 256][hi: Cout x Kpad f16][pad to 256][lo: Cout x Kpad f16], Kpad = K rounded up to 32
        const size_t K = (size_t)a.ks * a.ks * (a.C0 + a.C1), kpad = (K + 31) & ~(size_t)31;
        const size_t hi_off = align256(K * a.Cout * 4), lo_off = hi_off + align256((size_t)a.Cout * kpad * 2);
        a.wx_hi = (const half_t*)(wb + op.w_off + hi_off);
        a.wx_lo = (const half_t*)(wb + op.w_off + lo_off);
        a.wx_kpad = (int)kpad;
    }
    return R.ok;
}
// DWCONV (3x3 s1, SiLU on all channels or none, optional residual) and DWCONV_G
inline bool build_dw32(Dw32Args& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.src = R.f(op.src0); a.lds = op.src0.ld; a.B = op.B; a.H = op.H; a.W = op.W; a.C = op.src0.C; a.OH = op.OH; a.OW = op.OW;
    a.dst = R.f(op.dst); a.ldd = op.dst.ld;
    if (op.kind == BSY_OP_DWCONV_G) {
        dwg_fields(a, op, wb);
    } else {
        a.kh = a.kw = 3; a.stride = 1; a.wld = op.src0.C;
        a.w = (const float*)(wb + op.w_off); a.b = (const float*)(wb + op.b_off); a.act_c = op.act ? op.src0.C : 0;
        a.res = R.f(op.res); a.ldr = op.res.buf >= 0 ? op.res.ld : 0;
    }
    return R.ok;
}
inline bool build_ela32(ElaArgs& a, const float*& src, float*& dst, const bsy_op& op, Resolver& R, const char* wb) {  // a.src / a.dst unused
    ela_fields(a, op, R, wb);
    src = R.f(op.src0); dst = R.f(op.dst);
    return R.ok;
}

// ---- fp16 storage (bsy_op.prec 0) -------------------------------------------------------------------------------------------------
inline bool build_conv_first(ConvFirstArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.img = R.base(op.src0); a.img_dtype = op.in_dtype;
    a.B = op.B; a.H = op.H; a.W = op.W; a.OH = op.OH; a.OW = op.OW;
    a.ksize = op.ksize; a.stride = op.stride; a.pad = op.pad;
    a.w = (const void*)(wb + op.w_off); a.b = (const float*)(wb + op.b_off);
    a.dst = R.h(op.dst); a.ldd = op.dst.ld; a.Cout = op.dst.C; a.act = op.act;
    return R.ok;
}
// FIRST_POOL: CONV_FIRST's record with ksize / stride / pad = the conv's (3, 1, 1) and (OH, OW) = the POOLED extent the destination has
inline bool build_first_pool(ConvFirstArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    if (!build_conv_first(a, op, R, wb)) return false;
    a.pool = 1; a.OH = op.H; a.OW = op.W;
    if (op.stride != 1 || op.OH != op.H / 2 || op.OW != op.W / 2 || (op.H & 1) || (op.W & 1)) {
        R.ok = false;
        bsy_set_error("first_pool: a stride-1 conv on an even image, pooled to half its extent (got s=%d, %d x %d -> %d x %d)", op.stride, op.H, op.W, op.OH, op.OW);
    }
    return R.ok;
}
inline bool build_stem(StemArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.img = R.base(op.src0); a.img_dtype = op.in_dtype;
    a.B = op.B; a.H = op.H; a.W = op.W; a.OH = op.OH; a.OW = op.OW;
    a.w0 = (const void*)(wb + op.w_off); a.b0 = (const float*)(wb + op.b_off);
    a.w1 = (const void*)(wb + op.w2_off); a.b1 = (const float*)(wb + op.b2_off);
    a.C0 = op.mid_c; a.C1 = op.dst.C;
    int cp = 0;
    bsy_conv_packed_dims(a.C1, a.C0, 3, &cp, &a.Kpad1);
    a.dst = R.h(op.dst); a.ldd = op.dst.ld; a.act = op.act;
    return R.ok;
}
inline bool build_bneck(BneckArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.src = R.h(op.src0); a.lds = op.src0.ld; a.B = op.B; a.H = op.H; a.W = op.W;
    a.C = op.dst.C; a.CH = op.mid_c;
    a.w1 = (const void*)(wb + op.w_off); a.b1 = (const float*)(wb + op.b_off);
    a.w2 = (const void*)(wb + op.w2_off); a.b2 = (const float*)(wb + op.b2_off);
    int cp = 0;
    bsy_conv_packed_dims(a.CH, a.C, 3, &cp, &a.Kpad1);
    bsy_conv_packed_dims(a.C, a.CH, 3, &cp, &a.Kpad2);
    a.dst = R.h(op.dst); a.ldd = op.dst.ld; a.act = op.act;
    return R.ok;
}
inline bool build_s2d(const void*& img, half_t*& dst, const bsy_op& op, Resolver& R) {
    img = R.base(op.src0); dst = R.h(op.dst);
    return R.ok;
}
inline bool build_c3k2(C3k2Args& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.src = R.h(op.src0); a.lds = op.src0.ld; a.B = op.B; a.H = op.H; a.W = op.W;
    a.Cin = op.src0.C; a.C = op.mid_c; a.C2 = op.dst.C;
    a.w1 = wb + op.aux_off[0]; a.b1 = (const float*)(wb + op.aux_off[1]);
    a.wa = wb + op.aux_off[2]; a.ba = (const float*)(wb + op.aux_off[3]);
    a.wb = wb + op.aux_off[4]; a.bb = (const float*)(wb + op.aux_off[5]);
    a.w4 = wb + op.aux_off[6]; a.b4 = (const float*)(wb + op.aux_off[7]);
    a.dst = R.h(op.dst); a.ldd = op.dst.ld;
    return R.ok;
}
inline bool build_dwpw(DwPwArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.src = R.h(op.src0); a.lds = op.src0.ld; a.B = op.B; a.H = op.H; a.W = op.W; a.C = op.src0.C;
    a.dww = (const float*)(wb + op.w_off); a.dwb = (const float*)(wb + op.b_off);
    a.wgt = (const void*)(wb + op.w2_off); a.bias = (const float*)(wb + op.b2_off);
    a.dst = R.h(op.dst); a.ldd = op.dst.ld; a.Cout = op.dst.C; a.act = op.act;
    return R.ok;
}
// GHOST: mid_c = the hidden width CH (dst and res are [y | z], 2 CH channels); (w, b) = cv1 packed 1x1, (w2, b2) = cv2 depthwise f32 [25][CH];
// ksize / stride / pad describe cv2 and are fixed
inline bool build_ghost(GhostArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.src = R.h(op.src0); a.lds = op.src0.ld; a.B = op.B; a.H = op.H; a.W = op.W; a.Cin = op.src0.C; a.CH = op.mid_c;
    a.w1 = (const half_t*)(wb + op.w_off); a.b1 = (const float*)(wb + op.b_off);
    a.w2 = (const float*)(wb + op.w2_off); a.b2 = (const float*)(wb + op.b2_off);
    a.dst = R.h(op.dst); a.ldd = op.dst.ld; a.act = op.act;
    a.res = R.h(op.res); a.ldr = op.res.buf >= 0 ? op.res.ld : 0;
    if (R.ok && (op.dst.C != 2 * op.mid_c || (op.res.buf >= 0 && op.res.C != op.dst.C) || op.ksize != 5 || op.stride != 1 || op.pad != 2 || op.up0 ||
                 op.OH != op.H || op.OW != op.W)) {
        R.ok = false;
        bsy_set_error("ghost: dst (%d) and res must have 2 x mid_c (%d) channels, cv2 is 5x5 stride 1 pad 2 on the source's extent", op.dst.C, op.mid_c);
    }
    return R.ok;
}
inline bool build_dwconv_g(DwGenArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.src = R.h(op.src0); a.lds = op.src0.ld; a.B = op.B; a.H = op.H; a.W = op.W; a.C = op.src0.C; a.OH = op.OH; a.OW = op.OW;
    dwg_fields(a, op, wb);
    a.dst = R.h(op.dst); a.ldd = op.dst.ld;
    a.ident_c0 = op.mid_c;  // first channel of an identity-kernel half (plan.py dwconv_g kind "dwg_ext"), 0 = none
    return R.ok;
}
inline bool build_pmsfa_tail(PmsfaArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.P = R.h(op.src0); a.ldp = op.src0.ld; a.x = R.h(op.res); a.ldx = op.res.ld; a.dst = R.h(op.dst); a.ldd = op.dst.ld;
    a.B = op.B; a.H = op.H; a.W = op.W; a.C = op.dst.C;
    a.w2 = (const float*)(wb + op.aux_off[0]); a.b2 = (const float*)(wb + op.aux_off[1]); a.wld2 = op.heads;
    a.w3 = (const float*)(wb + op.aux_off[2]); a.b3 = (const float*)(wb + op.aux_off[3]); a.wld3 = op.key_dim;
    a.w4 = (const half_t*)(wb + op.aux_off[4]); a.b4 = (const float*)(wb + op.aux_off[5]);
    int cp = 0;
    bsy_conv_packed_dims(a.C, a.C, 1, &cp, &a.kpad4);
    if (R.ok && (op.src0.C != a.C || op.res.C != a.C)) {
        R.ok = false;
        bsy_set_error("pmsfa_tail: P (%d), x (%d) and dst (%d) must have the same channels", op.src0.C, op.res.C, a.C);
    }
    return R.ok;
}
inline bool build_msca_spatial(MscaSpArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.src = R.h(op.src0); a.lds = op.src0.ld; a.B = op.B; a.H = op.H; a.W = op.W; a.C = op.src0.C;
    for (int i = 0; i < 9; ++i) {
        a.w[i] = (const float*)(wb + op.aux_off[2 * i]);
        a.b[i] = (const float*)(wb + op.aux_off[2 * i + 1]);
    }
    for (int i = 0; i < 4; ++i) {
        const bsy_view &bv = msca_branch(op, i), &gv = msca_stat(op, i);
        a.br[i] = R.h(bv); a.ldb[i] = bv.ld; a.gap[i] = R.h(gv); a.ldg[i] = gv.ld;
    }
    return R.ok;
}
inline bool build_ela(ElaArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    ela_fields(a, op, R, wb);
    a.src = R.h(op.src0); a.dst = R.h(op.dst);
    return R.ok;
}
inline bool build_conv(ConvArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.src0 = R.h(op.src0); a.src1 = R.h(op.src1);
    a.ld0 = op.src0.ld; a.ld1 = op.src1.buf >= 0 ? op.src1.ld : 0;
    a.C0 = op.src0.C; a.C1 = op.src1.buf >= 0 ? op.src1.C : 0;
    a.up0 = op.up0; a.up1 = op.up1;
    a.B = op.B; a.H = op.H; a.W = op.W; a.OH = op.OH; a.OW = op.OW;
    a.ksize = op.ksize; a.stride = op.stride; a.pad = op.pad;
    a.wgt = (const half_t*)(wb + op.w_off); a.bias = (const float*)(wb + op.b_off);
    a.dst = op.out_f32 ? (void*)R.f(op.dst) : (void*)R.h(op.dst);
    a.ldd = op.dst.ld; a.Cout = op.dst.C; a.out_f32 = op.out_f32;
    a.res = R.h(op.res); a.ldr = op.res.buf >= 0 ? op.res.ld : 0;
    a.act = op.act; a.dst_scale = op.dst_scale; a.dst_dy = op.dst_dy; a.dst_dx = op.dst_dx;
    if (op.out_f32 >= 2) {  // fused Detect decoder: dst = the prediction tensor y, box[0] = the level's raw map (optional)
        a.epi = op.out_f32 == 4 ? 3 : op.out_f32; a.xyxy = op.out_f32 == 4;  // mode 4: the box branch (3) storing corners
        a.out_f32 = 0; a.dst = nullptr; a.ldd = 8; a.Cout = op.nl;
        a.y = R.base(op.dst); a.y_f32 = op.out_dtype == BSY_F32; a.A = op.A; a.a0 = op.lvl_h[1]; a.nrows = op.dst.C;
        a.lvl_stride = op.lvl_stride[0];
        a.raw = R.optional(op.box[0]); a.raw_f32 = a.y_f32; a.rawC = op.box[0].C;
        if (a.epi == 3 && op.mid_c > 0) {  // box-branch tail: this op is the 3x3 conv, (w2, b2) the branch's last 1x1 conv
            a.Cout = op.mid_c;
            a.tail_wgt = (const half_t*)(wb + op.w2_off); a.tail_bias = (const float*)(wb + op.b2_off);
        }
    }
    if (op.ksplit > 0 && op.out_f32 == 0) {  // split-K (latency-mode plans): ksplit = channel slices | tap slices << 8, box[0] = the f32 slab buffer
        a.nsl_c = op.ksplit & 255; a.nsl_t = (op.ksplit >> 8) & 255;
        a.split_ws = R.f(op.box[0]);
    }
    a.cfg = op.tuned_cfg - 1;  // 0 = not tuned -> heuristic
    return R.ok;
}
inline bool build_dwconv(DwArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.src = R.h(op.src0); a.lds = op.src0.ld; a.B = op.B; a.H = op.H; a.W = op.W; a.C = op.src0.C;
    a.w = (const float*)(wb + op.w_off); a.b = (const float*)(wb + op.b_off);
    a.dst = R.h(op.dst); a.ldd = op.dst.ld; a.act = op.act;
    a.res = R.h(op.res); a.ldr = op.res.buf >= 0 ? op.res.ld : 0;
    return R.ok;
}
inline bool build_attn(AttnArgs& a, const bsy_op& op, Resolver& R, const char* wb) {
    a.qkv = R.h(op.src0); a.ld = op.src0.ld; a.B = op.B; a.N = op.H * op.W; a.heads = op.heads;
    a.key_dim = op.key_dim; a.head_dim = op.head_dim; a.scale = op.scale;
    a.out = R.h(op.dst); a.ldo = op.dst.ld;
    if (op.act) {  // act = pe folded into the epilogue, w_off / b_off = its depthwise weights (include/bsyolo.h)
        a.H = op.H; a.W = op.W;
        a.pe_w = (const float*)(wb + op.w_off); a.pe_b = (const float*)(wb + op.b_off);
    }
    return R.ok;
}
