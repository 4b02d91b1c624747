// Stand-alone operator entry points of the C ABI (include/bsyolo.h): the kernels the engine launches, reached with scalar arguments
// for per-module hooks and parity tests.  Each fills the launch arguments of its kernel family (common.h) and launches on the caller's stream.
#include <stdlib.h>

#include "common.h"

// Output extent along one axis of a conv with "same" padding k / 2 (autopad, nn/modules/conv.py:29-35)
static int same_out(int n, int k, int stride) { return (n + 2 * (k / 2) - k) / stride + 1; }

extern "C" int bsy_conv2d(const void* x, int ldx, int B, int H, int W, int C1, const void* w, const float* b, void* y,
                          int ldy, int C2, int ksize, int stride, int act, const void* res, int ldr, int y_f32,
                          bsy_stream stream) {
    if (act < 0 || act > 2) BSY_FAIL(BSY_ERR_ARG, "conv2d: act = %d (0 identity, 1 SiLU, 2 ReLU)", act);
    if (!x || !w || !b || !y) BSY_FAIL(BSY_ERR_ARG, "conv2d: null pointer");
    ConvArgs a;
    a.src0 = (const half_t*)x; a.ld0 = ldx; a.C0 = C1; a.B = B; a.H = H; a.W = W;
    a.ksize = ksize; a.stride = stride; a.pad = ksize / 2;
    a.OH = same_out(H, ksize, stride); a.OW = same_out(W, ksize, stride);
    a.wgt = (const half_t*)w; a.bias = b; a.dst = y; a.ldd = ldy; a.Cout = C2; a.out_f32 = y_f32;
    a.res = (const half_t*)res; a.ldr = ldr; a.act = act; a.dst_scale = 1;
    const char* forced = getenv("BSY_CONV_CFG");  // experiments: BSY_CONV_CFG=<tile<<4|variant>; an id that is not valid
    a.cfg = forced ? atoi(forced) : -1;           // for this shape is an error (so A/B scripts see it), unset = heuristic
    if (a.cfg >= 0 && !conv_cfg_valid(a, a.cfg)) BSY_FAIL(BSY_ERR_ARG, "conv: BSY_CONV_CFG=%d is not valid for this shape", a.cfg);
    return launch_conv(a, (hipStream_t)stream);
}

// The three fp32 conv entry points share one shape check and one filler.  The image conv has no source view: it passes C1 = ldx = 3 to
// the check and ldx = 0 to the filler.
static bool conv32_shape_ok(int B, int H, int W, int C1, int C2, int ksize, int stride, int ldx, int ldy, const float* res, int ldr) {
    return B > 0 && H > 0 && W > 0 && C1 > 0 && C2 > 0 && ksize >= 1 && (ksize & 1) && (stride == 1 || stride == 2) && ldx >= C1 && ldy >= C2 &&
           !(res && ldr < C2);
}
static Conv32Args conv32_args(const void* x, int src_dtype, int ldx, int B, int H, int W, int C1, const float* w, const float* b, float* y,
                              int ldy, int C2, int ksize, int stride, int act, const float* res, int ldr) {
    Conv32Args a;
    a.src0 = x; a.src_dtype = src_dtype; a.ld0 = ldx; a.C0 = C1; a.B = B; a.H = H; a.W = W;
    a.ks = ksize; a.stride = stride; a.pad = ksize / 2;
    a.OH = same_out(H, ksize, stride); a.OW = same_out(W, ksize, stride);
    a.w = w; a.bias = b; a.dst = y; a.ldd = ldy; a.Cout = C2; a.res = res; a.ldr = ldr; a.act = act; a.dst_scale = 1;
    return a;
}
static int launch_conv32_impl(const Conv32Args& a, int impl, bsy_stream stream) {  // impl 0: the engine's routing, 1: scalar, 2: MFMA
    if (impl == 1) return launch_conv32_scalar(a, (hipStream_t)stream);
    if (impl == 2) return launch_conv32_mfma(a, (hipStream_t)stream);
    return launch_conv32(a, (hipStream_t)stream);
}

extern "C" int bsy_conv2d_f32(const float* x, int ldx, int B, int H, int W, int C1, const float* w, const float* b, float* y, int ldy,
                              int C2, int ksize, int stride, int act, const float* res, int ldr, int impl, bsy_stream stream) {
    if (act < 0 || act > 2) BSY_FAIL(BSY_ERR_ARG, "conv2d_f32: act = %d (0 identity, 1 SiLU, 2 ReLU)", act);
    if (!x || !w || !b || !y) BSY_FAIL(BSY_ERR_ARG, "conv2d_f32: null pointer");
    if (!conv32_shape_ok(B, H, W, C1, C2, ksize, stride, ldx, ldy, res, ldr) || impl < 0 || impl > 2)
        BSY_FAIL(BSY_ERR_ARG, "conv2d_f32: bad shape");
    return launch_conv32_impl(conv32_args(x, BSY_F32, ldx, B, H, W, C1, w, b, y, ldy, C2, ksize, stride, act, res, ldr), impl, stream);
}

extern "C" int bsy_conv2d_f32x(const float* x, int ldx, int B, int H, int W, int C1, const void* w_hi, const void* w_lo, int k_pad,
                               const float* b, float* y, int ldy, int C2, int ksize, int stride, int act, const float* res, int ldr,
                               bsy_stream stream) {
    if (act < 0 || act > 2) BSY_FAIL(BSY_ERR_ARG, "conv2d_f32x: act = %d (0 identity, 1 SiLU, 2 ReLU)", act);
    if (!x || !w_hi || !w_lo || !b || !y) BSY_FAIL(BSY_ERR_ARG, "conv2d_f32x: null pointer");
    if (!conv32_shape_ok(B, H, W, C1, C2, ksize, stride, ldx, ldy, res, ldr) || k_pad < ksize * ksize * C1 || (k_pad & 31))
        BSY_FAIL(BSY_ERR_ARG, "conv2d_f32x: bad shape");
    // w = w_hi: only its alignment is looked at (conv32_mfma_supported); this entry point never runs the exact kernels
    Conv32Args a = conv32_args(x, BSY_F32, ldx, B, H, W, C1, (const float*)w_hi, b, y, ldy, C2, ksize, stride, act, res, ldr);
    a.wx_hi = (const half_t*)w_hi; a.wx_lo = (const half_t*)w_lo; a.wx_kpad = k_pad;
    return launch_conv32x_mfma(a, (hipStream_t)stream);
}

extern "C" int bsy_conv_first_f32(const void* img, int img_dtype, int B, int H, int W, const float* w, const float* b, float* y, int ldy,
                                 int C2, int ksize, int stride, int act, int impl, bsy_stream stream) {
    if (act < 0 || act > 2) BSY_FAIL(BSY_ERR_ARG, "conv_first_f32: act = %d (0 identity, 1 SiLU, 2 ReLU)", act);
    if (!img || !w || !b || !y) BSY_FAIL(BSY_ERR_ARG, "conv_first_f32: null pointer");
    if (!conv32_shape_ok(B, H, W, 3, C2, ksize, stride, 3, ldy, nullptr, 0) || impl < 0 || impl > 2 || (img_dtype != BSY_F16 && img_dtype != BSY_F32))
        BSY_FAIL(BSY_ERR_ARG, "conv_first_f32: bad shape");
    Conv32Args a = conv32_args(img, img_dtype, 0, B, H, W, 3, w, b, y, ldy, C2, ksize, stride, act, nullptr, 0);
    a.first = 1;
    return launch_conv32_impl(a, impl, stream);
}

extern "C" int bsy_attention_f32(const float* qkv, int ld, int B, int N, int heads, int key_dim, int head_dim, float scale, float* out,
                                 int ldo, int impl, bsy_stream stream) {
    if (!qkv || !out || B <= 0 || N <= 0 || impl < 0 || impl > 3) BSY_FAIL(BSY_ERR_ARG, "attention_f32: bad argument");
    if (impl == 3) return launch_attn32x(qkv, ld, B, N, heads, key_dim, head_dim, scale, out, ldo, (hipStream_t)stream);
    return launch_attn32(qkv, ld, B, N, heads, key_dim, head_dim, scale, out, ldo, (hipStream_t)stream, impl);
}

extern "C" int bsy_conv_first(const void* img, int img_dtype, int B, int H, int W, const void* w, const float* b,
                              void* y, int ldy, int C2, int ksize, int stride, int act, bsy_stream stream) {
    if (act < 0 || act > 2) BSY_FAIL(BSY_ERR_ARG, "conv_first: act = %d (0 identity, 1 SiLU, 2 ReLU)", act);
    if (!img || !w || !b || !y) BSY_FAIL(BSY_ERR_ARG, "conv_first: null pointer");
    ConvFirstArgs a;
    a.img = img; a.img_dtype = img_dtype; a.B = B; a.H = H; a.W = W; a.ksize = ksize; a.stride = stride; a.pad = ksize / 2;
    a.OH = same_out(H, ksize, stride); a.OW = same_out(W, ksize, stride);
    a.w = w; a.b = b; a.dst = (half_t*)y; a.ldd = ldy; a.Cout = C2; a.act = act;
    return launch_conv_first(a, (hipStream_t)stream);
}

extern "C" int bsy_stem_fused(const void* img, int img_dtype, int B, int H, int W, const void* w0, const float* b0, int C0,
                              const void* w1, const float* b1, int C1, void* y, int ldy, int act, bsy_stream stream) {
    if (act < 0 || act > 2) BSY_FAIL(BSY_ERR_ARG, "stem: act = %d (0 identity, 1 SiLU, 2 ReLU)", act);
    if (!img || !w0 || !b0 || !w1 || !b1 || !y) BSY_FAIL(BSY_ERR_ARG, "stem: null pointer");
    StemArgs a;
    a.img = img; a.img_dtype = img_dtype; a.B = B; a.H = H; a.W = W;
    a.OH = same_out(same_out(H, 3, 2), 3, 2); a.OW = same_out(same_out(W, 3, 2), 3, 2);  // two 3x3 stride-2 convs
    a.w0 = w0; a.b0 = b0; a.w1 = w1; a.b1 = b1; a.C0 = C0; a.C1 = C1;
    int cp = 0;
    bsy_conv_packed_dims(C1, C0, 3, &cp, &a.Kpad1);
    a.dst = (half_t*)y; a.ldd = ldy; a.act = act;
    return launch_stem_fused(a, (hipStream_t)stream);
}

extern "C" int bsy_first_pool_supported(int C2, int H, int W) { return first_pool_supported(C2, H, W) ? 1 : 0; }
extern "C" int bsy_stem_fused_supported(int C0, int C1, int H, int W) { return stem_fused_supported(C0, C1, H, W) ? 1 : 0; }

extern "C" int bsy_bottleneck_fused(const void* x, int ldx, int B, int H, int W, int C, int CH, const void* w1,
                                    const float* b1, const void* w2, const float* b2, void* y, int ldy, int act,
                                    bsy_stream stream) {
    if (act < 0 || act > 1) BSY_FAIL(BSY_ERR_ARG, "bottleneck: act = %d (this kernel takes 0 or 1, SiLU; ReLU exists in the conv, image-conv and stem calls)", act);
    if (!x || !w1 || !b1 || !w2 || !b2 || !y) BSY_FAIL(BSY_ERR_ARG, "bottleneck: null pointer");
    if (C <= 0 || CH <= 0) BSY_FAIL(BSY_ERR_ARG, "bottleneck: bad widths");
    BneckArgs a;
    a.src = (const half_t*)x; a.lds = ldx; a.B = B; a.H = H; a.W = W; a.C = C; a.CH = CH;
    a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
    int cp = 0;
    bsy_conv_packed_dims(CH, C, 3, &cp, &a.Kpad1);
    bsy_conv_packed_dims(C, CH, 3, &cp, &a.Kpad2);
    a.dst = (half_t*)y; a.ldd = ldy; a.act = act;
    return launch_bneck_fused(a, (hipStream_t)stream);
}

extern "C" int bsy_bottleneck_fused_supported(int C, int CH) { return bneck_fused_supported(C, CH) ? 1 : 0; }

extern "C" int bsy_c3k2_fused(const void* x, int ldx, int B, int H, int W, int Cin, int c, int C2, const void* w1, const float* b1,
                              const void* wa, const float* ba, const void* wb, const float* bb, const void* w4, const float* b4,
                              void* y, int ldy, bsy_stream stream) {
    C3k2Args a;
    a.src = (const half_t*)x; a.lds = ldx; a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.C = c; a.C2 = C2;
    a.w1 = w1; a.b1 = b1; a.wa = wa; a.ba = ba; a.wb = wb; a.bb = bb; a.w4 = w4; a.b4 = b4;
    a.dst = (half_t*)y; a.ldd = ldy;
    return launch_c3k2_fused(a, (hipStream_t)stream);
}

extern "C" int bsy_c3k2_fused_supported(int Cin, int c, int C2) { return c3k2_fused_supported(Cin, c, C2) ? 1 : 0; }

extern "C" int bsy_dwconv(const void* x, int ldx, int B, int H, int W, int C, int kh, int kw, int stride, const float* w,
                          int wld, const float* b, void* y, int ldy, int act, bsy_stream stream) {
    if (act < 0 || act > 1) BSY_FAIL(BSY_ERR_ARG, "dwconv: act = %d (this kernel takes 0 or 1, SiLU; ReLU exists in the conv, image-conv and stem calls)", act);
    if (kh < 1 || kw < 1 || (stride != 1 && stride != 2)) BSY_FAIL(BSY_ERR_ARG, "dwconv: bad kernel / stride");
    DwGenArgs a;
    a.src = (const half_t*)x; a.lds = ldx; a.B = B; a.H = H; a.W = W; a.C = C; a.kh = kh; a.kw = kw; a.stride = stride;
    a.OH = same_out(H, kh, stride); a.OW = same_out(W, kw, stride);
    a.w = w; a.wld = wld; a.b = b; a.dst = (half_t*)y; a.ldd = ldy; a.act_c = act ? C : 0;
    return launch_dwconv_generic(a, (hipStream_t)stream);
}

extern "C" size_t bsy_ela_scratch_bytes(int B, int H, int W, int C) {
    return (B > 0 && H > 0 && W > 0 && C > 0) ? ela_scratch_floats(H, W, C) * (size_t)B * sizeof(float) : 0;
}

extern "C" int bsy_ela(const void* x, int ldx, int B, int H, int W, int C, int k, const float* wsp, const float* wch,
                       const float* gnw, const float* gnb, const float* coef, void* scratch, void* y, int ldy,
                       bsy_stream stream) {
    if (!coef) BSY_FAIL(BSY_ERR_ARG, "ela: null coefficient pointer");
    ElaArgs a;
    a.src = (const half_t*)x; a.lds = ldx; a.B = B; a.H = H; a.W = W; a.C = C; a.k = k;
    a.wsp = wsp; a.wch = wch; a.gnw = gnw; a.gnb = gnb; a.ch_coef = coef[0]; a.sp_coef = coef[1]; a.res_coef = coef[2];
    a.scratch = (float*)scratch; a.dst = (half_t*)y; a.ldd = ldy;
    return launch_ela(a, (hipStream_t)stream);
}

extern "C" int bsy_dwpw_fused(const void* x, int ldx, int B, int H, int W, int C, const float* dww, const float* dwb,
                              const void* w, const float* b, void* y, int ldy, int C2, int act, bsy_stream stream) {
    if (act < 0 || act > 1) BSY_FAIL(BSY_ERR_ARG, "dwpw_fused: act = %d (this kernel takes 0 or 1, SiLU; ReLU exists in the conv, image-conv and stem calls)", act);
    DwPwArgs a;
    a.src = (const half_t*)x; a.lds = ldx; a.B = B; a.H = H; a.W = W; a.C = C; a.dww = dww; a.dwb = dwb; a.wgt = w; a.bias = b;
    a.dst = (half_t*)y; a.ldd = ldy; a.Cout = C2; a.act = act;
    return launch_dwpw_fused(a, (hipStream_t)stream);
}

extern "C" int bsy_dwpw_fused_supported(int C, int C2) { return dwpw_fused_supported(C, C2) ? 1 : 0; }
extern "C" int bsy_attention_supported(int key_dim, int head_dim) { return attention_supported(key_dim, head_dim) ? 1 : 0; }
extern "C" int bsy_pmsfa_tail_supported(int C) { return pmsfa_tail_supported(C) ? 1 : 0; }
extern "C" int bsy_msca_spatial_supported(int H, int W) { return msca_spatial_supported(H, W) ? 1 : 0; }
extern "C" int bsy_ghost_fused_supported(int Cin, int CH) { return ghost_fused_supported(Cin, CH) ? 1 : 0; }

extern "C" int bsy_dwconv3x3(const void* x, int ldx, int B, int H, int W, int C, const float* w, const float* b, void* y,
                             int ldy, int act, const void* res, int ldr, bsy_stream stream) {
    if (act < 0 || act > 1) BSY_FAIL(BSY_ERR_ARG, "dwconv3x3: act = %d (this kernel takes 0 or 1, SiLU; ReLU exists in the conv, image-conv and stem calls)", act);
    if (!x || !w || !b || !y) BSY_FAIL(BSY_ERR_ARG, "dwconv3x3: null pointer");
    DwArgs a;
    a.src = (const half_t*)x; a.lds = ldx; a.B = B; a.H = H; a.W = W; a.C = C; a.w = w; a.b = b;
    a.dst = (half_t*)y; a.ldd = ldy; a.act = act; a.res = (const half_t*)res; a.ldr = ldr;
    return launch_dwconv(a, (hipStream_t)stream);
}

extern "C" int bsy_sppf_pool(void* buf, int ld, int B, int H, int W, int C, bsy_stream stream) {
    if (!buf) BSY_FAIL(BSY_ERR_ARG, "sppf_pool: null pointer");
    return launch_sppf_pool((half_t*)buf, ld, B, H, W, C, (hipStream_t)stream);
}

extern "C" int bsy_pool_down(const void* x, int ldx, int xoff, void* y, int ldy, int yoff, int B, int H, int W, int C, int mode, int dtype,
                             bsy_stream stream) {
    return launch_pool_down(x, ldx, xoff, y, ldy, yoff, B, H, W, C, mode, dtype, (hipStream_t)stream);
}

extern "C" int bsy_maxpool2d(const void* x, int ldx, int xoff, void* y, int ldy, int yoff, int B, int H, int W, int C, int mode, int dtype,
                             bsy_stream stream) {
    return launch_maxpool(x, ldx, xoff, y, ldy, yoff, B, H, W, C, mode, dtype, (hipStream_t)stream);
}

extern "C" int bsy_maxsig_attn(const void* embed, int lde, const void* proj, int ldp, void* out, int ldo, int B, int H, int W, int heads, int hc,
                               const void* G, int nc, const float* bias_scale, int dtype, bsy_stream stream) {
    if (H < 1 || W < 1 || (long long)H * W > 0x7fffffff) BSY_FAIL(BSY_ERR_ARG, "maxsig: bad map size %d x %d", H, W);
    MaxSigArgs a;
    a.embed = embed; a.lde = lde; a.proj = proj; a.ldp = ldp; a.dst = out; a.ldd = ldo; a.B = B; a.HW = H * W; a.heads = heads; a.hc = hc;
    a.G = G; a.nc = nc; a.bias_scale = bias_scale; a.dtype = dtype;
    return launch_maxsig(a, (hipStream_t)stream);
}

extern "C" int bsy_cbfuse(const void* const* taps, const int* ld_taps, const int* shifts, int n_taps, const void* last, int ld_last, void* out,
                          int ld_out, int B, int H, int W, int C, int dtype, bsy_stream stream) {
    if (n_taps < 1 || n_taps > BSY_CBFUSE_MAX_TAPS) BSY_FAIL(BSY_ERR_ARG, "cbfuse: %d taps (1 to %d)", n_taps, BSY_CBFUSE_MAX_TAPS);
    if (!taps || !ld_taps || !shifts) BSY_FAIL(BSY_ERR_ARG, "cbfuse: null pointer (the host arrays of the taps)");
    CbFuseArgs a;
    for (int i = 0; i < n_taps; ++i) { a.tap[i] = taps[i]; a.ldt[i] = ld_taps[i]; a.shift[i] = shifts[i]; }
    a.n = n_taps; a.last = last; a.ldl = ld_last; a.dst = out; a.ldd = ld_out; a.B = B; a.H = H; a.W = W; a.C = C; a.dtype = dtype;
    return launch_cbfuse(a, (hipStream_t)stream);
}

extern "C" int bsy_maxsig_supported(int hc) { return maxsig_supported(hc) ? 1 : 0; }

extern "C" int bsy_attention(const void* qkv, int ld, int B, int N, int heads, int key_dim, int head_dim, float scale,
                             void* out, int ldo, bsy_stream stream) {
    if (!qkv || !out) BSY_FAIL(BSY_ERR_ARG, "attention: null pointer");
    AttnArgs a;
    a.qkv = (const half_t*)qkv; a.ld = ld; a.B = B; a.N = N; a.heads = heads; a.key_dim = key_dim; a.head_dim = head_dim;
    a.scale = scale; a.out = (half_t*)out; a.ldo = ldo;
    return launch_attention(a, (hipStream_t)stream);
}

extern "C" int bsy_attention_pe(const void* qkv, int ld, int B, int H, int W, int heads, int key_dim, int head_dim, float scale,
                                const float* pe_w, const float* pe_b, void* out, int ldo, int impl, bsy_stream stream) {
    if (!qkv || !out || (pe_w && !pe_b)) BSY_FAIL(BSY_ERR_ARG, "attention_pe: null pointer");
    if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffff) BSY_FAIL(BSY_ERR_ARG, "attention_pe: bad map size");
    AttnArgs a;
    a.qkv = (const half_t*)qkv; a.ld = ld; a.B = B; a.N = H * W; a.heads = heads; a.key_dim = key_dim; a.head_dim = head_dim;
    a.scale = scale; a.out = (half_t*)out; a.ldo = ldo;
    a.H = H; a.W = W; a.pe_w = pe_w; a.pe_b = pe_w ? pe_b : nullptr;
    return launch_attention(a, (hipStream_t)stream, impl);
}

extern "C" int bsy_detect_decode(const float* const* box, const int* ldb, const float* const* cls, const int* ldc,
                                 const float* const* msk, const int* ldm, const int* lvl_h, const int* lvl_w,
                                 const float* lvl_stride, int nl, int B, int nc, int nm, void* y, int y_dtype,
                                 bsy_stream stream) {
    return bsy_detect_decode_fmt(box, ldb, cls, ldc, msk, ldm, lvl_h, lvl_w, lvl_stride, nl, B, nc, nm, 0, y, y_dtype, stream);
}

extern "C" int bsy_detect_decode_fmt(const float* const* box, const int* ldb, const float* const* cls, const int* ldc,
                                     const float* const* msk, const int* ldm, const int* lvl_h, const int* lvl_w,
                                     const float* lvl_stride, int nl, int B, int nc, int nm, int xyxy, void* y, int y_dtype,
                                     bsy_stream stream) {
    if (!box || !ldb || !cls || !ldc || !lvl_h || !lvl_w || !lvl_stride || !y || nl < 1 || nl > BSY_MAX_LEVELS)
        BSY_FAIL(BSY_ERR_ARG, "detect_decode: bad argument");
    if (nm && (!msk || !ldm)) BSY_FAIL(BSY_ERR_ARG, "detect_decode: mask inputs missing");
    if (xyxy != 0 && xyxy != 1) BSY_FAIL(BSY_ERR_ARG, "detect_decode: xyxy = %d (0 or 1)", xyxy);
    DecodeArgs a;
    a.xyxy = xyxy;
    a.nl = nl; a.B = B; a.nc = nc; a.nm = nm;
    for (int l = 0; l < nl; ++l) {
        a.box[l] = box[l]; a.cls[l] = cls[l]; a.msk[l] = nm ? msk[l] : nullptr;
        a.ldb[l] = ldb[l]; a.ldc[l] = ldc[l]; a.ldm[l] = nm ? ldm[l] : 0;
        a.h[l] = lvl_h[l]; a.w[l] = lvl_w[l]; a.stride[l] = lvl_stride[l];
    }
    a.y = y; a.y_dtype = y_dtype;
    return launch_decode(a, (hipStream_t)stream);
}
