// Shared declarations for the gfx950 kernels of libbsyolo_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/bsyolo.h"

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- error plumbing (thread-local message, no C++ exceptions across the ABI) ----
void bsy_set_error(const char* fmt, ...);
#define BSY_FAIL(code, ...)        \
    do {                           \
        bsy_set_error(__VA_ARGS__); \
        return (code);             \
    } while (0)
#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) BSY_FAIL(BSY_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                       __FILE__, __LINE__);                                               \
    } while (0)

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return ceil_div(a, b) * b; }
static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- resolved (pointer-level) launch arguments; filled by the builders of op_args.h (the engine's op records) or by the stand-alone C
// entry points (ops_api.hip).  Every field starts zeroed: a field a filler does not mention is off, whichever filler it is. ----
struct ConvArgs {
    const half_t* src0 = nullptr;  // incl. channel offset
    const half_t* src1 = nullptr;  // second concat operand or nullptr
    int ld0 = 0, ld1 = 0;          // channels per pixel row of each source buffer
    int C0 = 0, C1 = 0;            // channels taken from each source (Cin = C0 + C1), multiples of 8
    int up0 = 0, up1 = 0;          // nearest-x2 read
    int B = 0, H = 0, W = 0, OH = 0, OW = 0;  // logical input / output extents
    int ksize = 0, stride = 0, pad = 0;
    const half_t* wgt = nullptr;   // [CoutPad][Kpad]
    const float* bias = nullptr;   // [CoutPad]
    void* dst = nullptr;           // incl. channel offset; f16 or f32
    int ldd = 0, Cout = 0, out_f32 = 0;
    const half_t* res = nullptr;   // incl. channel offset or nullptr
    int ldr = 0;
    int act = 0;
    int dst_scale = 0, dst_dy = 0, dst_dx = 0;
    int cfg = 0;  // kernel configuration id (tile << 4 | variant) chosen by the autotuner; < 0 = heuristic
    // Fused Detect decoder (epi != 0: the conv is the last layer of a head branch and writes the decoded prediction tensor
    // y (B, nrows, A) directly instead of a logit map; `dst` is then unused):
    //   epi 2: class scores  y[n, 4 + c, a0 + pix] = sigmoid(logit)                 (head.py:147)
    //   epi 3: boxes         y[n, 0..3, a0 + pix]  = dist2bbox(DFL(logits)) * stride (head.py:141-146, block.py:58-77)
    // raw (optional, may be null): the level's raw map (B, rawC, OH, OW) that Detect.forward also returns (head.py:74),
    // box logits at channels 0..63, class logits at 64...
    int epi = 0;
    void* y = nullptr;
    int y_f32 = 0, A = 0, a0 = 0, nrows = 0;
    float lvl_stride = 0.f;
    int xyxy = 0;  // epi 3: rows 0..3 are (x1, y1, x2, y2) * stride -- dist2bbox(xywh=False), an end2end head (head.py:148) -- instead of xywh
    void* raw = nullptr;
    int raw_f32 = 0, rawC = 0;
    // Box-branch tail (3x3 conv + the branch's last 1x1 conv + DFL decode in one launch; conv_patch.hip conv3x3_patch_kernel<.., TAIL>):
    // this op is the 3x3 conv (Cout = 64, its map never reaches HBM), tail_wgt / tail_bias the packed 64 -> 64 1x1 conv, epi = 3 and
    // the decoder fields above describe what the tail writes.  nullptr: no tail.
    const half_t* tail_wgt = nullptr;
    const float* tail_bias = nullptr;
    // Split-K (latency mode): nsl_c channel slices x nsl_t tap slices of the layer's K walk, computed by separate workgroups of one launch
    // into f32 slabs of split_ws (nsl_c * nsl_t * B * OH * OW * round_up(Cout, 32) floats) and summed in slice order by a second
    // launch.  0 / 1 x 0 / 1: off.  Implicit-GEMM kernel only (conv_cfg_valid).
    int nsl_c = 0, nsl_t = 0;
    float* split_ws = nullptr;
};
int launch_conv(const ConvArgs& a, hipStream_t s);
#define BSY_CONV_MAX_CFG 64
int conv_candidates(const ConvArgs& a, int* out, int max_out);  // valid configuration ids, heuristic best first
bool conv_cfg_valid(const ConvArgs& a, int cfg);
int conv_korder(const ConvArgs& a);  // the layer's K walk (0 packed order, 1 / 2 chunk-major with 32- / 64-channel chunks): a function of its shape

struct ConvFirstArgs {
    const void* img = nullptr;
    int img_dtype = 0;
    int B = 0, H = 0, W = 0, OH = 0, OW = 0, ksize = 0, stride = 0, pad = 0;
    const void* w = nullptr;   // packed f16 [CoutPad][32], k = (kh, kw, c)  (same layout as every other conv)
    const float* b = nullptr;  // [CoutPad]
    half_t* dst = nullptr;
    int ldd = 0, Cout = 0, act = 0;
    int pool = 0;  // 1 (stride 1 only): MaxPool2d(2, 2, 0) in the epilogue; OH x OW stays the conv's extent, dst is (OH / 2) x (OW / 2)
};
int launch_conv_first(const ConvFirstArgs& a, hipStream_t s);
bool first_pool_supported(int Cout, int H, int W);

// Fused stem (stem_fused.hip): image -> Conv 3x3 s2 (3 -> C0) -> Conv 3x3 s2 (C0 -> C1), layer 0 kept on chip.
struct StemArgs {
    const void* img = nullptr;
    int img_dtype = 0;
    int B = 0, H = 0, W = 0, OH = 0, OW = 0;  // image extent; OH/OW = layer-1 output extent
    const void* w0 = nullptr;  // layer 0: packed f16 [CoutPad][32]
    const float* b0 = nullptr;
    const void* w1 = nullptr;  // layer 1: packed f16 [CoutPad][Kpad1], k = (kh, kw, c)
    const float* b1 = nullptr;
    int C0 = 0, C1 = 0, Kpad1 = 0;
    half_t* dst = nullptr;
    int ldd = 0, act = 0;
};
bool stem_fused_supported(int C0, int C1, int H, int W);
int launch_stem_fused(const StemArgs& a, hipStream_t s);

// Fused Bottleneck (bneck_fused.hip): y = x + conv3x3(conv3x3(x)), hidden map kept on chip.
struct BneckArgs {
    const half_t* src = nullptr;  // (B,H,W,lds) view of C channels
    int lds = 0;
    int B = 0, H = 0, W = 0, C = 0, CH = 0;
    const void *w1 = nullptr, *w2 = nullptr;  // packed f16 [CoutPad][Kpad1] (C -> CH) and [CoutPad][Kpad2] (CH -> C)
    const float *b1 = nullptr, *b2 = nullptr;
    int Kpad1 = 0, Kpad2 = 0;
    half_t* dst = nullptr;
    int ldd = 0, act = 0;
};
bool bneck_fused_supported(int C, int CH);
int launch_bneck_fused(const BneckArgs& a, hipStream_t s);

// Fused C3k2 block (c3k2_fused.hip): out = cv2(cat(y0, y1, y1 + m.cv2(m.cv1(y1)))), [y0 | y1] = cv1(x); nothing but x and out in HBM.
struct C3k2Args {
    const half_t* src = nullptr;  // (B,H,W,lds) view of Cin channels
    int lds = 0;
    int B = 0, H = 0, W = 0, Cin = 0, C = 0, C2 = 0;  // C = hidden width c of the block (cv1 -> 2c), bottleneck hidden c/2, output C2
    // packed f16 [CoutPad][Kpad]: cv1 (Cin -> 2c), m.cv1 (c -> c/2, 3x3), m.cv2 (c/2 -> c, 3x3), cv2 (3c -> C2)
    const void *w1 = nullptr, *wa = nullptr, *wb = nullptr, *w4 = nullptr;
    const float *b1 = nullptr, *ba = nullptr, *bb = nullptr, *b4 = nullptr;
    half_t* dst = nullptr;
    int ldd = 0;
};
bool c3k2_fused_supported(int Cin, int C, int C2);
int launch_c3k2_fused(const C3k2Args& a, hipStream_t s);

// GhostConv with a 1x1 stride-1 cv1 (ghost_fused.hip): dst = [y | z] (+ res), y = act(cv1 x), z = act(cv2 y), cv2 depthwise 5x5; y only on chip
// between the two convs.
struct GhostArgs {
    const half_t* src = nullptr;  // (B,H,W,lds) view of Cin channels
    int lds = 0;
    int B = 0, H = 0, W = 0, Cin = 0, CH = 0;  // CH = hidden width: cv1 Cin -> CH, cv2 depthwise on CH, dst / res 2 CH channels
    const half_t* w1 = nullptr;  // cv1: packed f16 [CoutPad][Kpad]
    const float* b1 = nullptr;
    const float* w2 = nullptr;   // cv2: f32 [25][CH]
    const float* b2 = nullptr;   // f32 [CH]
    half_t* dst = nullptr;
    int ldd = 0, act = 0;
    const half_t* res = nullptr;  // shortcut operand (2 CH channels) or nullptr; may be dst's view
    int ldr = 0;
};
bool ghost_fused_supported(int Cin, int CH);
int launch_ghost_fused(const GhostArgs& a, hipStream_t s);

// ---- BS-YOLO-only modules (bsyolo_ops.hip) ----------------------------------------------------------------------------
struct DwGenArgs {       // depthwise kh x kw, stride 1 / 2, "same" padding, + bias (+SiLU)
    const half_t* src = nullptr;
    int lds = 0;
    int B = 0, H = 0, W = 0, C = 0, OH = 0, OW = 0, kh = 0, kw = 0, stride = 0;
    const float* w = nullptr;  // [kh*kw][wld] (already offset to this launch's first channel)
    int wld = 0;
    const float* b = nullptr;
    half_t* dst = nullptr;
    int ldd = 0, act_c = 0;    // SiLU on channels [0, act_c) of this launch, identity on the rest
    int ident_c0 = 0;    // > 0: channels [ident_c0, C) carry an identity kernel (centre tap 1, bias 0: PMSFA.conv3's pass-through half,
                         // weights.py "dwg_ext") -- the tiled kernels write x + 0 for them, which is what the full tap loop returns
};
int launch_dwconv_generic(const DwGenArgs& a, hipStream_t s);
struct PmsfaArgs {       // PMSFA's tail in one launch (pmsfa_fused.hip): dst = conv4([conv3(conv2(p1)[:C/4]) | conv2(p1)[C/4:] | p2]) + x, P = [p1 | p2] = conv1(x)
    const half_t* P = nullptr;   // conv1's output, C channels
    int ldp = 0;
    const half_t* x = nullptr;   // the module's input (shortcut operand), C channels
    int ldx = 0;
    half_t* dst = nullptr;
    int ldd = 0;
    int B = 0, H = 0, W = 0, C = 0;
    const float* w2 = nullptr;   // conv2: depthwise 5x5 on C/2 channels, f32 [25][wld2]
    const float* b2 = nullptr;
    int wld2 = 0;
    const float* w3 = nullptr;   // conv3: depthwise 7x7 on C/4 channels, f32 [49][wld3]
    const float* b3 = nullptr;
    int wld3 = 0;
    const half_t* w4 = nullptr;  // conv4: packed 1x1 weights [cout][kpad4]
    const float* b4 = nullptr;
    int kpad4 = 0;
};
bool pmsfa_tail_supported(int C);
int launch_pmsfa_tail(const PmsfaArgs& a, hipStream_t s);
int launch_copy_view(const half_t* src, int lds_, int up, int B, int H, int W, int C, half_t* dst, int ldd, hipStream_t s);
int launch_gap(const half_t* src, int lds_, int B, int H, int W, int C, half_t* out, int ldo, hipStream_t s);
struct MscaSpArgs {
    const half_t* src = nullptr;
    int lds = 0, B = 0, H = 0, W = 0, C = 0;
    const float* w[9] = {};  // conv0, conv0_1, conv0_2, conv1_1, conv1_2, conv2_1, conv2_2, conv3_1, conv3_2
    const float* b[9] = {};
    half_t* br[4] = {};
    int ldb[4] = {};
    half_t* gap[4] = {};
    int ldg[4] = {};
};
bool msca_spatial_supported(int H, int W);
int launch_msca_spatial(const MscaSpArgs& a, hipStream_t s);
struct MixArgs {
    const half_t* br[4] = {};
    int ldb[4] = {};
    const float* lg[4] = {};  // branch logits (B, ldl) f32
    int ldl[4] = {};
    int B = 0, HW = 0, C = 0;
    half_t* dst = nullptr;
    int ldd = 0;
};
int launch_msca_mix(const MixArgs& a, hipStream_t s);
int launch_mul(const half_t* a, int lda, const half_t* b, int ldb, long long npix, int C, half_t* dst, int ldd, hipStream_t s);
int launch_add(const half_t* a, int lda, const half_t* b, int ldb, long long npix, int C, half_t* dst, int ldd, hipStream_t s);  // dst may be a
struct ElaArgs {
    const half_t* src = nullptr;
    int lds = 0;
    int B = 0, H = 0, W = 0, C = 0, k = 0;
    // spatial_conv [C][k], ch_att conv [C][k], GroupNorm weight / bias [C]
    const float *wsp = nullptr, *wch = nullptr, *gnw = nullptr, *gnb = nullptr;
    float ch_coef = 0.f, sp_coef = 0.f, res_coef = 0.f;  // sigmoid(ch_weight), sigmoid(sp_weight), sigmoid(res_weight)
    float* scratch = nullptr;                            // ela_scratch_floats(H, W, C) * B floats
    half_t* dst = nullptr;
    int ldd = 0;
};
size_t ela_scratch_floats(int H, int W, int C);
int launch_ela(const ElaArgs& a, hipStream_t s);
int launch_ela_gate(const ElaArgs& a, hipStream_t s);

// ---- fp32 correctness mode (ref32.hip): plans with bsy_op.prec == 1; NHWC f32 views --------------------------------------------
struct Conv32Args {
    const void* src0 = nullptr;  // f32 view, or (first) the BCHW image in src_dtype
    const void* src1 = nullptr;
    int src_dtype = 0, first = 0;
    int ld0 = 0, ld1 = 0, C0 = 0, C1 = 0, up0 = 0, up1 = 0;
    int B = 0, H = 0, W = 0, OH = 0, OW = 0, ks = 0, stride = 0, pad = 0;
    const float* w = nullptr;     // f32 [k*k*Cin][Cout], k = (kh, kw, cin)
    const float* bias = nullptr;  // f32 [Cout]
    float* dst = nullptr;
    int ldd = 0, Cout = 0;
    const float* res = nullptr;
    int ldr = 0, act = 0, dst_scale = 0, dst_dy = 0, dst_dx = 0;
    // fp32x mode (conv32x_mfma.hip): the same weights split into two f16 planes [Cout][wx_kpad], w = hi + lo, K padded to 32
    // with zeros; nullptr = the exact fp32 kernels only
    const half_t* wx_hi = nullptr;
    const half_t* wx_lo = nullptr;
    int wx_kpad = 0;
};
int launch_conv32(const Conv32Args& a, hipStream_t s);          // routes to the MFMA kernel where it applies, else the scalar one
bool conv32x_mfma_supported(const Conv32Args& a);               // conv32x_mfma.hip: split-f16 operands, three f16 MFMAs per product
int launch_conv32x_mfma(const Conv32Args& a, hipStream_t s);
int launch_conv32_scalar(const Conv32Args& a, hipStream_t s);   // ref32.hip: one thread per output, sequential fmaf chain
bool conv32_mfma_supported(const Conv32Args& a);                // conv32_mfma.hip: v_mfma_f32_32x32x2_f32, the same chain bit for bit
int launch_conv32_mfma(const Conv32Args& a, hipStream_t s);
struct Dw32Args {
    const float* src = nullptr;
    int lds = 0, B = 0, H = 0, W = 0, C = 0, OH = 0, OW = 0, kh = 0, kw = 0, stride = 0;
    const float* w = nullptr;  // f32 [kh*kw][wld]
    int wld = 0;
    const float* b = nullptr;
    float* dst = nullptr;
    int ldd = 0, act_c = 0;
    const float* res = nullptr;
    int ldr = 0;
};
int launch_dw32(const Dw32Args& a, hipStream_t s);
struct Mix32Args {
    const float* br[4] = {};
    int ldb[4] = {};
    const float* lg[4] = {};
    int ldl[4] = {};
    int B = 0, HW = 0, C = 0;
    float* dst = nullptr;
    int ldd = 0;
};
int launch_mix32(const Mix32Args& a, hipStream_t s);
int launch_sppf32(float* buf, int ld, int B, int H, int W, int C, hipStream_t s);
int launch_attn32(const float* qkv, int ld, int B, int N, int heads, int kd, int hd, float scale, float* out, int ldo, hipStream_t s,
                  int impl = 0);  // impl 0: tiled kernel where it applies (key_dim 32, head_dim 64), 1: generic kernel, 2: tiled or error
bool attn32x_supported(int ld, int ldo, int kd, int hd, const void* qkv, const void* out);  // attention32x.hip (fp32x mode)
int launch_attn32x(const float* qkv, int ld, int B, int N, int heads, int kd, int hd, float scale, float* out, int ldo, hipStream_t s);
int launch_nhwc2nchw32(const float* src, int ld, int B, int C, int hw, void* out, int out_dtype, hipStream_t s);
int launch_copy32(const float* src, int lds_, int up, int B, int H, int W, int C, float* dst, int ldd, hipStream_t s);
int launch_gap32(const float* src, int lds_, int B, int H, int W, int C, float* out, int ldo, hipStream_t s);
int launch_mul32(const float* x, int ldx, const float* y, int ldy, long long npix, int C, float* dst, int ldd, hipStream_t s);
int launch_add32(const float* x, int ldx, const float* y, int ldy, long long npix, int C, float* dst, int ldd, hipStream_t s);  // dst may be x
int launch_ela32(const ElaArgs& a, const float* src, float* dst, hipStream_t s);  // a.src / a.dst unused

// Fused DWConv 3x3 (+SiLU) -> Conv 1x1 (+act) (dwpw_fused.hip: dwpw_fused_kernel)
struct DwPwArgs {
    const half_t* src = nullptr;
    int lds = 0;
    int B = 0, H = 0, W = 0, C = 0;
    const float *dww = nullptr, *dwb = nullptr;  // depthwise f32 [9][C], [C]
    const void* wgt = nullptr;                   // 1x1 packed f16 [CoutPad][Kpad]
    const float* bias = nullptr;
    half_t* dst = nullptr;
    int ldd = 0, Cout = 0, act = 0;
};
bool dwpw_fused_supported(int C, int Cout);
int launch_dwpw_fused(const DwPwArgs& a, hipStream_t s);

struct DwArgs {
    const half_t* src = nullptr;
    int lds = 0;
    int B = 0, H = 0, W = 0, C = 0;
    const float* w = nullptr;  // [9][C]
    const float* b = nullptr;
    half_t* dst = nullptr;
    int ldd = 0;
    int act = 0;
    const half_t* res = nullptr;
    int ldr = 0;
};
int launch_dwconv(const DwArgs& a, hipStream_t s);
int launch_sppf_pool(half_t* buf, int ld, int B, int H, int W, int C, hipStream_t s);
// pool_down.hip: src / dst = first element of the buffers, soff / doff = first channel of the views; dtype BSY_F16 / BSY_F32
int launch_pool_down(const void* src, int lds_, int soff, void* dst, int ldd, int doff, int B, int H, int W, int C, int mode, int dtype,
                     hipStream_t s);
// maxpool.hip: the same calling convention; mode 0 = MaxPool2d(2, 2, 0), 1 = ZeroPad2d((0, 1, 0, 1)) + MaxPool2d(2, 1, 0)
int launch_maxpool(const void* src, int lds_, int soff, void* dst, int ldd, int doff, int B, int H, int W, int C, int mode, int dtype,
                   hipStream_t s);
int launch_s2d(const void* img, int img_dtype, int B, int H, int W, half_t* dst, int ldd, hipStream_t s);

// maxsig.hip: MaxSigmoidAttnBlock's gate (block.py:3483-3515), dst = proj * scale[m] * sigmoid(max_n <embed, G[n]>_head m + bias[m]).  Views of
// `dtype` (BSY_F16 / BSY_F32) over B * HW pixels; arguments as bsy_maxsig_attn's, checked in the launcher (the engine's op and the entry
// point share the checks)
struct MaxSigArgs {
    const void* embed = nullptr;
    const void* proj = nullptr;
    void* dst = nullptr;
    int lde = 0, ldp = 0, ldd = 0;
    int B = 0, HW = 0, heads = 0, hc = 0, nc = 0;
    const void* G = nullptr;          // [rows][heads * hc] of dtype; f16: rows = nc rounded up to 32, the padding rows copies of row 0
    const float* bias_scale = nullptr;  // [bias (heads) | scale (heads)]
    int dtype = 0;
};
inline bool maxsig_supported(int hc) { return hc >= 16 && hc <= 128 && hc % 16 == 0; }  // the fp16 kernel's head widths: 1 .. 8 k-steps of 16
int launch_maxsig(const MaxSigArgs& a, hipStream_t s);

// cbfuse.hip: CBFuse (block.py:3760-3772), dst = tap 0 + ... + tap n-1 + last in f32, in that order; tap i stored at (H >> shift, W >> shift).
// Pointers include the channel offset; views of `dtype` (BSY_F16 / BSY_F32).  dst may be `last` itself and must not overlap a tap.
struct CbFuseArgs {
    const void* tap[BSY_CBFUSE_MAX_TAPS] = {};
    int ldt[BSY_CBFUSE_MAX_TAPS] = {}, shift[BSY_CBFUSE_MAX_TAPS] = {};
    int n = 0;
    const void* last = nullptr;
    void* dst = nullptr;
    int ldl = 0, ldd = 0, B = 0, H = 0, W = 0, C = 0, dtype = 0;
};
// tap count 1 .. 5, shifts 0 .. 4 that divide H and W; sets the error text.  What both callers check without a pointer (the engine's record
// through op_args.h cbfuse_record_ok, the launcher for the entry point)
inline bool cbfuse_shape_ok(int n, const int* shift, int H, int W) {
    if (n < 1 || n > BSY_CBFUSE_MAX_TAPS) { bsy_set_error("cbfuse: %d taps (1 to %d)", n, BSY_CBFUSE_MAX_TAPS); return false; }
    if (H < 1 || W < 1) { bsy_set_error("cbfuse: bad map size %d x %d", H, W); return false; }
    for (int i = 0; i < n; ++i) {
        if (shift[i] < 0 || shift[i] > 4) { bsy_set_error("cbfuse: tap %d has shift %d (0 to 4)", i, shift[i]); return false; }
        if (H % (1 << shift[i]) || W % (1 << shift[i])) {
            bsy_set_error("cbfuse: tap %d: %d x %d is not divisible by %d", i, H, W, 1 << shift[i]);
            return false;
        }
    }
    return true;
}
int launch_cbfuse(const CbFuseArgs& a, hipStream_t s);

struct AttnArgs {
    const half_t* qkv = nullptr;
    int ld = 0;
    int B = 0, N = 0, heads = 0, key_dim = 0, head_dim = 0;
    float scale = 0.f;
    half_t* out = nullptr;
    int ldo = 0;
    // pe (block.py:4286 `+ self.pe(v)`) folded into the epilogue: depthwise 3x3 + bias on v over the H x W map (H * W = N), added to
    // the attention output as dwconv3x3_kernel<false, true> adds it.  pe_w f32 [9][heads * head_dim], pe_b f32 [heads * head_dim]; null: no pe
    int H = 0, W = 0;
    const float* pe_w = nullptr;
    const float* pe_b = nullptr;
};
int launch_attention(const AttnArgs& a, hipStream_t s, int impl = 0);  // impl 0 auto / 1 resident / 2 streaming (attention.hip)
bool attention_supported(int key_dim, int head_dim);

struct DecodeArgs {
    const float* box[BSY_MAX_LEVELS] = {};
    const float* cls[BSY_MAX_LEVELS] = {};
    const float* msk[BSY_MAX_LEVELS] = {};
    int ldb[BSY_MAX_LEVELS] = {}, ldc[BSY_MAX_LEVELS] = {}, ldm[BSY_MAX_LEVELS] = {};
    int h[BSY_MAX_LEVELS] = {}, w[BSY_MAX_LEVELS] = {};
    float stride[BSY_MAX_LEVELS] = {};
    int nl = 0, B = 0, nc = 0, nm = 0, A = 0;
    void* y = nullptr;
    int y_dtype = 0;
    int ne = 0;  // OBB angle channels (0 / 1): msk[l] then holds the angle logits and nm is 0
    int halves = 0;  // 1: the DFL sums run in the fused head epilogue's order at every level count (a Detect plan whose decode launch stands
                     // in for the fused head, bsy_op.act); 0: that order for heads of four levels only, bin order up to three
    int nk = 0, kdim = 0;  // Pose keypoint channels (nkpt * kdim; 0: none) and channels per keypoint (2 / 3): msk[l] then holds the level's keypoint
                           // logits (nm = ne = 0); y gets nk decoded rows behind the scores (Pose.kpts_decode, kpt_decode.h)
    void* kraw = nullptr;  // nk: (B, nk, A) tensor of y's dtype for the undecoded logits, or null
    int xyxy = 0;  // 1: rows 0..3 are (x1, y1, x2, y2) * stride, the box form of an end2end head (dist2bbox(xywh=False), head.py:148); nm = ne = nk = 0
};
int launch_decode(const DecodeArgs& a, hipStream_t s);
// val_match.hip: the validator's matching rule on an IoU matrix (B, Lmax, max_det) made elsewhere (val_masks.hip); arguments as
// bsy_val_match's, already validated by the caller
int val_match_from_iou(const float* iou, const float* det, int row, const int32_t* counts, int B, int max_det, const float* gt_cls,
                       const int32_t* gt_counts, int Lmax, const float* iouv_host, int n_iou, unsigned char* out, hipStream_t s);
int launch_nhwc2nchw(const half_t* src, int ld, int B, int C, int hw, void* out, int out_dtype, hipStream_t s);
int launch_raw_nchw(const float* box, int ldb, const float* cls, int ldc, int B, int h, int w, int nc, void* out,
                    int out_dtype, hipStream_t s);
// classify.hip: Classify's tail (head.py:300-304) -- row softmax of the f32 logit map, the logits in out_dtype and the k most
// probable classes, one launch; arguments as bsy_classify_tail's, checked here (the engine's op and the entry point share the bounds)
int launch_classify_tail(const float* logits, int ld, int B, int nc, void* y, void* x, int out_dtype, int k, int32_t* topk_idx,
                         float* topk_val, hipStream_t s);

// WHY these exist (round 1): the natural form `fmaf((float)h[j], w[j], a[j])` compiles to
// v_cvt_f32_f16 (SDWA WORD_1 for the odd elements) feeding SLP-packed v_pk_fma_f32 -- and that sequence returned wrong
// odd elements, sporadically, whenever MFMA kernels of another stream shared the CUs (SCDown's depthwise conv: 26 of 48
// forwards; 0 of 48 with packing off).  Depthwise kernels therefore use v_fma_mix_f32 (no conversion, no packing) and
// the whole library is built with -fno-slp-vectorize (build.py).
// acc + f32(h) * w with ONE instruction per element: v_fma_mix_f32 reads the f16 operand (low / high half of a packed
// register) directly, so a depthwise tap costs 8 VALU issues per 8 channels instead of 8 v_cvt_f32_f16 + 4 v_pk_fma_f32
// (and packed f32 math is the slower choice beside MFMAs).  Same value as fmaf((float)h, w, acc): the conversion is exact.
__device__ __forceinline__ float fma_mix_lo(unsigned hpair, float w, float acc) {
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hpair), "v"(w), "v"(acc));
    return r;
}
__device__ __forceinline__ float fma_mix_hi(unsigned hpair, float w, float acc) {
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hpair), "v"(w), "v"(acc));
    return r;
}
// element J (compile-time) of a half8 register quadruple
template <int J>
__device__ __forceinline__ float fma_mix_e(const half8& v, float w, float acc) {
    union { half8 h; unsigned u[4]; } x;
    x.h = v;
    return (J & 1) ? fma_mix_hi(x.u[J >> 1], w, acc) : fma_mix_lo(x.u[J >> 1], w, acc);
}
// a[0..7] += f32(v[0..7]) * (w0, w1)
__device__ __forceinline__ void fma_mix8(float (&a)[8], const half8& v, const f32x4& w0, const f32x4& w1) {
    union { half8 h; unsigned u[4]; } x;
    x.h = v;
    a[0] = fma_mix_lo(x.u[0], w0[0], a[0]); a[1] = fma_mix_hi(x.u[0], w0[1], a[1]);
    a[2] = fma_mix_lo(x.u[1], w0[2], a[2]); a[3] = fma_mix_hi(x.u[1], w0[3], a[3]);
    a[4] = fma_mix_lo(x.u[2], w1[0], a[4]); a[5] = fma_mix_hi(x.u[2], w1[1], a[5]);
    a[6] = fma_mix_lo(x.u[3], w1[2], a[6]); a[7] = fma_mix_hi(x.u[3], w1[3], a[7]);
}

// Loads through a buffer descriptor (round 3): a lane whose voffset is out of range (>= num_records = `bytes`) receives ZEROS, so
// padding taps, pixels past the map, couts past Cout and K tails need neither a branch around the load nor a zero-initialised
// destination, and the address is a 32-bit offset instead of a 64-bit pointer per lane.  The host pass only needs the launch stubs.
#if defined(__HIP_DEVICE_COMPILE__)
typedef __amdgpu_buffer_rsrc_t bsy_rsrc_t;
__device__ __forceinline__ bsy_rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
// 16 bytes at base + voff as T (half8, f32x4)
template <typename T>
__device__ __forceinline__ T buf_load16(bsy_rsrc_t r, unsigned voff) {
    static_assert(sizeof(T) == 16, "buf_load16: 16-byte type");
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    union { u32x4 u; T t; } v;
    v.u = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, 0, 0);
    return v.t;
}
#else
typedef int bsy_rsrc_t;
__device__ __forceinline__ bsy_rsrc_t make_rsrc(const void*, unsigned) { return 0; }
template <typename T>
__device__ __forceinline__ T buf_load16(bsy_rsrc_t, unsigned) { return T{}; }
#endif
// voffsets out of range for every descriptor (num_records < 2^32 - 32): BSY_OOB for a single 16-byte read, BSY_OOB_PAIR for a
// 32-byte piece read as two halves at voff and voff + 16 (the second half stays out of range)
#define BSY_OOB 0xFFFFFFF0u
#define BSY_OOB_PAIR 0xFFFFFFE0u

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for vmcnt(0) -- every global load and STORE the
// wave has in flight -- so in a persistent tile loop each barrier after a prefetch or behind the tile's output stores exposed a
// full HBM round trip (round 3, SQ counters of the fused kernels: 44-60 % of the wave cycles spent waiting).  Registers filled
// by a prefetch are still safe to use: the compiler places its own counted vmcnt wait in front of their first use.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// XCD-aware, bijective block remap: blocks that share an XCD (bid % 8) get consecutive logical tiles, so the cout tiles of one
// pixel tile re-read the pixel operand from that XCD's L2.
__device__ __forceinline__ int xcd_remap(int bid, int nb) {
    const int q = nb >> 3, r = nb & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// Tile walk of a persistent workgroup, XCD-aware.  Workgroup b of a grid of G lands on XCD b % 8 (round-robin dispatch): with the
// plain walk (tile = b, b + G, ...) the four / eight spatial neighbours of a tile run on OTHER XCDs, so the halo every fused kernel
// re-reads (the C3k2 block reads its input 2.5 times) misses the XCD's L2 each time: PMC traffic of the block 927 MB for 629 MB.
// Here XCD x owns one contiguous eighth of the tiles and its workgroups walk it side by side: at any moment an XCD works on ~G / 8
// consecutive tiles -- a few tile rows of one image -- and the halos hit its L2.
struct TileWalk {
    int tile, step, end;
};
__device__ __forceinline__ TileWalk xcd_tile_walk(int b, int G, int ntiles) {
    const int X = G < 8 ? G : 8;
    const int x = b % X, i = b / X;
    const int gx = (G - x + X - 1) / X;          // workgroups on this XCD
    const int q = ntiles / X, r = ntiles % X;
    const int start = x * q + (x < r ? x : r);
    return TileWalk{start + i, gx, start + q + (x < r ? 1 : 0)};
}

// Tile grid of a persistent fused kernel: B images x tiles_y x tiles_x tiles, tile index = (n * tiles_y + ty) * tiles_x + tx.  The
// kernel divides by multiply-high with host-made magics; a kernel-argument struct holds these five fields last, in this order.
struct TileGrid {
    int tiles_x, tiles_y, ntiles;
    unsigned magic_x, magic_y;  // ceil(2^32 / tiles_x), ceil(2^32 / tiles_y): exact quotients for tile < 2^32 / divisor
};
// Grid of th x tw tiles over B images of H x W (H, W positive).  Each side is padded to at least two tiles, as the magic for
// divisor 1 would be 2^32; the extra tiles lie outside the map and store nothing.
static inline int make_tile_grid(TileGrid& g, int B, int H, int W, int th, int tw, const char* who) {
    g.tiles_x = ceil_div(W, tw);
    g.tiles_y = ceil_div(H, th);
    if (g.tiles_x < 2) g.tiles_x = 2;
    if (g.tiles_y < 2) g.tiles_y = 2;
    const long long nt = (long long)B * g.tiles_x * g.tiles_y;
    if (nt <= 0 || nt * (g.tiles_x > g.tiles_y ? g.tiles_x : g.tiles_y) >= (1LL << 32))
        BSY_FAIL(BSY_ERR_ARG, "%s: tile count out of range", who);
    g.ntiles = (int)nt;
    g.magic_x = (unsigned)(((1ULL << 32) + g.tiles_x - 1) / g.tiles_x);
    g.magic_y = (unsigned)(((1ULL << 32) + g.tiles_y - 1) / g.tiles_y);
    return BSY_OK;
}
struct TileIdx {
    int n, ty, tx;
};
__device__ __forceinline__ TileIdx tile_index(const TileGrid& g, int tile) {
    TileIdx t;
    const int r = (int)__umulhi((unsigned)tile, g.magic_x);
    t.tx = tile - r * g.tiles_x;
    t.n = (int)__umulhi((unsigned)r, g.magic_y);
    t.ty = r - t.n * g.tiles_y;
    return t;
}

// An MFMA accumulator tile (32 couts x 32 pixels, lane = pixel) that STARTS at the bias of its rows (round 3: every conv kernel of the
// fp16 path accumulates bias + sum instead of adding the bias in its epilogue -- one VALU instruction less per activation in
// kernels whose SIMDs are ~80 % busy issuing SiLU; all kernels do it alike, so fused and un-fused launches still agree bit for bit).
// Register r of lane half lh is cout (r & 3) + 8 (r >> 2) + 4 lh of the tile; `bias` points at the tile's first cout (f32, 16-byte
// aligned, 32 readable values: the packed bias vectors are padded to a multiple of 128).
__device__ __forceinline__ void acc_bias(f32x16& acc, const float* bias, int lh) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + 8 * g + 4 * lh);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * g + e] = bv[e];
    }
}

// SiLU in fp32: x * sigmoid(x) = x / (1 + 2^(-x*log2 e)); v_exp_f32 + v_rcp_f32 (1 ulp each) -- the result is rounded
// to fp16 right after, so the IEEE-division expansion (~10 VALU) would buy nothing.  exp2 overflow -> inf -> rcp -> 0.
__device__ __forceinline__ float silu_rcp(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f));
}
// The fp16 path's SiLU: the product passes through an empty asm.  Where a conversion to f16 follows directly, the compiler
// otherwise folds the final multiply and the conversion into v_fma_mixlo/hi_f16 -- ONE rounding of the exact product -- in some
// kernels and not in others (it did in c3k2_fused.hip's Bottleneck stage, not in bneck_fused.hip: 2 pixels in 1000 differed by
// one f16 ulp).  Every kernel rounds twice (f32, then f16), so fused and unfused launches agree bit for bit.  Kernels that keep
// the result in f32 (conv32x_mfma.hip) call silu_rcp: there the asm only costs, turning `act ? silu(t) : t` into branches.
__device__ __forceinline__ float silu_f(float x) {
    float r = silu_rcp(x);
    asm("" : "+v"(r));
    return r;
}
// a + b element by element: a vector-typed `a + b` is a pair of v_pk_add_f32, this is four v_add_f32 (the kernels that run
// beside other streams' MFMA kernels carry no packed f32 arithmetic at all; see the note on fma_mix_lo above)
__device__ __forceinline__ f32x4 add4_f(f32x4 a, f32x4 b) {
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = a[i] + b[i];
    return r;
}
// Four at a time, element by element (with -fno-slp-vectorize these stay scalar instructions; packed, the compiler's
// choice under plain -O3, they were not one microsecond faster over a forward).
__device__ __forceinline__ f32x4 silu4_f(f32x4 x) {
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = silu_f(x[i]);
    return r;
}
// ReLU (activation id 2 of include/bsyolo.h), the one form every precision mode uses: a compare and a select, exact.  NaN fails the
// compare and passes through, as torch.relu returns it (fmaxf would answer 0); the sign of a zero result is not specified.
__device__ __forceinline__ float relu_f(float x) { return x < 0.0f ? 0.0f : x; }
__device__ __forceinline__ f32x4 relu4_f(f32x4 x) {
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = relu_f(x[i]);
    return r;
}
// The activation of a CONV_FIRST / FIRST_POOL / STEM / CONV op on the fp16 path: act = 0 identity, 1 SiLU, 2 ReLU.  Every fp16 conv
// kernel exists twice: <name>, whose epilogue is `if (act) silu` as it always was -- instruction for instruction the kernel it was
// before id 2 existed (tools/isa_diff.py) --, and <name>_relu, the same body instantiated with RELU = true, whose epilogue is
// relu_f / relu4_f whatever `act` says.  The launchers pick by `act == 2`.  Every form that chose inside ONE kernel cost the SiLU path
// occupancy, scratch or 0.2 - 5 % of the YOLO11s step: docs/experiments.md, "ReLU as activation id 2".
// The fp32-storage kernels (conv32x_mfma.hip, conv32_mfma.hip, ref32.hip) pass their own SiLU (silu_rcp, silu32: no asm, so the choice
// compiles to selects there).
template <class SiLU>
__device__ __forceinline__ float act32(float t, int act, SiLU silu) { return act == 2 ? relu_f(t) : act ? silu(t) : t; }
// SiLU of the exact fp32 mode (ref32.hip, conv32_mfma.hip): the scalar and the MFMA kernels return the same bits only while both
// evaluate this the same way, so every user is built with -ffp-contract=off -fno-vectorize (build.py).
__device__ __forceinline__ float silu32(float x) { return x / (1.0f + expf(-x)); }
// Sigmoid of the fp16 path's gates and of the Detect decoders (the fused head epilogues of conv_kernels.h and detect.hip must agree)
__device__ __forceinline__ float sigmoid_f(float v) { return 1.0f / (1.0f + __expf(-v)); }
