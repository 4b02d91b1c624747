// The two dispatch switches of a plan: an op record's kind and precision mode choose a builder (op_args.h: what the record means) and
// the launcher its arguments go to.  Nothing is decoded here.  A builder returns false with the error text set, whether a required
// view did not resolve or the record's shapes are wrong; nothing is launched then.
#include "engine.h"

namespace {
// Build, then launch or refuse: every kind whose launcher takes an *Args struct goes through here.
template <typename Args>
int run(bool (*build)(Args&, const bsy_op&, Resolver&, const char*), int (*launch)(const Args&, hipStream_t), const bsy_op& op,
        Resolver& R, const char* wb, hipStream_t s) {
    Args a;
    return build(a, op, R, wb) ? launch(a, s) : BSY_ERR_ARG;
}
}  // namespace

int run_op(const bsy_op& op, Resolver& R, const char* wb, hipStream_t s) {
    if (op.prec < 0 || op.prec > 2) BSY_FAIL(BSY_ERR_ARG, "plan_run: unknown precision mode %d", op.prec);
    // fp32 correctness mode (bsy_op.prec == 1, and 2 = fp32x) first: same op records, f32 views, kernels of ref32.hip.  DECODE, RAW_NCHW
    // and CLASSIFY_TAIL consume f32 logit maps in every mode, POOL_DOWN and MAXPOOL take the storage type as an argument, E2E_TOPK reads a tensor of
    // out_dtype, MAXSIG's and CBFUSE's launchers take the storage type as an argument too: they break out of this switch into the common one.
    Views<float> v32;
    if (op.prec) switch (op.kind) {
        case BSY_OP_CONV_FIRST:
        case BSY_OP_CONV: {
            Conv32Args a;
            if (!build_conv32(a, op, R, wb)) return BSY_ERR_ARG;
            // fp32x: split-f16 planes behind the f32 matrix; shapes the kernel does not take stay exact
            return op.prec == 2 && conv32x_mfma_supported(a) ? launch_conv32x_mfma(a, s) : launch_conv32(a, s);
        }
        case BSY_OP_DWCONV:
        case BSY_OP_DWCONV_G:
            return run(build_dw32, launch_dw32, op, R, wb, s);
        case BSY_OP_SPPF_POOL:
            return build_views(v32, op, R, 1) ? launch_sppf32(v32.src0, op.src0.ld, op.B, op.H, op.W, op.src0.C, s) : BSY_ERR_ARG;
        case BSY_OP_ATTN:
            if (!build_views(v32, op, R, 2)) return BSY_ERR_ARG;
            if (op.prec == 2 && attn32x_supported(op.src0.ld, op.dst.ld, op.key_dim, op.head_dim, v32.src0, v32.dst))  // fp32x: split-f16 products on the matrix pipe
                return launch_attn32x(v32.src0, op.src0.ld, op.B, op.H * op.W, op.heads, op.key_dim, op.head_dim, op.scale, v32.dst, op.dst.ld, s);
            return launch_attn32(v32.src0, op.src0.ld, op.B, op.H * op.W, op.heads, op.key_dim, op.head_dim, op.scale, v32.dst, op.dst.ld, s);
        case BSY_OP_NHWC2NCHW: {
            const float* src;
            void* out;
            bool skip;
            if (!build_nhwc2nchw(src, out, skip, op, R)) return BSY_ERR_ARG;
            return skip ? BSY_OK : launch_nhwc2nchw32(src, op.src0.ld, op.B, op.src0.C, op.H * op.W, out, op.out_dtype, s);
        }
        case BSY_OP_COPY:
            if (!build_views(v32, op, R, 2)) return BSY_ERR_ARG;
            return launch_copy32(v32.src0, op.src0.ld, op.up0, op.B, op.H, op.W, op.src0.C, v32.dst, op.dst.ld, s);
        case BSY_OP_GAP:
            return build_views(v32, op, R, 2) ? launch_gap32(v32.src0, op.src0.ld, op.B, op.H, op.W, op.src0.C, v32.dst, op.dst.ld, s) : BSY_ERR_ARG;
        case BSY_OP_MSCA_MIX:
            return run(build_mix<float, Mix32Args>, launch_mix32, op, R, wb, s);
        case BSY_OP_MUL:
            if (!build_views(v32, op, R, 3)) return BSY_ERR_ARG;
            return launch_mul32(v32.src0, op.src0.ld, v32.src1, op.src1.ld, (long long)op.B * op.H * op.W, op.dst.C, v32.dst, op.dst.ld, s);
        case BSY_OP_ADD:
            if (!build_views(v32, op, R, 3)) return BSY_ERR_ARG;
            return launch_add32(v32.src0, op.src0.ld, v32.src1, op.src1.ld, (long long)op.B * op.H * op.W, op.dst.C, v32.dst, op.dst.ld, s);
        case BSY_OP_ELA: {
            ElaArgs a;
            const float* src;
            float* dst;
            return build_ela32(a, src, dst, op, R, wb) ? launch_ela32(a, src, dst, s) : BSY_ERR_ARG;
        }
        case BSY_OP_POOL_DOWN:
        case BSY_OP_MAXPOOL:
        case BSY_OP_CLASSIFY_TAIL:
        case BSY_OP_DECODE:
        case BSY_OP_RAW_NCHW:
        case BSY_OP_E2E_TOPK:
        case BSY_OP_MAXSIG:
        case BSY_OP_CBFUSE:
            break;
        default:
            BSY_FAIL(BSY_ERR_ARG, "fp32 mode: op kind %d has no fp32 implementation (fused kinds are fp16-only)", op.kind);
    }
    Views<half_t> v;
    switch (op.kind) {
        case BSY_OP_CONV_FIRST: return run(build_conv_first, launch_conv_first, op, R, wb, s);
        case BSY_OP_FIRST_POOL: return run(build_first_pool, launch_conv_first, op, R, wb, s);
        case BSY_OP_STEM: return run(build_stem, launch_stem_fused, op, R, wb, s);
        case BSY_OP_BNECK: return run(build_bneck, launch_bneck_fused, op, R, wb, s);
        case BSY_OP_C3K2: return run(build_c3k2, launch_c3k2_fused, op, R, wb, s);
        case BSY_OP_DWPW: return run(build_dwpw, launch_dwpw_fused, op, R, wb, s);
        case BSY_OP_DWCONV_G: return run(build_dwconv_g, launch_dwconv_generic, op, R, wb, s);
        case BSY_OP_PMSFA_TAIL: return run(build_pmsfa_tail, launch_pmsfa_tail, op, R, wb, s);
        case BSY_OP_GHOST: return run(build_ghost, launch_ghost_fused, op, R, wb, s);
        case BSY_OP_MSCA_SPATIAL: return run(build_msca_spatial, launch_msca_spatial, op, R, wb, s);
        case BSY_OP_MSCA_MIX: return run(build_mix<half_t, MixArgs>, launch_msca_mix, op, R, wb, s);
        case BSY_OP_ELA: return run(build_ela, launch_ela, op, R, wb, s);
        case BSY_OP_CONV: return run(build_conv, launch_conv, op, R, wb, s);
        case BSY_OP_DWCONV: return run(build_dwconv, launch_dwconv, op, R, wb, s);
        case BSY_OP_DECODE: return run(build_decode, launch_decode, op, R, wb, s);
        case BSY_OP_MAXSIG: return run(build_maxsig, launch_maxsig, op, R, wb, s);  // f16 views, f32 in the fp32-storage modes
        case BSY_OP_CBFUSE: return run(build_cbfuse, launch_cbfuse, op, R, wb, s);  // f16 views, f32 in the fp32-storage modes
        case BSY_OP_ATTN: {
            AttnArgs a;
            return build_attn(a, op, R, wb) ? launch_attention(a, s) : BSY_ERR_ARG;
        }
        case BSY_OP_S2D: {
            const void* img;
            half_t* dst;
            return build_s2d(img, dst, op, R) ? launch_s2d(img, op.in_dtype, op.B, op.H, op.W, dst, op.dst.ld, s) : BSY_ERR_ARG;
        }
        case BSY_OP_COPY:
            if (!build_views(v, op, R, 2)) return BSY_ERR_ARG;
            return launch_copy_view(v.src0, op.src0.ld, op.up0, op.B, op.H, op.W, op.src0.C, v.dst, op.dst.ld, s);
        case BSY_OP_GAP:
            return build_views(v, op, R, 2) ? launch_gap(v.src0, op.src0.ld, op.B, op.H, op.W, op.src0.C, v.dst, op.dst.ld, s) : BSY_ERR_ARG;
        case BSY_OP_MUL:
            if (!build_views(v, op, R, 3)) return BSY_ERR_ARG;
            return launch_mul(v.src0, op.src0.ld, v.src1, op.src1.ld, (long long)op.B * op.H * op.W, op.dst.C, v.dst, op.dst.ld, s);
        case BSY_OP_ADD:
            if (!build_views(v, op, R, 3)) return BSY_ERR_ARG;
            return launch_add(v.src0, op.src0.ld, v.src1, op.src1.ld, (long long)op.B * op.H * op.W, op.dst.C, v.dst, op.dst.ld, s);
        case BSY_OP_SPPF_POOL:
            return build_views(v, op, R, 1) ? launch_sppf_pool(v.src0, op.src0.ld, op.B, op.H, op.W, op.src0.C, s) : BSY_ERR_ARG;
        case BSY_OP_POOL_DOWN: {  // f16 views, f32 in the fp32-storage modes
            const char* src;
            char* dst;
            if (!build_pool_down(src, dst, op, R)) return BSY_ERR_ARG;
            return launch_pool_down(src, op.src0.ld, op.src0.coff, dst, op.dst.ld, op.dst.coff, op.B, op.H, op.W, op.src0.C, op.level,
                                    op.prec ? BSY_F32 : BSY_F16, s);
        }
        case BSY_OP_MAXPOOL: {  // f16 views, f32 in the fp32-storage modes
            const char* src;
            char* dst;
            if (!build_maxpool(src, dst, op, R)) return BSY_ERR_ARG;
            return launch_maxpool(src, op.src0.ld, op.src0.coff, dst, op.dst.ld, op.dst.coff, op.B, op.H, op.W, op.src0.C, op.level,
                                  op.prec ? BSY_F32 : BSY_F16, s);
        }
        case BSY_OP_RAW_NCHW: {
            RawNchwArgs a;
            if (!build_raw_nchw(a, op, R)) return BSY_ERR_ARG;
            return a.skip ? BSY_OK : launch_raw_nchw(a.box, a.ldb, a.cls, a.ldc, op.B, a.h, a.w, op.nc, a.out, op.out_dtype, s);
        }
        case BSY_OP_NHWC2NCHW: {
            const half_t* src;
            void* out;
            bool skip;
            if (!build_nhwc2nchw(src, out, skip, op, R)) return BSY_ERR_ARG;
            return skip ? BSY_OK : launch_nhwc2nchw(src, op.src0.ld, op.B, op.src0.C, op.H * op.W, out, op.out_dtype, s);
        }
        case BSY_OP_CLASSIFY_TAIL: {
            ClassifyArgs a;
            if (!build_classify_tail(a, op, R)) return BSY_ERR_ARG;
            return launch_classify_tail(a.logits, op.src0.ld, op.B, op.nc, a.y, a.x, op.out_dtype, a.k, a.idx, a.val, s);
        }
        case BSY_OP_E2E_TOPK: {  // the two launches of bsy_end2end_topk on `s`: nothing but kernel launches, so it is captured like any op
            TopkArgs a;
            if (!build_e2e_topk(a, op, R)) return BSY_ERR_ARG;
            return bsy_end2end_topk(a.pred, op.out_dtype, op.B, op.nc, op.A, op.ksize, a.rows, a.ws, a.ws_bytes, (bsy_stream)s);
        }
        default:
            BSY_FAIL(BSY_ERR_ARG, "plan_run: unknown op kind %d", op.kind);
    }
}
