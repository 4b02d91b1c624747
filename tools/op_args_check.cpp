// Stand-alone host check of the op-record builders (csrc/op_args.h): what a bsy_op record becomes BEFORE anything is launched -- the
// refusals of the resolver, the optional outputs that turn into null pointers, and the overloaded fields of the conv, DWCONV_G and ELA
// records, against literals taken from the comments of include/bsyolo.h.  The resolver works over a host vector, the weight blob is a
// host array whose addresses are only compared: the program needs no GPU and is meant for a host sanitizer:
//   C=bs_yolo_amd/csrc; hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -x hip -fno-slp-vectorize -Xarch_host -fsanitize=address,undefined \
//       -I$C tools/op_args_check.cpp $C/err.cpp -o tools/bin/op_args_check && tools/bin/op_args_check
// Exit status 0: every case held (and the sanitizers silent).
#include "op_args.h"
#include <cstdio>
#include <cstring>
#include <vector>

static int n_checks = 0, n_bad = 0;
static void expect(bool ok, const char* what, int line) {
    ++n_checks;
    if (!ok) { ++n_bad; printf("line %d: NOT %s   (last error: %s)\n", line, what, bsy_last_error()); }
}
#define EXPECT(c) expect((c), #c, __LINE__)

static bsy_view view(int buf, int ld, int coff, int C) { return bsy_view{buf, ld, coff, C}; }
static bsy_op blank(int kind) {  // every view absent, every scalar zero
    bsy_op op;
    memset(&op, 0, sizeof(op));
    op.kind = kind;
    op.src0.buf = op.src1.buf = op.dst.buf = op.res.buf = -1;
    for (int l = 0; l < BSY_MAX_LEVELS; ++l) op.box[l].buf = op.cls[l].buf = op.msk[l].buf = -1;
    return op;
}
static void clear_error() { bsy_set_error("%s", ""); }
static bool error_set() { return bsy_last_error()[0] != 0; }

int main() {
    // workspace: four buffers at uneven offsets of a host vector; external slots 0 and 2 bound, 1 unbound, 3.. beyond n_ext
    std::vector<char> ws(4096, 0);
    const size_t off[4] = {0, 768, 1024, 2816};
    std::vector<char> ext0(256), ext2(256), blob(8192);
    void* ext[3] = {ext0.data(), nullptr, ext2.data()};
    const char* wb = blob.data();
    auto resolver = [&]() { return Resolver{ws.data(), off, 4, ext, 3}; };
    const int E = BSY_EXT_BASE;

    // ---- refusals: a REQUIRED view that does not resolve is false with a text; bound() on the same view is false and silent ----
    const bsy_view unbound = view(E + 1, 8, 0, 8), beyond = view(E + 3, 8, 0, 8), no_buf = view(4, 8, 0, 8);
    for (const bsy_view* bad : {&unbound, &beyond, &no_buf}) {
        Resolver R = resolver();
        clear_error();
        EXPECT(!R.bound(*bad));
        EXPECT(!error_set() && R.ok);
        bsy_op op = blank(BSY_OP_COPY);
        op.src0 = view(0, 16, 0, 8); op.dst = *bad;
        Views<half_t> v;
        EXPECT(!build_views(v, op, R, 2));
        EXPECT(error_set() && !R.ok && v.dst == nullptr);
    }
    {
        Resolver R = resolver();
        clear_error();
        EXPECT(R.bound(view(3, 8, 0, 8)) && R.bound(view(E + 2, 8, 0, 8)) && !R.bound(view(-1, 0, 0, 0)));
        EXPECT(R.base(view(-1, 0, 0, 0)) == nullptr && R.ok && !error_set());  // an absent view is no error
        EXPECT(R.h(view(1, 32, 8, 8)) == (half_t*)(ws.data() + 768) + 8 && R.f(view(3, 32, 4, 8)) == (float*)(ws.data() + 2816) + 4);
        EXPECT(R.base(view(E + 2, 8, 4, 4)) == ext2.data());
    }

    // ---- optional outputs: an unbound slot is a null pointer, not a refusal ----
    {   // CONV with the class decoder in its epilogue (out_f32 = 2): box[0] = the level's raw map
        Resolver R = resolver();
        bsy_op op = blank(BSY_OP_CONV);
        op.src0 = view(0, 64, 0, 64); op.dst = view(E + 0, 0, 0, 84); op.out_f32 = 2; op.nl = 80; op.box[0] = view(E + 1, 0, 0, 144);
        ConvArgs a;
        clear_error();
        EXPECT(build_conv(a, op, R, wb) && !error_set());
        EXPECT(a.raw == nullptr && a.rawC == 144 && a.y == ext0.data());
        op.box[0].buf = E + 2;
        ConvArgs b;
        EXPECT(build_conv(b, op, R, wb) && b.raw == ext2.data());
    }
    {   // DECODE of a Pose head: res = the raw keypoint tensor
        Resolver R = resolver();
        bsy_op op = blank(BSY_OP_DECODE);
        op.nl = 1; op.nc = 1; op.nk = 51; op.kdim = 3; op.dst = view(E + 0, 0, 0, 56); op.res = view(E + 3, 0, 0, 51);
        op.box[0] = view(0, 64, 0, 64); op.cls[0] = view(1, 4, 0, 1); op.msk[0] = view(2, 52, 0, 51);
        DecodeArgs a;
        clear_error();
        EXPECT(build_decode(a, op, R, wb) && !error_set());
        EXPECT(a.kraw == nullptr && a.nk == 51 && a.kdim == 3 && a.msk[0] == (float*)(ws.data() + 1024) && a.ldm[0] == 52);
        op.res.buf = E + 2;
        DecodeArgs b;
        EXPECT(build_decode(b, op, R, wb) && b.kraw == ext2.data());
    }
    {   // CLASSIFY_TAIL: the top-k rows only together
        Resolver R = resolver();
        bsy_op op = blank(BSY_OP_CLASSIFY_TAIL);
        op.src0 = view(0, 12, 0, 10); op.nc = 10; op.dst = view(E + 0, 0, 0, 10); op.ksize = 5;
        op.box[0] = view(E + 2, 0, 0, 5); op.cls[0] = view(E + 1, 0, 0, 5);
        ClassifyArgs a;
        clear_error();
        EXPECT(build_classify_tail(a, op, R) && !error_set());
        EXPECT(a.idx == nullptr && a.val == nullptr && a.k == 0 && a.x == nullptr && a.y == ext0.data());
    }

    {   // MAXSIG: both storage types through one builder; what the record alone says is refused before a view is resolved
        Resolver R = resolver();
        bsy_op op = blank(BSY_OP_MAXSIG);
        op.B = 2; op.H = 3; op.W = 5; op.heads = 2; op.head_dim = 32; op.nc = 12; op.w_off = 512; op.b_off = 4096;
        op.src0 = view(0, 160, 8, 64); op.src1 = view(0, 160, 72, 64); op.dst = op.src1;
        MaxSigArgs a;
        clear_error();
        EXPECT(build_maxsig(a, op, R, wb) && !error_set());
        EXPECT(a.embed == (half_t*)ws.data() + 8 && a.proj == (half_t*)ws.data() + 72 && a.dst == a.proj && a.dtype == BSY_F16);
        EXPECT(a.lde == 160 && a.HW == 15 && a.heads == 2 && a.hc == 32 && a.nc == 12 && a.G == wb + 512 && a.bias_scale == (const float*)(wb + 4096));
        op.prec = 1; op.head_dim = 7; op.src0.C = op.src1.C = op.dst.C = 14;
        MaxSigArgs b;
        EXPECT(build_maxsig(b, op, R, wb) && b.dtype == BSY_F32 && b.embed == (float*)ws.data() + 8 && b.hc == 7);
        op.prec = 0;
        for (int bad = 0; bad < 4; ++bad) {
            bsy_op o = op;
            o.head_dim = 32; o.src0.C = o.src1.C = o.dst.C = 64;
            if (bad == 0) o.nc = 0;
            if (bad == 1) { o.head_dim = 8; o.src0.C = o.src1.C = o.dst.C = 16; }
            if (bad == 2) o.dst = view(0, 160, 40, 64);  // over the embedding's channels
            if (bad == 3) o.src1.buf = -1;
            Resolver Rb = resolver();
            MaxSigArgs c;
            clear_error();
            EXPECT(!build_maxsig(c, o, Rb, wb) && error_set() && !Rb.ok && c.embed == nullptr);
        }
    }

    // ---- the conv record, field by field ----
    {   // two sources (virtual Concat), the second read through nearest-x2
        Resolver R = resolver();
        bsy_op op = blank(BSY_OP_CONV);
        op.B = 2; op.H = 20; op.W = 24; op.OH = 10; op.OW = 12; op.ksize = 3; op.stride = 2; op.pad = 1; op.act = 1;
        op.src0 = view(0, 64, 8, 16); op.src1 = view(1, 32, 0, 24); op.up1 = 1;
        op.dst = view(2, 48, 16, 32); op.w_off = 512; op.b_off = 4096;
        ConvArgs a;
        EXPECT(build_conv(a, op, R, wb));
        EXPECT(a.src0 == (half_t*)ws.data() + 8 && a.src1 == (half_t*)(ws.data() + 768));
        EXPECT(a.ld0 == 64 && a.ld1 == 32 && a.C0 == 16 && a.C1 == 24 && a.up0 == 0 && a.up1 == 1);
        EXPECT(a.B == 2 && a.H == 20 && a.W == 24 && a.OH == 10 && a.OW == 12 && a.ksize == 3 && a.stride == 2 && a.pad == 1 && a.act == 1);
        EXPECT((const char*)a.wgt == wb + 512 && (const char*)a.bias == wb + 4096);
        EXPECT(a.dst == (half_t*)(ws.data() + 1024) + 16 && a.ldd == 48 && a.Cout == 32 && a.out_f32 == 0);
        EXPECT(a.res == nullptr && a.ldr == 0 && a.epi == 0 && a.y == nullptr && a.tail_wgt == nullptr && a.nsl_c == 0 && a.split_ws == nullptr);
        op.out_f32 = 1;  // f32 output: the channel offset counts floats
        ConvArgs b;
        EXPECT(build_conv(b, op, R, wb) && b.dst == (float*)(ws.data() + 1024) + 16 && b.out_f32 == 1);
    }
    {   // one source: the absent second one is null with zero width; ConvTranspose2d(2, 2, s2) as scattered 1x1 convs
        Resolver R = resolver();
        bsy_op op = blank(BSY_OP_CONV);
        op.src0 = view(0, 64, 0, 64); op.dst = view(2, 32, 0, 32); op.res = view(1, 40, 8, 32);
        op.dst_scale = 2; op.dst_dy = 1; op.dst_dx = 0; op.tuned_cfg = 5;
        ConvArgs a;
        EXPECT(build_conv(a, op, R, wb));
        EXPECT(a.src1 == nullptr && a.ld1 == 0 && a.C1 == 0);
        EXPECT(a.dst_scale == 2 && a.dst_dy == 1 && a.dst_dx == 0);
        EXPECT(a.res == (half_t*)(ws.data() + 768) + 8 && a.ldr == 40);
        EXPECT(a.cfg == 4);  // tuned_cfg = 1 + configuration id
        op.tuned_cfg = 0;
        ConvArgs b;
        EXPECT(build_conv(b, op, R, wb) && b.cfg == -1);  // 0 = heuristic
    }
    {   // fused Detect decoder, class branch (epi 2) and box branch (epi 3) with and without the 1x1 tail
        Resolver R = resolver();
        bsy_op op = blank(BSY_OP_CONV);
        op.src0 = view(0, 64, 0, 64); op.dst = view(E + 2, 0, 4, 84); op.out_f32 = 2; op.nl = 80; op.out_dtype = BSY_F32;
        op.A = 8400; op.lvl_h[0] = 80; op.lvl_h[1] = 6400; op.lvl_stride[0] = 16.f; op.ksplit = 2 | 3 << 8;
        op.w2_off = 1024; op.b2_off = 2048;
        ConvArgs a;
        EXPECT(build_conv(a, op, R, wb));
        EXPECT(a.epi == 2 && a.out_f32 == 0 && a.Cout == 80 && a.ldd == 8 && a.dst == nullptr);
        EXPECT(a.y == ext2.data() && a.y_f32 == 1 && a.raw_f32 == 1 && a.A == 8400 && a.a0 == 6400 && a.nrows == 84 && a.lvl_stride == 16.f);
        EXPECT(a.tail_wgt == nullptr && a.tail_bias == nullptr);
        EXPECT(a.nsl_c == 0 && a.nsl_t == 0 && a.split_ws == nullptr);  // ksplit is for plain f16 outputs only
        op.out_f32 = 3; op.nl = 64; op.out_dtype = BSY_F16;
        ConvArgs b;
        EXPECT(build_conv(b, op, R, wb) && b.epi == 3 && b.Cout == 64 && b.y_f32 == 0 && b.tail_wgt == nullptr);
        op.mid_c = 48;  // (not 64, so that Cout = mid_c and Cout = nl differ)
        ConvArgs c;
        EXPECT(build_conv(c, op, R, wb) && c.Cout == 48);
        EXPECT((const char*)c.tail_wgt == wb + 1024 && (const char*)c.tail_bias == wb + 2048);
    }
    {   // split-K: channel slices | tap slices << 8, box[0] = the f32 slab buffer; ignored for an f32 output
        Resolver R = resolver();
        bsy_op op = blank(BSY_OP_CONV);
        op.src0 = view(0, 64, 0, 64); op.dst = view(2, 32, 0, 32); op.ksplit = 2 | 3 << 8; op.box[0] = view(3, 32, 4, 32);
        ConvArgs a;
        EXPECT(build_conv(a, op, R, wb) && a.nsl_c == 2 && a.nsl_t == 3 && a.split_ws == (float*)(ws.data() + 2816) + 4);
        op.out_f32 = 1;
        ConvArgs b;
        EXPECT(build_conv(b, op, R, wb) && b.nsl_c == 0 && b.nsl_t == 0 && b.split_ws == nullptr);
    }

    // ---- DWCONV_G: ksize = height, pad = WIDTH, heads = weight row length, key_dim = first channel, act = channels with SiLU ----
    {
        Resolver R = resolver();
        bsy_op op = blank(BSY_OP_DWCONV_G);
        op.B = 1; op.H = 9; op.W = 11; op.OH = 5; op.OW = 6; op.ksize = 5; op.pad = 7; op.stride = 2; op.heads = 96; op.key_dim = 32;
        op.act = 16; op.mid_c = 24; op.src0 = view(0, 64, 8, 32); op.dst = view(1, 32, 0, 32); op.res = view(2, 32, 0, 32);
        op.w_off = 256; op.b_off = 6144;
        DwGenArgs a;
        EXPECT(build_dwconv_g(a, op, R, wb));
        EXPECT(a.kh == 5 && a.kw == 7 && a.stride == 2 && a.wld == 96 && a.act_c == 16 && a.ident_c0 == 24);
        EXPECT(a.w == (const float*)(wb + 256) + 32 && a.b == (const float*)(wb + 6144) + 32);
        EXPECT(a.src == (half_t*)ws.data() + 8 && a.lds == 64 && a.C == 32 && a.OH == 5 && a.OW == 6 && a.dst == (half_t*)(ws.data() + 768) && a.ldd == 32);
        Dw32Args b;
        EXPECT(build_dw32(b, op, R, wb));
        EXPECT(b.kh == 5 && b.kw == 7 && b.stride == 2 && b.wld == 96 && b.act_c == 16);
        EXPECT(b.w == (const float*)(wb + 256) + 32 && b.b == (const float*)(wb + 6144) + 32);
        EXPECT(b.src == (float*)ws.data() + 8 && b.dst == (float*)(ws.data() + 768) && b.res == nullptr && b.ldr == 0);  // no residual in this kind
        op.kind = BSY_OP_DWCONV; op.act = 1;  // the 3x3 kind in fp32 storage: SiLU on all channels, residual
        Dw32Args c;
        EXPECT(build_dw32(c, op, R, wb) && c.kh == 3 && c.kw == 3 && c.stride == 1 && c.wld == 32 && c.act_c == 32);
        EXPECT(c.w == (const float*)(wb + 256) && c.res == (float*)(ws.data() + 1024) && c.ldr == 32);
    }

    // ---- ELA: w_off -> [spatial_conv C*k][ch_att conv C*k][gn.weight C][gn.bias C]; scale, lvl_stride[0..1] = the coefficients ----
    {
        Resolver R = resolver();
        bsy_op op = blank(BSY_OP_ELA);
        op.B = 2; op.H = 6; op.W = 10; op.ksize = 7; op.src0 = view(0, 32, 8, 16); op.dst = view(1, 16, 0, 16); op.res = view(3, 16, 0, 16);
        op.w_off = 1280; op.scale = 0.25f; op.lvl_stride[0] = 0.5f; op.lvl_stride[1] = 0.75f;
        const float* blob_f = (const float*)(wb + 1280);
        ElaArgs a;
        EXPECT(build_ela(a, op, R, wb));
        EXPECT(a.wsp == blob_f && a.wch == blob_f + 112 && a.gnw == blob_f + 224 && a.gnb == blob_f + 240);
        EXPECT(a.ch_coef == 0.25f && a.sp_coef == 0.5f && a.res_coef == 0.75f && a.C == 16 && a.k == 7 && a.lds == 32 && a.ldd == 16);
        EXPECT(a.scratch == (float*)(ws.data() + 2816) && a.src == (half_t*)ws.data() + 8 && a.dst == (half_t*)(ws.data() + 768));
        ElaArgs b;
        const float* src = nullptr;
        float* dst = nullptr;
        EXPECT(build_ela32(b, src, dst, op, R, wb));
        EXPECT(b.wsp == blob_f && b.wch == blob_f + 112 && b.gnw == blob_f + 224 && b.gnb == blob_f + 240 && b.res_coef == 0.75f);
        EXPECT(src == (float*)ws.data() + 8 && dst == (float*)(ws.data() + 768) && b.src == nullptr && b.dst == nullptr);
    }
    printf("%d checks, %d failed\n", n_checks, n_bad);
    return n_bad != 0;
}
