// First convolution of the graph: image BCHW (fp16 or fp32, 3 channels) -> conv 3x3 stride S pad 1 + bias + SiLU -> NHWC fp16, S = 2
// (every YOLOv5u .. YOLO11 graph) or 1 (YOLOv3: cfg/models/v3/yolov3.yaml:14, yolov3-tiny.yaml:14).
//
// Replaces model.0 Conv.forward_fuse (nn/modules/conv.py:149-151; layer 0 of cfg/models/11/yolo11-seg.yaml:17) and
// absorbs the NCHW->NHWC layout change.  HBM-bound (reads 3*H*W, writes Cout*H*W/4 elements per image), so the job is
// to touch every input byte ~once, coalesced, and keep the 27-deep contraction off the VALU:
//   * a workgroup owns a 4 x 64 output tile; its 9 x 132 x 3 input patch (stride 1: 6 x 72 x 3) is read in aligned groups of
//     4 pixels per plane and parked in LDS pixel-interleaved with a zero 4th channel (image_conv.h);
//   * the contraction runs on v_mfma_f32_32x32x16_f16 with K = 9 taps x 4 = 36 padded to 48 -- weights packed like every
//     other conv ([CoutPad][Kpad], k = (kh, kw, c)) but with the zero 4th input channel, held in registers as the A
//     operand; a lane's B fragment is two taps = two 8-byte LDS reads at compile-time offsets;
//   * epilogue as conv_gemm.hip: the tile goes through LDS so every store is a coalesced 16-byte piece.
// POOL (stride 1 only; BSY_OP_FIRST_POOL): nn.MaxPool2d(2, 2, 0) in the same launch -- yolov3-tiny's layers 0 + 1.  The tile is in LDS
// as activated, rounded fp16 anyway; the store loop writes the 2 x 32 pooled tile, each piece the max of four entries (pool_max.h:
// SiLU is not monotone, so the max comes after activation and rounding).  The full-size map, the largest activation of that graph by
// a factor of four, is never written: the bits of CONV_FIRST stride 1 -> MAXPOOL mode 0.
#include "image_conv.h"
#include "pool_max.h"

#define CF_TH 4
#define CF_TW 64
// patch geometry for stride S: rows S * (TH - 1) + 3 (9 / 6); 4-pixel groups per row covering image columns S*TW*tx - 4 ..
// S*TW*tx + S * (TW - 1) + 1 (33 / 18 groups = 132 / 72 patch pixels of 8 bytes each)
#define CF_PR(S) ((S) * (CF_TH - 1) + 3)
#define CF_NG(S) (((S) * (CF_TW - 1) + 6 + 3) / 4)

#define BSY_K(n) n
#define BSY_RELU false
#include "conv_first_kernel.h"
#undef BSY_K
#undef BSY_RELU
#define BSY_K(n) n##_relu
#define BSY_RELU true
#include "conv_first_kernel.h"
#undef BSY_K
#undef BSY_RELU

template <typename T, int S, bool POOL>
static int launch_t(const ConvFirstArgs& a, hipStream_t s) {
    const int tiles_x = ceil_div(a.OW, CF_TW), tiles_y = ceil_div(a.OH, CF_TH);
    const long long nblk = (long long)a.B * tiles_x * tiles_y;
    if (nblk > 0x7fffffffLL) BSY_FAIL(BSY_ERR_ARG, "conv_first: grid too large");
    dim3 grid((unsigned)nblk);
    const T* img = (const T*)a.img;
    const half_t* w = (const half_t*)a.w;
    if (a.Cout <= 32)
        { if (a.act == 2) hipLaunchKernelGGL((conv_first_mfma_kernel_relu<T, 1, S, POOL>), grid, dim3(256), 0, s, img, w, a.b, a.dst, a.H, a.W, a.OH, a.OW,
                           a.ldd, a.Cout, a.act, tiles_x, tiles_y); else hipLaunchKernelGGL((conv_first_mfma_kernel<T, 1, S, POOL>), grid, dim3(256), 0, s, img, w, a.b, a.dst, a.H, a.W, a.OH, a.OW,
                           a.ldd, a.Cout, a.act, tiles_x, tiles_y); }
    else if (a.Cout <= 64)
        { if (a.act == 2) hipLaunchKernelGGL((conv_first_mfma_kernel_relu<T, 2, S, POOL>), grid, dim3(256), 0, s, img, w, a.b, a.dst, a.H, a.W, a.OH, a.OW,
                           a.ldd, a.Cout, a.act, tiles_x, tiles_y); else hipLaunchKernelGGL((conv_first_mfma_kernel<T, 2, S, POOL>), grid, dim3(256), 0, s, img, w, a.b, a.dst, a.H, a.W, a.OH, a.OW,
                           a.ldd, a.Cout, a.act, tiles_x, tiles_y); }
    else if (a.Cout <= 96)
        { if (a.act == 2) hipLaunchKernelGGL((conv_first_mfma_kernel_relu<T, 3, S, POOL>), grid, dim3(256), 0, s, img, w, a.b, a.dst, a.H, a.W, a.OH, a.OW,
                           a.ldd, a.Cout, a.act, tiles_x, tiles_y); else hipLaunchKernelGGL((conv_first_mfma_kernel<T, 3, S, POOL>), grid, dim3(256), 0, s, img, w, a.b, a.dst, a.H, a.W, a.OH, a.OW,
                           a.ldd, a.Cout, a.act, tiles_x, tiles_y); }
    else
        { if (a.act == 2) hipLaunchKernelGGL((conv_first_mfma_kernel_relu<T, 4, S, POOL>), grid, dim3(256), 0, s, img, w, a.b, a.dst, a.H, a.W, a.OH, a.OW,
                           a.ldd, a.Cout, a.act, tiles_x, tiles_y); else hipLaunchKernelGGL((conv_first_mfma_kernel<T, 4, S, POOL>), grid, dim3(256), 0, s, img, w, a.b, a.dst, a.H, a.W, a.OH, a.OW,
                           a.ldd, a.Cout, a.act, tiles_x, tiles_y); }
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

// What the pooling form takes: the conv's widths, and a map MaxPool2d(2, 2, 0) halves exactly
bool first_pool_supported(int Cout, int H, int W) { return Cout > 0 && !(Cout % 8) && Cout <= 128 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1); }

// a.pool: a.OH x a.OW stays the CONV's output extent (H x W at stride 1); dst is the (OH / 2) x (OW / 2) pooled map
int launch_conv_first(const ConvFirstArgs& a, hipStream_t s) {
    if (a.ksize != 3 || (a.stride != 2 && a.stride != 1) || a.pad != 1)
        BSY_FAIL(BSY_ERR_ARG, "conv_first: only 3x3 stride 1 or 2 pad 1 (got k=%d s=%d p=%d)", a.ksize, a.stride, a.pad);
    if (a.Cout % 8 || a.Cout > 128 || a.ldd % 8 || ((uintptr_t)a.dst & 15) || ((uintptr_t)a.w & 15) || ((uintptr_t)a.b & 15))
        BSY_FAIL(BSY_ERR_ARG, "conv_first: Cout must be a multiple of 8 and <= 128; 16-byte aligned pointers");
    if (a.OH != (a.H + 2 - 3) / a.stride + 1 || a.OW != (a.W + 2 - 3) / a.stride + 1) BSY_FAIL(BSY_ERR_ARG, "conv_first: output extent mismatch");
    if (a.img_dtype != BSY_F16 && a.img_dtype != BSY_F32) BSY_FAIL(BSY_ERR_ARG, "conv_first: image dtype %d unsupported", a.img_dtype);
    const bool f16 = a.img_dtype == BSY_F16;
    if (a.pool) {
        if (a.stride != 1 || !first_pool_supported(a.Cout, a.H, a.W))
            BSY_FAIL(BSY_ERR_ARG, "first_pool: stride 1 on an even H x W image (got s=%d, %d x %d, Cout %d)", a.stride, a.H, a.W, a.Cout);
        return f16 ? launch_t<half_t, 1, true>(a, s) : launch_t<float, 1, true>(a, s);
    }
    if (a.stride == 1) return f16 ? launch_t<half_t, 1, false>(a, s) : launch_t<float, 1, false>(a, s);
    return f16 ? launch_t<half_t, 2, false>(a, s) : launch_t<float, 2, false>(a, s);
}
