// Fused stem: image BCHW (f16 / f32) -> Conv 3x3 s2 (3 -> C0) + SiLU -> Conv 3x3 s2 (C0 -> C1) + SiLU -> NHWC f16.
//
// Replaces model.0 + model.1 (both Conv.forward_fuse, nn/modules/conv.py:149-151; layers 0 and 1 of
// cfg/models/11/yolo11.yaml and cfg/models/v8/yolov8.yaml).  Unfused, layer 0's output (B x H/2 x W/2 x C0 f16, the
// largest activation of the graph: 419 MB at B = 64, 640 x 640, C0 = 32) is written to HBM and read straight back:
// 840 MB of the ~10 GB a forward moves, and the two launches took 0.36 ms of 3.9.  Here it never leaves the CU:
//   * a workgroup (4 waves) owns a 4 x 16 tile of layer-1 pixels.  It needs a 9 x 33 patch of layer-0 pixels, which
//     needs a 19 x 67 x 3 image patch (68 columns are loaded so that every piece is an aligned group of 4 pixels);
//   * layer 0 runs on v_mfma_f32_32x32x16_f16 exactly like conv_first.hip (image_conv.h: pixel-interleaved patch with a
//     zero 4th channel, K = 36 -> 48, a lane's B fragment = two 8-byte LDS reads), bias + SiLU, rounds to f16 -- the same values the unfused path stores -- and parks the
//     patch in LDS ([row][column parity][column / 2][C0], 16-byte chunks XOR-swizzled).  Patch positions outside the
//     layer-0 map are layer 1's zero padding and are stored as zeros;
//   * layer 1 reads its B fragments straight from that patch (stride-2 taps = consecutive entries of one parity
//     plane) and keeps its weights -- the A operand, 9*C0/16 fragments per wave -- in registers for the whole launch;
//   * workgroups are persistent (grid = 3 per CU) and fetch the next tile's image patch into registers before they
//     start computing the current one, so HBM latency hides under the MFMA / LDS work; stores go through an LDS tile
//     as coalesced 16-byte pieces.
// Accumulation order (K ascending in 16-wide MFMA steps, k = (kh, kw, c)) equals conv_first.hip's and conv_gemm.hip's,
// so the result is bit-identical to the unfused pair (tests/test_gpu_parity.py::test_stem_fused_matches_unfused_and_oracle).
#include "fused_tile.h"
#include "image_conv.h"

#define ST_TH 4
#define ST_TW 16
#define ST_R0 (2 * ST_TH + 1)   // 9 layer-0 rows
#define ST_C0W (2 * ST_TW + 1)  // 33 layer-0 columns
#define ST_NE (ST_R0 * ST_C0W)  // 297 layer-0 patch entries
#define ST_NMT ((ST_NE + 31) / 32)  // 10 MFMA pixel tiles of layer 0
#define ST_EV (ST_TW + 1)       // 17 even-parity columns per patch row (then 16 odd ones)
#define ST_IR (2 * ST_R0 + 1)   // 19 image rows
#define ST_NG 17                // 4-pixel groups per image row (68 columns, first = image column 4*ox0 - 4)
#define ST_ROWPX (4 * ST_NG)    // 68 patch pixels per row (8 bytes each: 3 channels + zero)
#define ST_NITEM (ST_IR * ST_NG)  // 323 load items (4 px x 3 ch) per tile
#define ST_NLOAD ((ST_NITEM + 255) / 256)

struct StemK {
    const void* img;
    const half_t* w0;
    const float* b0;
    const half_t* w1;
    const float* b1;
    half_t* dst;
    int B, H, W, OH0, OW0, OH1, OW1, ldd, Kpad1, act;
    TileGrid grid;
};

// f32 images: the prefetched patch items are twice as wide; at three workgroups per CU (168 VGPRs) the kernel spilled 13 registers -> two
#define BSY_K(n) n
#define BSY_RELU false
#include "stem_fused_kernel.h"
#undef BSY_K
#undef BSY_RELU
#define BSY_K(n) n##_relu
#define BSY_RELU true
#include "stem_fused_kernel.h"
#undef BSY_K
#undef BSY_RELU

bool stem_fused_supported(int C0, int C1, int H, int W) {
    return ((C0 == 32 && C1 == 64) || (C0 == 16 && C1 == 32)) && !(W & 3) && H >= 4 && W >= 4;
}

template <typename T>
static int launch_t(const StemArgs& a, const StemK& k, hipStream_t s) {
    const int slots = sizeof(T) == 4 ? 512 : 768;      // 3 workgroups per CU (register-limited: a fourth needs <= 128 VGPRs and spills 61; f32 images: 2), tiles dealt round-robin
    const int grid = persistent_grid(k.grid.ntiles, slots);
    if (a.C0 == 32) { if (k.act == 2) hipLaunchKernelGGL((stem_fused_kernel_relu<T, 32, 64>), dim3(grid), dim3(256), 0, s, k); else hipLaunchKernelGGL((stem_fused_kernel<T, 32, 64>), dim3(grid), dim3(256), 0, s, k); }
    else { if (k.act == 2) hipLaunchKernelGGL((stem_fused_kernel_relu<T, 16, 32>), dim3(grid), dim3(256), 0, s, k); else hipLaunchKernelGGL((stem_fused_kernel<T, 16, 32>), dim3(grid), dim3(256), 0, s, k); }
    HIP_TRY(hipGetLastError());
    return BSY_OK;
}

int launch_stem_fused(const StemArgs& a, hipStream_t s) {
    if (!stem_fused_supported(a.C0, a.C1, a.H, a.W))
        BSY_FAIL(BSY_ERR_ARG, "stem: unsupported shape (C0 %d, C1 %d, H %d, W %d): need (32,64) or (16,32) channels, W %% 4 == 0", a.C0, a.C1, a.H, a.W);
    const int OH0 = (a.H - 1) / 2 + 1, OW0 = (a.W - 1) / 2 + 1;
    const int OH1 = (OH0 - 1) / 2 + 1, OW1 = (OW0 - 1) / 2 + 1;
    if (a.OH != OH1 || a.OW != OW1) BSY_FAIL(BSY_ERR_ARG, "stem: output extent mismatch (%d x %d, expected %d x %d)", a.OH, a.OW, OH1, OW1);
    const int esz = a.img_dtype == BSY_F32 ? 4 : 2;
    if (((uintptr_t)a.img & (4 * esz - 1)) || !all_aligned16(a.dst, a.w0, a.w1, a.b0, a.b1) || (a.ldd & 7) || (a.Kpad1 & 7) || a.Kpad1 < 9 * a.C0 ||
        a.Kpad1 < 16 * ((9 * a.C0 + 15) / 16))
        BSY_FAIL(BSY_ERR_ARG, "stem: misaligned pointer / leading dimension");
    StemK k;
    k.img = a.img; k.w0 = (const half_t*)a.w0; k.b0 = a.b0; k.w1 = (const half_t*)a.w1; k.b1 = a.b1; k.dst = a.dst;
    k.B = a.B; k.H = a.H; k.W = a.W; k.OH0 = OH0; k.OW0 = OW0; k.OH1 = OH1; k.OW1 = OW1; k.ldd = a.ldd; k.Kpad1 = a.Kpad1;
    k.act = a.act;
    const int rc = make_tile_grid(k.grid, a.B, OH1, OW1, ST_TH, ST_TW, "stem");
    if (rc != BSY_OK) return rc;
    if (a.img_dtype == BSY_F16) return launch_t<half_t>(a, k, s);
    if (a.img_dtype == BSY_F32) return launch_t<float>(a, k, s);
    BSY_FAIL(BSY_ERR_ARG, "stem: image dtype %d unsupported", a.img_dtype);
}
