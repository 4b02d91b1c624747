// Pose.kpts_decode's arithmetic per element (nn/modules/head.py:273-279, the non-export branch), shared by the stand-alone keypoint
// decode (pose.hip, bsy_kpts_decode) and the keypoint mode of the Detect decode launch (detect.hip): one text, so the two return the
// same bits.  Contraction is switched off inside every function: pose.hip is compiled without it, detect.hip with the default.
#pragma once
#include "common.h"

// The reference's expression per dtype.  fp32: (v * 2 + (ax - 0.5)) * stride, every operation rounded once.  fp16: torch rounds to
// fp16 after every operation, and the anchors and strides are fp16 tensors themselves (make_anchors takes the feature maps' dtype);
// a sum or product of two fp16 values rounded to fp32 and then to fp16 is the correctly rounded fp16 result, so the fp32 pipe
// with a conversion after each step returns those bits.  `a` is the anchor's integer cell coordinate (the anchor is a + 0.5).
__device__ __forceinline__ float kpt_xy(float v, float a, float stride) {
#pragma clang fp contract(off)
    return (v * 2.0f + (a + 0.5f - 0.5f)) * stride;
}
__device__ __forceinline__ half_t kpt_xy(half_t v, float a, float stride) {
#pragma clang fp contract(off)
    const half_t a16 = (half_t)((float)(half_t)(a + 0.5f) - 0.5f);
    const half_t t = (half_t)((float)v * 2.0f);
    const half_t s = (half_t)((float)t + (float)a16);
    return (half_t)((float)s * (float)(half_t)stride);
}
__device__ __forceinline__ float kpt_vis(float v) {
#pragma clang fp contract(off)
    return 1.0f / (1.0f + expf(-v));
}
__device__ __forceinline__ half_t kpt_vis(half_t v) {
#pragma clang fp contract(off)
    return (half_t)(1.0f / (1.0f + expf(-(float)v)));
}
