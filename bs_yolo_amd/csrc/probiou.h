// probiou of two oriented boxes in the reference's operation order (utils/metrics.py:261-278 _get_covariance_matrix, :327-358
// batch_probiou), shared by the rotated NMS (obb.hip) and the rotated validator matching (val_match.hip).  Both are compiled with
// -ffp-contract=off: every operation rounds on its own, as the fp32 torch ops do.
#pragma once
#include "common.h"

// _get_covariance_matrix (metrics.py:272-278): (w^2 / 12, h^2 / 12, theta) -> a cos^2 + b sin^2, a sin^2 + b cos^2, (a - b) cos sin,
// and clamp(a b - c^2, 0) as batch_probiou takes it under the square root (clamp_(0) keeps a NaN)
struct ObbCov {
    float a, b, c, det;
};

__device__ __forceinline__ ObbCov obb_covariance(const float w, const float h, const float th) {
    const float ga = (w * w) / 12.0f, gb = (h * h) / 12.0f;
    const float cs = cosf(th), sn = sinf(th);
    const float cos2 = cs * cs, sin2 = sn * sn;
    ObbCov r;
    r.a = ga * cos2 + gb * sin2;
    r.b = ga * sin2 + gb * cos2;
    r.c = ((ga - gb) * cs) * sn;
    const float d = r.a * r.b - r.c * r.c;
    r.det = d < 0.0f ? 0.0f : d;
    return r;
}

// batch_probiou (metrics.py:342-358) of obb1 = j and obb2 = i; each box as (x, y, a, b), c, det.  Not bit-symmetric in (j, i).
__device__ __forceinline__ float probiou(const f32x4 j0, const float jc, const float jd, const f32x4 i0, const float ic, const float id) {
    const float eps = 1e-7f;
    const float x1 = j0[0], y1 = j0[1], a1 = j0[2], b1 = j0[3];
    const float x2 = i0[0], y2 = i0[1], a2 = i0[2], b2 = i0[3];
    const float sa = a1 + a2, sb = b1 + b2, sc = jc + ic;
    const float dy = y1 - y2, dx = x1 - x2;
    const float core = sa * sb - sc * sc;
    const float t1 = ((sa * (dy * dy) + sb * (dx * dx)) / (core + eps)) * 0.25f;
    const float t2 = (((sc * (x2 - x1)) * dy) / (core + eps)) * 0.5f;
    const float t3 = logf(core / (4.0f * sqrtf(jd * id) + eps) + eps) * 0.5f;
    float bd = t1 + t2 + t3;
    bd = bd < eps ? eps : (bd > 100.0f ? 100.0f : bd);  // clamp(eps, 100); a NaN stays NaN
    const float hd = sqrtf(1.0f - expf(-bd) + eps);
    return 1.0f - hd;
}
