// The 2x2 max that maxpool.hip and the pooling epilogue of conv_first.hip share: ATen's max_pool2d update rule, taps in row-major
// order from -inf -- a value replaces the running maximum when it is greater OR a NaN, so a NaN wins and stays, and of +0 / -0 the
// first one met stays.  One definition: BSY_OP_FIRST_POOL returns the bits of CONV_FIRST -> MAXPOOL because both call this.
#pragma once
#include "common.h"

template <typename T> struct PoolVec;
template <> struct PoolVec<half_t> { typedef half8 vec; static constexpr int N = 8; };
template <> struct PoolVec<float> { typedef f32x4 vec; static constexpr int N = 4; };

template <typename T>
__device__ __forceinline__ typename PoolVec<T>::vec pool_max4(const typename PoolVec<T>::vec& a, const typename PoolVec<T>::vec& b,
                                                              const typename PoolVec<T>::vec& c, const typename PoolVec<T>::vec& d) {
    typename PoolVec<T>::vec o;
#pragma unroll
    for (int e = 0; e < PoolVec<T>::N; ++e) {
        const float v[4] = {(float)a[e], (float)b[e], (float)c[e], (float)d[e]};
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) m = ((v[t] > m) | (v[t] != v[t])) ? v[t] : m;
        o[e] = (T)m;  // one of the four inputs: the conversion back is exact
    }
    return o;
}
