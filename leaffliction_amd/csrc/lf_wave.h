// Wave and workgroup reductions, the plane kernels' storage helpers and the head's class limit, stated once for the
// units that reduce over a 64-lane wave: lf_nn.hip, lf_tta.hip, lf_calib.hip, lf_cam.hip, lf_novelty.hip and
// lf_augment.hip.  The
// tests derive their error bounds from these exact shuffle patterns and orders.  An inline helper is compiled with
// the flags of the unit that includes it (lf_tta, lf_calib and lf_augment are built without FMA contraction); none of
// them contains a product-sum, so the bits are the same everywhere.
#pragma once
#include "lf_common.h"

#if defined(__HIPCC__)
namespace lf {

constexpr int kHeadMaxClasses = 4096;   // classes of lf_head_*: what every consumer of probability rows accepts

// plane-kernel storage: float, or bf16 held as uint16_t
__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(uint16_t v) { return bf16_up(v); }
template <typename T>
__device__ __forceinline__ T narrow(float v);
template <>
__device__ __forceinline__ float narrow<float>(float v) { return v; }
template <>
__device__ __forceinline__ uint16_t narrow<uint16_t>(float v) { return bf16_down(v); }

// V consecutive elements moved as one access (a native vector: an array in a struct lets the compiler
// split the load and sink parts of it into a branch)
template <typename T, int V>
using Vec = T __attribute__((ext_vector_type(V)));

// sum over the 64-lane wave, result valid in lane 0
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// The same value in every lane of the 64-lane wave (xor butterfly: both partners of a step add / compare the same
// pair, so the lanes agree bit for bit).
template <typename T>
__device__ __forceinline__ T wave_sum_all(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max_all(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// the larger of two (value, index) pairs; the lower index on equal values (np.argmax)
__device__ __forceinline__ void take_larger(float& bv, int& bi, float ov, int oi) {
    if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
    }
}
// its twin: the smaller of two (value, index) pairs; the lower index on equal values (np.argmin)
__device__ __forceinline__ void take_smaller(float& bv, int& bi, float ov, int oi) {
    if (ov < bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
    }
}
// the wave's largest pair in every lane (xor butterfly, as wave_max_all): bv becomes its value, its index is returned
__device__ __forceinline__ int wave_argmax_all(float& bv, int bi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        take_larger(bv, bi, ov, oi);
    }
    return bi;
}

// Sums of K values over a workgroup of 256 threads; result valid in thread 0: the four wave partials of value k
// added as ((r0 + r1) + r2) + r3.  Every caller accumulates from +0.0, so no partial is -0.0 and this equals
// (((0 + r0) + r1) + r2) + r3 bit for bit, the order in which the double sums of BatchNorm's plane route and of the
// AdamW norm were first written.
template <int K, typename T>
__device__ __forceinline__ void block_sum(T (&v)[K], T* red /* [K][4] */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = wave_sum(v[k]);
        if (lane == 0) red[k * 4 + wid] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = red[k * 4] + red[k * 4 + 1] + red[k * 4 + 2] + red[k * 4 + 3];
    }
}

}  // namespace lf
#endif  // __HIPCC__

namespace lf {

// The model's normalisation constants as six floats for a kernel's argument list.  mean3 / denom3 are HOST pointers
// (3 floats each), both set or both null (no normalisation: mean 0, denominator 1).
inline void norm_consts(const float* mean3, const float* denom3, float (&m)[3], float (&d)[3]) {
    for (int c = 0; c < 3; ++c) {
        m[c] = mean3 != nullptr ? mean3[c] : 0.f;
        d[c] = mean3 != nullptr ? denom3[c] : 1.f;
    }
}

}  // namespace lf
