// Reflected bilinear sampling of u8 HWC images, as the view kernels state it (lf_tta.hip, lf_policy.hip): the taps of
// a source coordinate, the three lerps on the bytes as floats, and lf_augment.hip's pack arithmetic on the result.
// Both files are built without FMA contraction (Makefile, NO_CONTRACT): with an integer coordinate the weights are 0
// and what comes out is the source byte itself.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace lf {

// position of index i in its period of 2n (fill_mode="reflect", lf_nn.hip's reflect_idx: d c b a | a b c d | d c b a),
// for any number of periods and negative i; most indices lie inside the first period and skip the division
__device__ __forceinline__ int period_pos(int i, int period) {
    if ((unsigned)i >= (unsigned)period) {
        i %= period;
        if (i < 0) i += period;
    }
    return i;
}
__device__ __forceinline__ int fold(int m, int n) { return m < n ? m : 2 * n - 1 - m; }

// floor(f) and its neighbour, both reflected into [0, n); *frac = f - floor(f).  A coordinate beyond +-2^30 (a
// zoom or shift of that size) is held there, so that the integer arithmetic stays defined; the indices are in range
// whatever f is, a NaN included.
__device__ __forceinline__ void taps(float f, int n, int* i0, int* i1, float* frac) {
    const float f0 = floorf(f);
    *frac = f - f0;
    const int period = 2 * n;
    const int m = period_pos((int)fminf(fmaxf(f0, -1073741824.f), 1073741824.f), period);
    *i0 = fold(m, n);
    *i1 = fold(m + 1 == period ? 0 : m + 1, n);
}

// channel c of the 2 x 2 footprint (rows r0, r1 of the source, columns xs[0], xs[1]) at the weights (ax, ay)
__device__ __forceinline__ float bilerp_u8(const uint8_t* r0, const uint8_t* r1, const int (&xs)[2], int c, float ax,
                                           float ay) {
    const float v00 = r0[xs[0] * 3 + c], v01 = r0[xs[1] * 3 + c];
    const float v10 = r1[xs[0] * 3 + c], v11 = r1[xs[1] * 3 + c];
    const float top = v00 + (v01 - v00) * ax, bot = v10 + (v11 - v10) * ax;
    return top + (bot - top) * ay;
}

// lf_pack_hwc_u8_to_nchw_f32's normalisation (lf_augment.hip): the division and the subtraction round on their own
template <bool NORM>
__device__ __forceinline__ float pack_norm(float v, float mean, float denom) {
    return NORM ? __fdiv_rn(__fsub_rn(v, mean), denom) : v;
}
// and its whole pack_value on a byte (or an interpolated byte)
template <bool NORM>
__device__ __forceinline__ float pack_value(float byte, float mean, float denom) {
    return pack_norm<NORM>(__fdiv_rn(byte, 255.0f), mean, denom);
}

}  // namespace lf
