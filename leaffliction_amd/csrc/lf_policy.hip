// libleafhip — the online augmentation policy's input stage (lf_input_stage_policy_f32): per image one projective
// warp, one colour transform and one erase box, u8 HWC -> f32 NCHW in one launch.  The rule is stated in
// include/leafhip.h and DESIGN.md.
//
// Built without FMA contraction (Makefile, NO_CONTRACT): every product, sum and division of the coordinates below
// rounds on its own, so numpy float32 restates them bit for bit (tests/policy_ref.py), and the rule's exact cases
// come for free:
//   - the identity row ({1,0,0,0,1,0,0,0}, M = I, t = 0, empty box): a*u = u, every other product is a zero, den = 1,
//     fx = u + cx = ox exactly; the weights are 0, the lerps return the byte, the colour sum is r + 0 + 0 + 0, and
//     what is stored is pack_value's arithmetic (lf_sample.h): lf_pack_hwc_u8_to_nchw_f32 bit for bit;
//   - a pure mirror (a = -1) or an integer translation (c, f integers) with the identity M: the coordinates are
//     integers again, so the output is the pack of the mirrored or moved (reflected) image bit for bit.
#include <math.h>

#include "lf_common.h"
#include "lf_sample.h"
#include "lf_wave.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRow = 24;            // floats per image: {a,b,c,d,e,f,g,k}, M (3x3, row-major), t (3), {y0,y1,x0,x1}
constexpr float kMinDen = 0.0625f;  // the projective denominator is held at 1/16 or above
constexpr float kMaxCoord = 1048576.f;  // source coordinates are held within +-2^20 before floor

// a source coordinate as the taps take it: finite and small enough for the index arithmetic whatever the row holds
// (fmaxf returns the other operand for a NaN)
__device__ __forceinline__ float held(float f) { return fminf(fmaxf(f, -kMaxCoord), kMaxCoord); }

// lf_tta.hip's views kernel for one view per image with the row read from memory: one thread = one output pixel and
// its three channels, grid = (pixel blocks, images), the blocks of an image neighbours in one XCD's dispatch sequence
// (lf::xcd_block2) so that its 3*h*w source bytes are fetched into one L2.  The row is uniform over the workgroup:
// its 24 floats arrive through scalar loads.  A wave stores 256 contiguous bytes per plane; the gather is twelve bytes
// per pixel through the L1, neighbouring lanes on neighbouring pixels, so a wave's taps fall into a few lines of each
// source row (more of them the stronger the warp).  An erased pixel reads nothing.
template <bool NORM, bool NT>
__global__ __launch_bounds__(kBlock) void input_policy_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                              const float* __restrict__ pol, int h, int w, float m0,
                                                              float m1, float m2, float d0, float d1, float d2) {
    const lf::Block2 blk = lf::xcd_block2();
    const size_t hw = (size_t)h * w;
    const size_t p = (size_t)blk.x * kBlock + threadIdx.x;
    if (p >= hw) return;
    const float* row = pol + (size_t)blk.y * kRow;
    const float nm[3] = {m0, m1, m2}, nd[3] = {d0, d1, d2};
    const int oy = (int)(p / (unsigned)w), ox = (int)p - oy * w;
    float* dst = out + (size_t)blk.y * 3 * hw + p;
    const float fox = (float)ox, foy = (float)oy;
    if (row[20] <= foy && foy < row[21] && row[22] <= fox && fox < row[23]) {   // a NaN edge: outside
#pragma unroll
        for (int c = 0; c < 3; ++c) lf::stg<NT>(dst + c * hw, 0.0f);
        return;
    }
    const float cx = (float)(w - 1) * 0.5f, cy = (float)(h - 1) * 0.5f;
    const float u = fox - cx, v = foy - cy;
    const float den = fmaxf(row[6] * u + row[7] * v + 1.0f, kMinDen);
    const float fx = held(__fdiv_rn(row[0] * u + row[1] * v + row[2], den) + cx);
    const float fy = held(__fdiv_rn(row[3] * u + row[4] * v + row[5], den) + cy);
    int xs[2], ys[2];
    float ax, ay;
    lf::taps(fx, w, &xs[0], &xs[1], &ax);
    lf::taps(fy, h, &ys[0], &ys[1], &ay);
    const uint8_t* src = in + (size_t)blk.y * hw * 3;
    const uint8_t* r0 = src + (size_t)ys[0] * w * 3;
    const uint8_t* r1 = src + (size_t)ys[1] * w * 3;
    float rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = __fdiv_rn(lf::bilerp_u8(r0, r1, xs, c, ax, ay), 255.0f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* mc = row + 8 + 3 * c;
        const float q = mc[0] * rgb[0] + mc[1] * rgb[1] + mc[2] * rgb[2] + row[17 + c];
        // fmaxf first: a NaN (a NaN or infinite entry of M or t) is read as 0
        lf::stg<NT>(dst + c * hw, lf::pack_norm<NORM>(fminf(fmaxf(q, 0.0f), 1.0f), nm[c], nd[c]));
    }
}

}  // namespace

extern "C" {

int lf_input_stage_policy_f32(const uint8_t* in, float* out, int n, int h, int w, const float* pol24,
                              const float* mean3, const float* denom3, lf_stream_t stream) {
    LF_REQUIRE(in && out && pol24, "lf_input_stage_policy: null buffer");
    LF_REQUIRE(n > 0 && n <= 65535, "lf_input_stage_policy: n=%d images (1..65535)", n);
    LF_REQUIRE(h > 1 && w > 1, "lf_input_stage_policy: bad dims h=%d w=%d (at least 2 x 2)", h, w);
    LF_REQUIRE((size_t)h * w <= ((size_t)1 << 28), "lf_input_stage_policy: image too large h=%d w=%d", h, w);
    LF_REQUIRE((mean3 == nullptr) == (denom3 == nullptr), "lf_input_stage_policy: mean/denom must both be set");
    float m[3], d[3];
    lf::norm_consts(mean3, denom3, m, d);
    for (int c = 0; c < 3; ++c) {
        LF_REQUIRE(isfinite(m[c]), "lf_input_stage_policy: mean %d is not finite", c);
        LF_REQUIRE(isfinite(d[c]) && d[c] != 0.f, "lf_input_stage_policy: denom %d is zero or not finite", c);
    }
    const bool norm = mean3 != nullptr;
    const size_t hw = (size_t)h * w;
    const bool nt = lf::streaming((size_t)n * hw * 3 * (1 + 4));
    const dim3 grid((unsigned)((hw + kBlock - 1) / kBlock), (unsigned)n);
    LF_REQUIRE((size_t)grid.x * n <= ((size_t)1 << 31), "lf_input_stage_policy: batch too large n=%d h=%d w=%d", n, h,
               w);
    auto kern = norm ? (nt ? input_policy_kernel<true, true> : input_policy_kernel<true, false>)
                     : (nt ? input_policy_kernel<false, true> : input_policy_kernel<false, false>);
    kern<<<grid, kBlock, 0, lf::as_stream(stream)>>>(in, out, pol24, h, w, m[0], m[1], m[2], d[0], d[1], d[2]);
    return lf::check_launch("lf_input_stage_policy");
}

}  // extern "C"
