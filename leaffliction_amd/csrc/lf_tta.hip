// libleafhip — test-time augmentation: one batch of model inputs -> v views of every image in one launch
// (lf_tta_views_f32), and the v probability rows of every image folded back into one answer (lf_tta_combine_f32).
// The two rules are stated in include/leafhip.h and DESIGN.md.
//
// Built without FMA contraction (Makefile, NO_CONTRACT): a view row with cos = 1, sin = 0, zoom = 1 and integer
// shifts has integer source coordinates in exact arithmetic, every product and sum below is then exact in fp32, the
// interpolation weights are 0, and what is stored is pack_value's arithmetic (lf_sample.h) on the source byte:
// lf_pack_hwc_u8_to_nchw_f32 of the moved image, bit for bit.
#include <limits.h>
#include <math.h>

#include "lf_common.h"
#include "lf_sample.h"
#include "lf_wave.h"

namespace {

using lf::kHeadMaxClasses;
using lf::pack_value;
using lf::take_larger;
using lf::taps;
using lf::wave_argmax_all;

constexpr int kBlock = 256;
constexpr int kMaxViews = 16;

// the view rows as a kernel argument: uniform over the launch, read through scalar registers
struct ViewRows {
    float r[kMaxViews][6];   // {flip, cos, sin, zoom, dy, dx}
};
struct ViewWeights {
    float w[kMaxViews];
};

// One thread = one output pixel, for all v views of its image one after the other: grid = (pixel blocks, images), and
// the blocks of one image are neighbours in one XCD's dispatch sequence (lf::xcd_block2), so the 3*h*w source bytes of
// an image are fetched into one L2 and read there by all its views while they are hot.  The writes are the traffic
// (4*v output bytes per input byte): a wave stores 256 contiguous bytes per plane and view.  What bounds the kernel is
// the gather, twelve bytes per pixel and view through the L1: with neighbouring lanes on neighbouring pixels a wave's
// taps fall into two or three cache lines of each source row.  Four consecutive pixels per thread and one 16-byte
// store per plane were measured and are slower, 4.02 against 3.08 ms for 14 views of 1,024 x 224 x 224, because a
// wave's taps then spread over four times as many lines.
template <bool NORM, bool NT>
__global__ __launch_bounds__(kBlock) void tta_views_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                           int h, int w, int v, ViewRows rows, float m0, float m1,
                                                           float m2, float d0, float d1, float d2) {
    const lf::Block2 blk = lf::xcd_block2();
    const size_t hw = (size_t)h * w;
    const size_t p = (size_t)blk.x * kBlock + threadIdx.x;
    if (p >= hw) return;
    const uint8_t* src = in + (size_t)blk.y * hw * 3;
    const float cx = (float)(w - 1) * 0.5f, cy = (float)(h - 1) * 0.5f;
    const float nm[3] = {m0, m1, m2}, nd[3] = {d0, d1, d2};
    const int oy = (int)(p / (unsigned)w), ox = (int)p - oy * w;
    const float u = (float)ox - cx, t = (float)oy - cy;
#pragma unroll 1
    for (int k = 0; k < v; ++k) {
        const float flip = rows.r[k][0], cs = rows.r[k][1], sn = rows.r[k][2], zoom = rows.r[k][3];
        const float dy = rows.r[k][4], dx = rows.r[k][5];
        const float fx = zoom * (cs * u - sn * t) + cx + dx;
        const float fy = zoom * (sn * u + cs * t) + cy + dy;
        int xs[2], ys[2];
        float ax, ay;
        taps(fx, w, &xs[0], &xs[1], &ax);
        taps(fy, h, &ys[0], &ys[1], &ay);
        if (flip != 0.f) {   // the flip precedes the rotation: sample the mirrored source
            xs[0] = w - 1 - xs[0];
            xs[1] = w - 1 - xs[1];
        }
        const uint8_t* r0 = src + (size_t)ys[0] * w * 3;
        const uint8_t* r1 = src + (size_t)ys[1] * w * 3;
        float* dst = out + ((size_t)blk.y * v + k) * 3 * hw + p;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lf::stg<NT>(dst + c * hw, pack_value<NORM>(lf::bilerp_u8(r0, r1, xs, c, ax, ay), nm[c], nd[c]));
        }
    }
}

// One workgroup = one wave per image.  Lane l owns the classes l, l + 64, ...: it averages them over the views in
// ascending order and keeps its best, the best of the wave is found by butterfly; then every counted view's own
// argmax the same way.
__global__ __launch_bounds__(64) void tta_combine_kernel(const float* __restrict__ probs, ViewWeights wt,
                                                         float wsum, int v, float* __restrict__ out,
                                                         int32_t* __restrict__ top, int32_t* __restrict__ agree,
                                                         int c) {
    const size_t i = blockIdx.x;
    const float* mine = probs + i * v * c;
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int j = threadIdx.x; j < c; j += 64) {
        float acc = 0.f;
#pragma unroll 1
        for (int k = 0; k < v; ++k) acc += wt.w[k] * mine[(size_t)k * c + j];
        const float mean = acc / wsum;
        out[i * c + j] = mean;
        take_larger(bv, bi, mean, j);
    }
    const int best = wave_argmax_all(bv, bi);
    int count = 0;
#pragma unroll 1
    for (int k = 0; k < v; ++k) {
        if (!(wt.w[k] > 0.f)) continue;   // uniform over the wave
        float kv = -INFINITY;
        int ki = INT_MAX;
        for (int j = threadIdx.x; j < c; j += 64) take_larger(kv, ki, mine[(size_t)k * c + j], j);
        count += wave_argmax_all(kv, ki) == best;
    }
    if (threadIdx.x == 0) {
        top[i] = best;
        agree[i] = count;
    }
}

}  // namespace

extern "C" {

int lf_tta_views_f32(const uint8_t* in, float* out, int n, int h, int w, const float* view6, int v,
                     const float* mean3, const float* denom3, lf_stream_t stream) {
    LF_REQUIRE(in && out && view6, "lf_tta_views: null buffer");
    LF_REQUIRE(n > 0 && h > 1 && w > 1, "lf_tta_views: bad dims n=%d h=%d w=%d", n, h, w);
    LF_REQUIRE(v >= 1 && v <= kMaxViews, "lf_tta_views: v=%d views (1..%d)", v, kMaxViews);
    LF_REQUIRE((long long)n * v <= 65535, "lf_tta_views: n*v=%lld rows (at most 65535)", (long long)n * v);
    LF_REQUIRE((size_t)h * w <= ((size_t)1 << 28), "lf_tta_views: image too large h=%d w=%d", h, w);
    LF_REQUIRE((mean3 == nullptr) == (denom3 == nullptr), "lf_tta_views: mean/denom must both be set");
    ViewRows rows = {};
    for (int k = 0; k < v; ++k) {
        for (int e = 0; e < 6; ++e) {
            LF_REQUIRE(isfinite(view6[6 * k + e]), "lf_tta_views: view %d holds a value that is not finite", k);
            rows.r[k][e] = view6[6 * k + e];
        }
        LF_REQUIRE(rows.r[k][3] != 0.f, "lf_tta_views: view %d has zoom 0", k);
    }
    float m[3], d[3];
    lf::norm_consts(mean3, denom3, m, d);
    const bool norm = mean3 != nullptr;
    hipStream_t s = lf::as_stream(stream);
    const size_t hw = (size_t)h * w;
    const bool nt = lf::streaming((size_t)n * hw * 3 * (1 + 4 * (size_t)v));
    const dim3 grid((unsigned)((hw + kBlock - 1) / kBlock), (unsigned)n);
    LF_REQUIRE((size_t)grid.x * n <= ((size_t)1 << 31), "lf_tta_views: batch too large n=%d h=%d w=%d", n, h, w);
    auto kern = norm ? (nt ? tta_views_kernel<true, true> : tta_views_kernel<true, false>)
                     : (nt ? tta_views_kernel<false, true> : tta_views_kernel<false, false>);
    kern<<<grid, kBlock, 0, s>>>(in, out, h, w, v, rows, m[0], m[1], m[2], d[0], d[1], d[2]);
    return lf::check_launch("lf_tta_views");
}

int lf_tta_combine_f32(const float* probs, const float* weight, int v, float* out, int32_t* top, int32_t* agree,
                       int n, int c, lf_stream_t stream) {
    LF_REQUIRE(probs && out && top && agree, "lf_tta_combine: null buffer");
    LF_REQUIRE(n > 0 && c > 0 && c <= kHeadMaxClasses, "lf_tta_combine: bad dims n=%d c=%d", n, c);
    LF_REQUIRE(v >= 1 && v <= kMaxViews, "lf_tta_combine: v=%d views (1..%d)", v, kMaxViews);
    ViewWeights wt = {};
    float wsum = 0.f;
    for (int k = 0; k < v; ++k) {
        wt.w[k] = weight != nullptr ? weight[k] : 1.f;
        LF_REQUIRE(isfinite(wt.w[k]) && wt.w[k] >= 0.f, "lf_tta_combine: weight %d is negative or not finite", k);
        wsum += wt.w[k];
    }
    LF_REQUIRE(wsum > 0.f && isfinite(wsum), "lf_tta_combine: the weights must have a positive finite sum");
    tta_combine_kernel<<<(unsigned)n, 64, 0, lf::as_stream(stream)>>>(probs, wt, wsum, v, out, top, agree, c);
    return lf::check_launch("lf_tta_combine");
}

}  // extern "C"
