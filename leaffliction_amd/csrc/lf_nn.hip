// libleafhip — leaf_cnn non-conv kernels (NCHW): input stage (pack + in-model
// augmentation + Normalization), BatchNorm (train statistics / backward), Squeeze-Excite,
// residual tail (add + ReLU + SpatialDropout + MaxPool) forward/backward, GAP + Dense +
// softmax cross-entropy head, AdamW with per-tensor clipnorm + EMA, fp32 <-> bf16 casts.
//
// Activations are fp32.  The plane kernels (GAP, residual tail, GAP backward) also serve the
// mixed-precision step and bf16 inference on bf16 storage (template parameter T): arithmetic is
// fp32 after widening, values are rounded to bf16 (nearest even) exactly where they are stored,
// and every sum a later kernel relies on is taken over the stored values.
//
// All of these are HBM-bound streaming / reduction kernels: 16-byte accesses where the shape
// allows, one (n, c) plane per workgroup row so per-channel / per-sample parameters are uniform,
// and every cross-workgroup reduction goes through partial sums that are combined in a fixed
// order (deterministic; no float atomics).  Reference semantics: srcs/model/cnn.py:9-104,
// srcs/train/utils.py:17-57 (Keras 3 layer / optimizer definitions).
#include <float.h>

#include "lf_common.h"
#include "lf_wave.h"

namespace {

using lf::block_sum;
using lf::bn_dz1;
using lf::kHeadMaxClasses;
using lf::narrow;
using lf::Vec;
using lf::wave_max_all;
using lf::wave_sum_all;
using lf::widen;

constexpr int kBlock = 256;   // block_sum's workgroup
constexpr int kBnSplit = 64;  // partial sums per channel in the BN reductions

// the route bytes of N consecutive pooled values as one integer (byte k = value k)
template <int N>
using RouteWord = std::conditional_t<N == 4, unsigned, std::conditional_t<N == 2, uint16_t, uint8_t>>;

// ---------------------------------------------------------------------------
// input stage: u8 HWC -> [flip, rotate(bilinear, reflect), contrast] -> normalise -> f32 NCHW
// ---------------------------------------------------------------------------
// aug[n] = {flip, cos, sin, contrast}.  Sampling follows keras RandomFlip("horizontal") ->
// RandomRotation (affine about the image centre, bilinear, fill_mode="reflect") ->
// RandomContrast ((x - mean_hw) * f + mean_hw, clipped to [0, 255]) on the [0,1] image.
__device__ __forceinline__ int reflect_idx(int i, int n) {
    // fill_mode="reflect": (d c b a | a b c d | d c b a)
    const int period = 2 * n;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - 1 - i;
}

__device__ __forceinline__ void sample_aug(const uint8_t* __restrict__ src, int h, int w, int oy,
                                           int ox, float flip, float cs, float sn, float* rgb) {
    // output -> input coordinates (keras RandomRotation's projective matrix)
    const float wm = (float)(w - 1), hm = (float)(h - 1);
    const float xoff = (wm - (cs * wm - sn * hm)) * 0.5f;
    const float yoff = (hm - (sn * wm + cs * hm)) * 0.5f;
    const float fx = cs * ox - sn * oy + xoff;
    const float fy = sn * ox + cs * oy + yoff;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float ax = fx - x0f, ay = fy - y0f;
    int xs[2] = {reflect_idx((int)x0f, w), reflect_idx((int)x0f + 1, w)};
    const int ys[2] = {reflect_idx((int)y0f, h), reflect_idx((int)y0f + 1, h)};
    if (flip != 0.f) {  // the flip precedes the rotation: sample the mirrored source
        xs[0] = w - 1 - xs[0];
        xs[1] = w - 1 - xs[1];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v00 = src[((size_t)ys[0] * w + xs[0]) * 3 + c];
        const float v01 = src[((size_t)ys[0] * w + xs[1]) * 3 + c];
        const float v10 = src[((size_t)ys[1] * w + xs[0]) * 3 + c];
        const float v11 = src[((size_t)ys[1] * w + xs[1]) * 3 + c];
        const float top = v00 + (v01 - v00) * ax, bot = v10 + (v11 - v10) * ax;
        rgb[c] = (top + (bot - top) * ay) * (1.0f / 255.0f);
    }
}

// per-image channel sums of the flipped+rotated image (RandomContrast's mean), in kMeanSplit
// interleaved slices per image: grid = (kMeanSplit, n); input_aug_kernel adds the slices in order
constexpr int kMeanSplit = 8;
__global__ __launch_bounds__(kBlock) void aug_means_kernel(const uint8_t* __restrict__ in,
                                                           const float* __restrict__ aug,
                                                           float* __restrict__ means, int h, int w) {
    __shared__ float red[12];
    const int n = blockIdx.y;
    const uint8_t* src = in + (size_t)n * h * w * 3;
    const float flip = aug[4 * n], cs = aug[4 * n + 1], sn = aug[4 * n + 2];
    float acc[3] = {0.f, 0.f, 0.f};
    for (int p = blockIdx.x * kBlock + threadIdx.x; p < h * w; p += kMeanSplit * kBlock) {
        float rgb[3];
        sample_aug(src, h, w, p / w, p % w, flip, cs, sn, rgb);
        acc[0] += rgb[0];
        acc[1] += rgb[1];
        acc[2] += rgb[2];
    }
    block_sum<3>(acc, red);
    if (threadIdx.x == 0) {
        float* dst = means + ((size_t)n * kMeanSplit + blockIdx.x) * 3;
        dst[0] = acc[0];
        dst[1] = acc[1];
        dst[2] = acc[2];
    }
}

// The model view of one image: its source, its aug row and its contrast means (aug_means_kernel's slices added in
// order).  pixel() is the augmented value in the [0,1] domain, before normalisation.
struct AugView {
    const uint8_t* src;
    float flip, cs, sn, ct;
    float mu[3];

    __device__ __forceinline__ AugView(const uint8_t* __restrict__ in, const float* __restrict__ aug,
                                       const float* __restrict__ means, int n, size_t hw)
        : src(in + (size_t)n * hw * 3), flip(aug[4 * n]), cs(aug[4 * n + 1]), sn(aug[4 * n + 2]),
          ct(aug[4 * n + 3]), mu{0.f, 0.f, 0.f} {
        for (int k = 0; k < kMeanSplit; ++k) {
            const float* part = means + ((size_t)n * kMeanSplit + k) * 3;
            mu[0] += part[0];
            mu[1] += part[1];
            mu[2] += part[2];
        }
        const float inv = 1.0f / (float)hw;
        mu[0] *= inv;
        mu[1] *= inv;
        mu[2] *= inv;
    }

    __device__ __forceinline__ void pixel(int h, int w, int oy, int ox, float* v) const {
        float rgb[3];
        sample_aug(src, h, w, oy, ox, flip, cs, sn, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = fminf(fmaxf((rgb[c] - mu[c]) * ct + mu[c], 0.f), 255.f);
    }
};

__global__ __launch_bounds__(kBlock) void input_aug_kernel(const uint8_t* __restrict__ in,
                                                           float* __restrict__ out,
                                                           const float* __restrict__ aug,
                                                           const float* __restrict__ means, int h,
                                                           int w, float m0, float m1, float m2,
                                                           float d0, float d1, float d2) {
    const int n = blockIdx.y;
    const size_t hw = (size_t)h * w;
    float* dst = out + (size_t)n * hw * 3;
    const AugView own(in, aug, means, n, hw);
    const float nm[3] = {m0, m1, m2}, nd[3] = {d0, d1, d2};
    for (int p = blockIdx.x * kBlock + threadIdx.x; p < (int)hw; p += gridDim.x * kBlock) {
        float v[3];
        own.pixel(h, w, p / w, p % w, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[(size_t)c * hw + p] = (v[c] - nm[c]) / nd[c];
    }
}

// 0 for NaN and below 0, 1 above 1
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
// a mix row's partner as an index in [0, n) (NaN and negative values: 0)
__device__ __forceinline__ int mix_partner(float v, int n) { return (int)fminf(fmaxf(v, 0.f), (float)(n - 1)); }

// Mixup / CutMix (the rule: lf_input_stage_mix_f32 in leafhip.h), input_aug_kernel's layout: one pixel per thread,
// two model views of it blended with the weight of its side of the box.  A view whose weight is 0 is not sampled,
// and then the other one is stored as input_aug_kernel stores it, bit for bit.
__global__ __launch_bounds__(kBlock) void input_mix_kernel(const uint8_t* __restrict__ in,
                                                           float* __restrict__ out,
                                                           const float* __restrict__ aug,
                                                           const float* __restrict__ mix,
                                                           const float* __restrict__ means, int n_img,
                                                           int h, int w, float m0, float m1, float m2,
                                                           float d0, float d1, float d2) {
    const int n = blockIdx.y;
    const size_t hw = (size_t)h * w;
    float* dst = out + (size_t)n * hw * 3;
    const float* row = mix + 8 * (size_t)n;
    const float w_out = clamp01(row[1]), w_in = clamp01(row[2]);
    const float y0 = row[3], y1 = row[4], x0 = row[5], x1 = row[6];
    const AugView own(in, aug, means, n, hw);
    // built for every row on purpose, unmixed ones and partner == n included: 4 aug and 24 mean-slice loads per
    // thread, uniform over the workgroup, cost nothing measurable (173 against 172 us at 256 x 224^2) beside a branch
    const AugView other(in, aug, means, mix_partner(row[0], n_img), hw);
    const float nm[3] = {m0, m1, m2}, nd[3] = {d0, d1, d2};
    for (int p = blockIdx.x * kBlock + threadIdx.x; p < (int)hw; p += gridDim.x * kBlock) {
        const int oy = p / w, ox = p % w;
        const float fy = (float)oy, fx = (float)ox;
        const float wt = (fy >= y0 && fy < y1 && fx >= x0 && fx < x1) ? w_in : w_out;   // a NaN edge: outside
        float v[3];
        if (wt == 1.f) {
            own.pixel(h, w, oy, ox, v);
        } else if (wt == 0.f) {
            other.pixel(h, w, oy, ox, v);
        } else {
            float b[3];
            own.pixel(h, w, oy, ox, v);
            other.pixel(h, w, oy, ox, b);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = wt * v[c] + (1.f - wt) * b[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[(size_t)c * hw + p] = (v[c] - nm[c]) / nd[c];
    }
}

// yt'[i] = yt[partner] + t (yt[i] - yt[partner]); t = 1 keeps yt[i] and t = 0 takes yt[partner], both exactly
__global__ __launch_bounds__(kBlock) void mix_targets_kernel(const float* __restrict__ y,
                                                             const float* __restrict__ mix,
                                                             float* __restrict__ out, int n, int c) {
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= n * c) return;
    const int i = idx / c, j = idx - i * c;
    const float* row = mix + 8 * (size_t)i;
    const float t = clamp01(row[7]);
    const float yi = y[idx], yp = y[(size_t)mix_partner(row[0], n) * c + j];
    out[idx] = t == 1.f ? yi : yp + t * (yi - yp);
}

// ---------------------------------------------------------------------------
// plane-wise elementwise: out = act(x * scale[c] + shift[c])
// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(kBlock) void scale_shift_act_kernel(const float* __restrict__ x,
                                                                 float* __restrict__ out, int c,
                                                                 int hwv,
                                                                 const float* __restrict__ scale,
                                                                 const float* __restrict__ shift,
                                                                 int relu) {
    const int plane = blockIdx.x;
    const float sc = scale[plane % c], sh = shift[plane % c];
    const size_t base = (size_t)plane * hwv * VEC;
    for (int i = blockIdx.y * kBlock + threadIdx.x; i < hwv; i += gridDim.y * kBlock) {
        if (VEC == 4) {
            float4 v = reinterpret_cast<const float4*>(x + base)[i];
            v.x = fmaf(v.x, sc, sh); v.y = fmaf(v.y, sc, sh); v.z = fmaf(v.z, sc, sh); v.w = fmaf(v.w, sc, sh);
            if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            reinterpret_cast<float4*>(out + base)[i] = v;
        } else {
            float v = fmaf(x[base + i], sc, sh);
            out[base + i] = relu ? fmaxf(v, 0.f) : v;
        }
    }
}

// ---------------------------------------------------------------------------
// BatchNorm statistics (training): per-channel sum / sum of squares over N*H*W
// ---------------------------------------------------------------------------
// The BN reductions go through kBnSplit partial pairs per channel, part[C][kBnSplit][2]: a reduce kernel's thread 0
// stores the pair of its slice, a finalizer adds a channel's pairs in double, in slice order.
__device__ __forceinline__ void store_pair(float* __restrict__ part, int ch, int s, const float (&acc)[2]) {
    part[((size_t)ch * kBnSplit + s) * 2] = acc[0];
    part[((size_t)ch * kBnSplit + s) * 2 + 1] = acc[1];
}
__device__ __forceinline__ void sum_pairs(const float* __restrict__ part, int ch, double* s, double* q) {
    double a = 0.0, b = 0.0;
    for (int k = 0; k < kBnSplit; ++k) {
        a += part[((size_t)ch * kBnSplit + k) * 2];
        b += part[((size_t)ch * kBnSplit + k) * 2 + 1];
    }
    *s = a;
    *q = b;
}

// The V terms of one load as one addend: V = 4 is (t0 + t1) + (t2 + t3), and a term that is a product contracts
// with its own pair's sum, so the roundings do not depend on how the body around it is written.
template <int V, class F>
__device__ __forceinline__ float pair_fold(F&& term) {
    static_assert(V == 1 || V == 4, "pair_fold: one element or two pairs");
    if constexpr (V == 1)
        return term(0);
    else
        return (term(0) + term(1)) + (term(2) + term(3));
}

// grid = (kBnSplit, C): workgroup (s, c) reduces the planes n = s, s+kBnSplit, ... of channel c
// around a per-channel pivot (the first element) to keep sum-of-squares well conditioned.
// V = elements per load (4 needs hw % 4 == 0).
template <int V>
__global__ __launch_bounds__(kBlock) void bn_stats_kernel(const float* __restrict__ y, int n, int c,
                                                          int hw, float* __restrict__ part) {
    __shared__ float red[8];
    const int ch = blockIdx.y, s = blockIdx.x;
    const float pivot = y[(size_t)ch * hw];
    float acc[2] = {0.f, 0.f};
    for (int img = s; img < n; img += kBnSplit) {
        const Vec<float, V>* p = reinterpret_cast<const Vec<float, V>*>(y + ((size_t)img * c + ch) * hw);
        for (int i = threadIdx.x; i < hw / V; i += kBlock) {
            const Vec<float, V> v = p[i];
            float d[V];
#pragma unroll
            for (int e = 0; e < V; ++e) d[e] = v[e] - pivot;
            acc[0] += pair_fold<V>([&](int e) { return d[e]; });
            acc[1] += pair_fold<V>([&](int e) { return d[e] * d[e]; });
        }
    }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) store_pair(part, ch, s, acc);
}

// grid = (kBnSplit, C): workgroup (s, c) adds slice s of channel c's per-tile partial sums
// (written by the convolution epilogue, lf_conv2d_stats_f32) in a fixed order.
__global__ __launch_bounds__(kBlock) void bn_tile_reduce_kernel(const float* __restrict__ tile_part,
                                                                long long tiles,
                                                                float* __restrict__ part) {
    __shared__ float red[8];
    const int ch = blockIdx.y, s = blockIdx.x;
    const long long per = (tiles + kBnSplit - 1) / kBnSplit;
    const long long t0 = per * s, t1 = t0 + per < tiles ? t0 + per : tiles;
    const float2* src = reinterpret_cast<const float2*>(tile_part) + (size_t)ch * (size_t)tiles;
    float acc[2] = {0.f, 0.f};
    for (long long t = t0 + threadIdx.x; t < t1; t += kBlock) {
        const float2 v = src[t];
        acc[0] += v.x;
        acc[1] += v.y;
    }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) store_pair(part, ch, s, acc);
}

// One thread per channel: combine partials in double, produce mean / invstd / scale / shift and
// update the moving statistics (keras BatchNormalization: biased variance, momentum 0.99).
// `pivot_src[ch * pivot_stride]` is the value the partial sums were taken about (null = 0).
__global__ void bn_finalize_kernel(const float* __restrict__ pivot_src, int pivot_stride,
                                   const float* __restrict__ part, int c, double count, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float* __restrict__ mmean,
                                   float* __restrict__ mvar, float momentum, float eps,
                                   float* __restrict__ mean_o, float* __restrict__ invstd_o,
                                   float* __restrict__ scale_o, float* __restrict__ shift_o) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    double s, q;
    sum_pairs(part, ch, &s, &q);
    const double pivot = pivot_src != nullptr ? (double)pivot_src[(size_t)ch * pivot_stride] : 0.0;
    const double dm = s / count;
    double var = q / count - dm * dm;
    if (var < 0.0) var = 0.0;
    const float mean = (float)(pivot + dm);
    const float fvar = (float)var;
    const float invstd = 1.0f / sqrtf(fvar + eps);
    mean_o[ch] = mean;
    invstd_o[ch] = invstd;
    const float sc = gamma[ch] * invstd;
    scale_o[ch] = sc;
    shift_o[ch] = beta[ch] - mean * sc;
    mmean[ch] = mmean[ch] * momentum + mean * (1.0f - momentum);
    mvar[ch] = mvar[ch] * momentum + fvar * (1.0f - momentum);
}

__global__ void bn_infer_kernel(int c, const float* __restrict__ gamma,
                                const float* __restrict__ beta, const float* __restrict__ mmean,
                                const float* __restrict__ mvar, float eps,
                                float* __restrict__ scale_o, float* __restrict__ shift_o) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    const float sc = gamma[ch] / sqrtf(mvar[ch] + eps);
    scale_o[ch] = sc;
    shift_o[ch] = beta[ch] - mmean[ch] * sc;
}

// ---------------------------------------------------------------------------
// BatchNorm backward.  dz = (g * alpha[n,c] + beta[n,c]) masked by (mask > 0);
// xhat = (y - mean) * invstd.  Reduce: sum dz, sum dz*xhat per channel; apply:
// dy = gamma*invstd * (dz - sum_dz/M - xhat * sum_dzx/M).
// ---------------------------------------------------------------------------
struct BnBwdArgs {
    const float* g;      // upstream gradient [N][C][HW]
    const float* alpha;  // [N][C] or null (1)
    const float* addnc;  // [N][C] or null (0)
    const float* y;      // pre-BN activations
    const float* mean;
    const float* invstd;
    const float* scale;  // gamma*invstd, beta - mean*scale: the forward's BN apply
    const float* shift;
    int relu;            // 1: the BN was followed by ReLU -> gradient passes where y*scale+shift > 0
    int n, c, hw;
};

template <int V>
__global__ __launch_bounds__(kBlock) void bn_bwd_reduce_kernel(BnBwdArgs a, float* __restrict__ part) {
    __shared__ float red[8];
    const int ch = blockIdx.y, s = blockIdx.x;
    const float mean = a.mean[ch], invstd = a.invstd[ch], sc = a.scale[ch], sh = a.shift[ch];
    float acc[2] = {0.f, 0.f};
    for (int img = s; img < a.n; img += kBnSplit) {
        const size_t base = ((size_t)img * a.c + ch) * a.hw;
        const float al = a.alpha ? a.alpha[img * a.c + ch] : 1.f;
        const float ad = a.addnc ? a.addnc[img * a.c + ch] : 0.f;
        const Vec<float, V>* gv = reinterpret_cast<const Vec<float, V>*>(a.g + base);
        const Vec<float, V>* yv = reinterpret_cast<const Vec<float, V>*>(a.y + base);
        for (int i = threadIdx.x; i < a.hw / V; i += kBlock) {
            const Vec<float, V> g = gv[i], y = yv[i];
            float dz[V];
#pragma unroll
            for (int e = 0; e < V; ++e) dz[e] = bn_dz1(g[e], y[e], al, ad, sc, sh, a.relu);
            acc[0] += pair_fold<V>([&](int e) { return dz[e]; });
            acc[1] += pair_fold<V>([&](int e) { return dz[e] * ((y[e] - mean) * invstd); });
        }
    }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) store_pair(part, ch, s, acc);
}

// dy = coef2*dz + coef3*y + coef4 with dz masked by y*coef0+coef1 > 0: the apply step as five
// per-channel coefficients, for consumers that form dy while they read g and y.  One channel's five, from the
// dgamma / dbeta just formed (the floats stored).
__device__ __forceinline__ void bn_bwd_coef1(int ch, int c, float mean, float invstd, float scale, float shift,
                                             float gamma, float dgamma, float dbeta, float inv_count,
                                             float* __restrict__ coef) {
    const float k = gamma * invstd;
    const float mdz = dbeta * inv_count, mdzx = dgamma * inv_count;
    coef[ch] = scale;
    coef[c + ch] = shift;
    coef[2 * c + ch] = k;
    coef[3 * c + ch] = -k * invstd * mdzx;
    coef[4 * c + ch] = k * (mean * invstd * mdzx - mdz);
}

// what every route to a channel's backward sums needs to end: scale, shift, gamma and inv_count are read only with coef
struct BnBwdOut {
    const float* mean;
    const float* invstd;
    const float* scale;
    const float* shift;
    const float* gamma;
    float inv_count;
    float* dgamma;
    float* dbeta;
    float* coef;   // [5][C] or null
};

// a channel's two sums stored, and with `coef` its five coefficients from the floats just stored
__device__ __forceinline__ void bn_bwd_store(const BnBwdOut& o, int ch, int c, float db, float dg) {
    o.dbeta[ch] = db;
    o.dgamma[ch] = dg;
    if (o.coef != nullptr)
        bn_bwd_coef1(ch, c, o.mean[ch], o.invstd[ch], o.scale[ch], o.shift[ch], o.gamma[ch], dg, db, o.inv_count,
                     o.coef);
}

// One thread per channel: dbeta = s and dgamma = q from the kBnSplit partial pairs {s, q} of bn_bwd_reduce_kernel
// ({sum dz, sum dz*xhat}), or with about_mean from pairs {sum d, sum d*y} (convolution-epilogue tile sums,
// lf_conv2d_bnbwd_f32), which become dgamma = invstd * (q - mean * s).
__global__ void bn_bwd_finalize_kernel(const float* __restrict__ part, int c, int about_mean, BnBwdOut o) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    double s, q;
    sum_pairs(part, ch, &s, &q);
    const double dg = about_mean ? (q - (double)o.mean[ch] * s) * (double)o.invstd[ch] : q;
    bn_bwd_store(o, ch, c, (float)s, (float)dg);
}

template <int V>
__global__ __launch_bounds__(kBlock) void bn_bwd_apply_kernel(BnBwdArgs a,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ dgamma,
                                                              const float* __restrict__ dbeta,
                                                              float inv_count,
                                                              float* __restrict__ dy) {
    const int plane = blockIdx.x, ch = plane % a.c;
    const float mean = a.mean[ch], invstd = a.invstd[ch], sc = a.scale[ch], sh = a.shift[ch];
    const float k = gamma[ch] * invstd;
    const float mdz = dbeta[ch] * inv_count, mdzx = dgamma[ch] * inv_count;
    const float al = a.alpha ? a.alpha[plane] : 1.f;
    const float ad = a.addnc ? a.addnc[plane] : 0.f;
    const size_t base = (size_t)plane * a.hw;
    const Vec<float, V>* gv = reinterpret_cast<const Vec<float, V>*>(a.g + base);
    const Vec<float, V>* yv = reinterpret_cast<const Vec<float, V>*>(a.y + base);
    Vec<float, V>* ov = reinterpret_cast<Vec<float, V>*>(dy + base);
    for (int i = blockIdx.y * kBlock + threadIdx.x; i < a.hw / V; i += gridDim.y * kBlock) {
        const Vec<float, V> g = gv[i], y = yv[i];
        Vec<float, V> o;
#pragma unroll
        for (int e = 0; e < V; ++e)
            o[e] = k * (bn_dz1(g[e], y[e], al, ad, sc, sh, a.relu) - mdz - ((y[e] - mean) * invstd) * mdzx);
        ov[i] = o;
    }
}

// ---------------------------------------------------------------------------
// global average pool per plane, and its broadcast backward
// ---------------------------------------------------------------------------
// out[plane] = mean_hw act(x*scale[c]+shift[c]) (scale null = plain mean); with mask_sums also
// {count of x*scale+shift > 0, sum of x over those} per plane (BatchNorm backward needs them).
// V = elements per load; each load's values are summed in pairs, left to right.
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void gap_kernel(const T* __restrict__ x,
                                                     float* __restrict__ out, int hw, int c,
                                                     const float* __restrict__ scale,
                                                     const float* __restrict__ shift, int relu,
                                                     float* __restrict__ mask_sums) {
    __shared__ float red[12];
    const size_t base = (size_t)blockIdx.x * hw;
    const bool pro = scale != nullptr;
    const float sc = pro ? scale[blockIdx.x % c] : 1.f, sh = pro ? shift[blockIdx.x % c] : 0.f;
    float acc[3] = {0.f, 0.f, 0.f};
    auto one = [&](T e) {
        const float xv = widen(e);
        float v = xv;
        if (pro) {
            v = fmaf(xv, sc, sh);
            if (v > 0.f) {
                acc[1] += 1.f;
                acc[2] += xv;
            }
            if (relu) v = fmaxf(v, 0.f);
        }
        return v;
    };
    const Vec<T, V>* xv = reinterpret_cast<const Vec<T, V>*>(x + base);
    for (int i = threadIdx.x; i < hw / V; i += kBlock) {
        const Vec<T, V> v = xv[i];
        float s = one(v[0]);
        if constexpr (V > 1) {
            s += one(v[1]);
#pragma unroll
            for (int e = 2; e < V; e += 2) {
                const float a = one(v[e]);
                s += a + one(v[e + 1]);
            }
        }
        acc[0] += s;
    }
    block_sum<3>(acc, red);
    if (threadIdx.x == 0) {
        out[blockIdx.x] = acc[0] / (float)hw;
        if (mask_sums != nullptr) {
            mask_sums[2 * (size_t)blockIdx.x] = acc[1];
            mask_sums[2 * (size_t)blockIdx.x + 1] = acc[2];
        }
    }
}

// out[plane][:] = v[plane] * scale, V values per store
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void bcast_planes_kernel(const float* __restrict__ v,
                                                              T* __restrict__ out, int hw,
                                                              float scale) {
    Vec<T, V> o;
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = narrow<T>(v[blockIdx.x] * scale);
    Vec<T, V>* dst = reinterpret_cast<Vec<T, V>*>(out + (size_t)blockIdx.x * hw);
    for (int i = blockIdx.y * kBlock + threadIdx.x; i < hw / V; i += gridDim.y * kBlock) dst[i] = o;
}

// ---------------------------------------------------------------------------
// Squeeze-Excite FC pair (1x1 convs with bias on [N,C,1,1]): one workgroup per sample
// ---------------------------------------------------------------------------
// w1 [C][Cr], b1 [Cr], w2 [Cr][C], b2 [C]  (keras kernel [1,1,in,out] flattened)
__global__ __launch_bounds__(kBlock) void se_fwd_kernel(const float* __restrict__ m,
                                                        const float* __restrict__ w1,
                                                        const float* __restrict__ b1,
                                                        const float* __restrict__ w2,
                                                        const float* __restrict__ b2,
                                                        float* __restrict__ z1,
                                                        float* __restrict__ s, int c, int cr) {
    extern __shared__ float sm[];  // [c] m, [cr] z
    float* lm = sm;
    float* lz = sm + c;
    const int n = blockIdx.x;
    for (int i = threadIdx.x; i < c; i += kBlock) lm[i] = m[(size_t)n * c + i];
    __syncthreads();
    for (int j = threadIdx.x; j < cr; j += kBlock) {
        float acc = b1[j];
        for (int i = 0; i < c; ++i) acc = fmaf(lm[i], w1[(size_t)i * cr + j], acc);
        acc = fmaxf(acc, 0.f);
        lz[j] = acc;
        z1[(size_t)n * cr + j] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < c; i += kBlock) {
        float acc = b2[i];
        for (int j = 0; j < cr; ++j) acc = fmaf(lz[j], w2[(size_t)j * c + i], acc);
        s[(size_t)n * c + i] = 1.0f / (1.0f + __expf(-acc));
    }
}

// per sample: dpre2 = ds*s*(1-s); dpre1 = (dpre2 . w2^T) * (z1>0); dm = dpre1 . w1^T
__global__ __launch_bounds__(kBlock) void se_bwd_sample_kernel(
    const float* __restrict__ ds, const float* __restrict__ s, const float* __restrict__ z1,
    const float* __restrict__ w1, const float* __restrict__ w2, float* __restrict__ dpre2,
    float* __restrict__ dpre1, float* __restrict__ dm, int c, int cr, float dm_scale) {
    extern __shared__ float sm[];  // [c] dpre2, [cr] dpre1
    float* l2 = sm;
    float* l1 = sm + c;
    const int n = blockIdx.x;
    for (int i = threadIdx.x; i < c; i += kBlock) {
        const float sv = s[(size_t)n * c + i];
        const float v = ds[(size_t)n * c + i] * sv * (1.f - sv);
        l2[i] = v;
        dpre2[(size_t)n * c + i] = v;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < cr; j += kBlock) {
        float acc = 0.f;
        for (int i = 0; i < c; ++i) acc = fmaf(l2[i], w2[(size_t)j * c + i], acc);
        if (!(z1[(size_t)n * cr + j] > 0.f)) acc = 0.f;
        l1[j] = acc;
        dpre1[(size_t)n * cr + j] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < c; i += kBlock) {
        float acc = 0.f;
        for (int j = 0; j < cr; ++j) acc = fmaf(l1[j], w1[(size_t)i * cr + j], acc);
        dm[(size_t)n * c + i] = acc * dm_scale;
    }
}

// out[i][j] = sum_n a[n][i] * b[n][j]  (i < ra, j < rb); i == ra row holds sum_n b[n][j] (bias)
// One workgroup = 64 outputs x 4 batch slices (one wave each); slices combined in fixed order.
__global__ __launch_bounds__(kBlock) void outer_sum_kernel(const float* __restrict__ a,
                                                           const float* __restrict__ b,
                                                           float* __restrict__ out,
                                                           float* __restrict__ bias_out, int n,
                                                           int ra, int rb) {
    static_assert(kBlock == 256, "outer_sum_kernel: 4 waves");
    __shared__ float part[4][64];
    const int total = (ra + 1) * rb;
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + lane;
    const int per = (n + 3) / 4;
    const int k0 = slice * per, k1 = min(n, k0 + per);
    float acc = 0.f;
    if (t < total) {
        const int i = t / rb, j = t - i * rb;
        if (i < ra) {
#pragma unroll 8
            for (int k = k0; k < k1; ++k) acc = fmaf(a[(size_t)k * ra + i], b[(size_t)k * rb + j], acc);
        } else {
#pragma unroll 8
            for (int k = k0; k < k1; ++k) acc += b[(size_t)k * rb + j];
        }
    }
    part[slice][lane] = acc;
    __syncthreads();
    if (slice == 0 && t < total) {
        const float r = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
        const int i = t / rb, j = t - i * rb;
        if (i < ra)
            out[(size_t)i * rb + j] = r;
        else
            bias_out[j] = r;
    }
}

// ---------------------------------------------------------------------------
// residual tail: r = relu(sc' + a*s[n,c]); p = drop[n,c] * maxpool2x2(r)
// ---------------------------------------------------------------------------
// a = relu(y*a_scale[c]+a_shift[c]) when a_scale is given (BN2+ReLU fused), else a = y;
// sc' = act(sc*sc_scale[c] + sc_shift[c]) (projection BN, or the stem's BN+ReLU) or sc.
template <typename T>
struct TailArgs {
    const T* y;
    const float* a_scale;
    const float* a_shift;
    const float* s;
    const T* sc;
    const float* sc_scale;
    const float* sc_shift;
    const float* drop;
    int sc_relu;
    int c, h, w;
};

template <typename T>
__device__ __forceinline__ float tail_r(const TailArgs<T>& t, float yv, float scv, float as, float ab,
                                        float sv, float ks, float kb) {
    float a = yv;
    if (t.a_scale) a = fmaxf(fmaf(yv, as, ab), 0.f);
    float sh = scv;
    if (t.sc_scale) {
        sh = fmaf(scv, ks, kb);
        if (t.sc_relu) sh = fmaxf(sh, 0.f);
    }
    return fmaxf(sh + a * sv, 0.f);
}

// window code: bits 0-1 = position of the first maximum in scan order (0,0),(0,1),(1,0),(1,1);
// bit 2 = that maximum is > 0 (the gradient of the block's final ReLU)
__device__ __forceinline__ unsigned tail_code(float r00, float r01, float r10, float r11, float& best) {
    best = r00;
    unsigned bi = 0;
    if (r01 > best) { best = r01; bi = 1; }
    if (r10 > best) { best = r10; bi = 2; }
    if (r11 > best) { best = r11; bi = 3; }
    return bi | (best > 0.f ? 4u : 0u);
}

// One thread = two rows x V input pixels = V/2 pooled values and their route bytes.  The residual r
// is not stored: backward only needs where each pooled value came from.  route == null: no backward
// pass follows (inference).  Keep: the raw y and sc at the recorded position of each window also go out, at
// pooled size (y_at, sc_at; either may be null), so that the backward pass reads them there instead of
// gathering one pixel in four from the full-size planes.
template <typename T, int V, bool Keep = false>
__global__ __launch_bounds__(kBlock) void tail_fwd_kernel(TailArgs<T> t, uint8_t* __restrict__ route,
                                                          T* __restrict__ p, T* __restrict__ y_at = nullptr,
                                                          T* __restrict__ sc_at = nullptr) {
    const int plane = blockIdx.x, ch = plane % t.c;
    const float sv = t.s ? t.s[plane] : 1.f;
    const float as = t.a_scale ? t.a_scale[ch] : 1.f, ab = t.a_scale ? t.a_shift[ch] : 0.f;
    const float ks = t.sc_scale ? t.sc_scale[ch] : 1.f, kb = t.sc_scale ? t.sc_shift[ch] : 0.f;
    const float dv = t.drop ? t.drop[plane] : 1.f;
    const int h = t.h, w = t.w, ph = h / 2, pw = w / 2, pwv = w / V;
    const size_t base = (size_t)plane * h * w, pbase = (size_t)plane * ph * pw;
    for (int q = blockIdx.y * kBlock + threadIdx.x; q < ph * pwv; q += gridDim.y * kBlock) {
        const int py = q / pwv, pxv = q - py * pwv;
        float r[2][V];
        Vec<T, V> yv[2], scv[2];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const size_t o = base + (size_t)(2 * py + dy) * w + V * pxv;
            yv[dy] = *reinterpret_cast<const Vec<T, V>*>(t.y + o);
            scv[dy] = *reinterpret_cast<const Vec<T, V>*>(t.sc + o);
#pragma unroll
            for (int e = 0; e < V; ++e)
                r[dy][e] = tail_r(t, widen(yv[dy][e]), widen(scv[dy][e]), as, ab, sv, ks, kb);
        }
        const size_t po = pbase + (size_t)py * pw + (V / 2) * pxv;
        unsigned codes = 0;
        Vec<T, V / 2> pooled, ya, sa;
#pragma unroll
        for (int k = 0; k < V / 2; ++k) {
            float m;
            const unsigned cd = tail_code(r[0][2 * k], r[0][2 * k + 1], r[1][2 * k], r[1][2 * k + 1], m);
            codes |= cd << (8 * k);
            pooled[k] = narrow<T>(m * dv);
            if (Keep) {
                const bool low = (cd & 2u) != 0, right = (cd & 1u) != 0;
                const T y0 = right ? yv[0][2 * k + 1] : yv[0][2 * k], y1 = right ? yv[1][2 * k + 1] : yv[1][2 * k];
                const T s0 = right ? scv[0][2 * k + 1] : scv[0][2 * k], s1 = right ? scv[1][2 * k + 1] : scv[1][2 * k];
                ya[k] = low ? y1 : y0;
                sa[k] = low ? s1 : s0;
            }
        }
        if (route != nullptr) *reinterpret_cast<RouteWord<V / 2>*>(route + po) = (RouteWord<V / 2>)codes;
        *reinterpret_cast<Vec<T, V / 2>*>(p + po) = pooled;
        if (Keep && y_at != nullptr) *reinterpret_cast<Vec<T, V / 2>*>(y_at + po) = ya;
        if (Keep && sc_at != nullptr) *reinterpret_cast<Vec<T, V / 2>*>(sc_at + po) = sa;
    }
}

// a * b rounded on its own, whatever the compiler would contract it with
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// dr = dp*drop routed to the recorded position of each 2x2 window when its maximum was > 0.
// Per plane: ds = sum dr*a with a = relu(y*a_scale+a_shift) (or y), and (a_scale given)
// plane_sums = {sum dr*[a>0], sum dr*[a>0]*y}: BatchNorm-2's backward sums without a second pass;
// sc_sums = {sum dr, sum dr*sc_y} (the projection shortcut's BatchNorm).  The sums are over dr as
// stored.  One thread = V/2 pooled values -> two rows x V gradient pixels.  Kept: where y_at / sc_at
// (tail_fwd_kernel's pooled-size copies of y / sc_y at the recorded positions) are given, the sums read
// them in place of y[pos] / sc_y[pos]: the same values, without touching the full-size planes.
// The sums' roundings are stated (products rounded on their own in the two second moments, one fma in ds), so
// that every instantiation adds the same floats: left to the compiler, the contraction differed between them.
template <typename T, int V, bool Kept = false>
__global__ __launch_bounds__(kBlock) void tail_bwd_kernel(const T* __restrict__ dp,
                                                          const uint8_t* __restrict__ route,
                                                          const T* __restrict__ y,
                                                          const float* __restrict__ a_scale,
                                                          const float* __restrict__ a_shift,
                                                          const float* __restrict__ drop,
                                                          T* __restrict__ dr,
                                                          float* __restrict__ ds,
                                                          float* __restrict__ plane_sums,
                                                          const T* __restrict__ sc_y,
                                                          float* __restrict__ sc_sums, int c,
                                                          int h, int w, const T* __restrict__ y_at = nullptr,
                                                          const T* __restrict__ sc_at = nullptr) {
    __shared__ float red[20];
    const int plane = blockIdx.x, ch = plane % c;
    const float dv = drop ? drop[plane] : 1.f;
    const float as = a_scale ? a_scale[ch] : 1.f, ab = a_scale ? a_shift[ch] : 0.f;
    const int ph = h / 2, pw = w / 2, pwv = w / V;
    const size_t base = (size_t)plane * h * w, pbase = (size_t)plane * ph * pw;
    const bool sums = ds != nullptr || plane_sums != nullptr;
    const bool sc_on = sc_y != nullptr || (Kept && sc_at != nullptr);
    const bool y_kept = Kept && y_at != nullptr, sc_kept = Kept && sc_at != nullptr;
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    Vec<T, V / 2> ya, sa;   // Kept: y_at / sc_at of this thread's pooled values
    auto tally = [&](float gg, size_t pos, int k) {
        if (sc_on && gg != 0.f) {  // the shortcut branch's (projection) BN: no mask
            acc[3] += gg;
            acc[4] += mul_rounded(gg, widen(sc_kept ? sa[k] : sc_y[pos]));
        }
        if (sums && gg != 0.f) {
            const float yv = widen(y_kept ? ya[k] : y[pos]);
            float av = yv;
            if (a_scale) {
                av = fmaf(yv, as, ab);
                if (av > 0.f) {
                    acc[1] += gg;
                    acc[2] += mul_rounded(gg, yv);
                } else {
                    av = 0.f;
                }
            }
            acc[0] = fmaf(gg, av, acc[0]);
        }
    };
    for (int q = threadIdx.x; q < ph * pwv; q += kBlock) {
        const int py = q / pwv, pxv = q - py * pwv;
        const size_t po = pbase + (size_t)py * pw + (V / 2) * pxv;
        const unsigned codes = *reinterpret_cast<const RouteWord<V / 2>*>(route + po);
        const Vec<T, V / 2> g = *reinterpret_cast<const Vec<T, V / 2>*>(dp + po);
        const size_t o0 = base + (size_t)(2 * py) * w + V * pxv, o1 = o0 + w;
        if (y_kept && sums) ya = *reinterpret_cast<const Vec<T, V / 2>*>(y_at + po);
        if (sc_kept) sa = *reinterpret_cast<const Vec<T, V / 2>*>(sc_at + po);
        Vec<T, V> top, bot;
#pragma unroll
        for (int k = 0; k < V / 2; ++k) {   // pooled value k -> input columns 2k, 2k+1
            const unsigned cd = (codes >> (8 * k)) & 0xffu, b = cd & 3u;
            const T gk = (cd & 4u) ? narrow<T>(widen(g[k]) * dv) : T(0);
            top[2 * k] = b == 0 ? gk : T(0);
            top[2 * k + 1] = b == 1 ? gk : T(0);
            bot[2 * k] = b == 2 ? gk : T(0);
            bot[2 * k + 1] = b == 3 ? gk : T(0);
            tally(widen(gk), (b < 2 ? o0 : o1) + 2 * k + (b & 1u), k);
        }
        *reinterpret_cast<Vec<T, V>*>(dr + o0) = top;
        *reinterpret_cast<Vec<T, V>*>(dr + o1) = bot;
    }
    if ((h & 1) || (w & 1)) {
        for (int t = threadIdx.x; t < h * w; t += kBlock) {
            const int yy = t / w, x = t - yy * w;
            if (yy >= 2 * ph || x >= 2 * pw) dr[base + t] = T(0);
        }
    }
    if (sums || sc_on) {
        block_sum<5>(acc, red);
        if (threadIdx.x == 0) {
            if (ds != nullptr) ds[plane] = acc[0];
            if (plane_sums != nullptr) {
                plane_sums[2 * (size_t)plane] = acc[1];
                plane_sums[2 * (size_t)plane + 1] = acc[2];
            }
            if (sc_sums != nullptr) {
                sc_sums[2 * (size_t)plane] = acc[3];
                sc_sums[2 * (size_t)plane + 1] = acc[4];
            }
        }
    }
}

// BatchNorm backward sums from per-plane sums (no pass over the activation): with
// dz = (g*alpha + add) * [y*scale+shift > 0],
//   sum dz       = sum_n alpha*G0 + add*M0          G = tail_bwd plane sums {sum g*mask, sum g*mask*y}
//   sum dz*xhat  = invstd * sum_n alpha*(G1 - mean*G0) + add*(M1 - mean*M0)   M = gap mask sums
// one workgroup per channel, fixed-order double accumulation, then bn_bwd_store.
__global__ __launch_bounds__(kBlock) void bn_bwd_planes_kernel(const float* __restrict__ plane_g,
                                                               const float* __restrict__ plane_m,
                                                               const float* __restrict__ alpha,
                                                               const float* __restrict__ addnc, int n, int c,
                                                               BnBwdOut o) {
    __shared__ double red[8];
    const int ch = blockIdx.x;
    const double mu = o.mean[ch];
    double acc[2] = {0.0, 0.0};
    for (int img = threadIdx.x; img < n; img += kBlock) {
        const size_t pl = (size_t)img * c + ch;
        const double al = alpha ? alpha[pl] : 1.0, ad = addnc ? addnc[pl] : 0.0;
        const double g0 = plane_g[2 * pl], g1 = plane_g[2 * pl + 1];
        const double m0 = plane_m ? plane_m[2 * pl] : 0.0, m1 = plane_m ? plane_m[2 * pl + 1] : 0.0;
        acc[0] += al * g0 + ad * m0;
        acc[1] += al * (g1 - mu * g0) + ad * (m1 - mu * m0);
    }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) bn_bwd_store(o, ch, c, (float)acc[0], (float)(acc[1] * (double)o.invstd[ch]));
}

// ---------------------------------------------------------------------------
// head: logits = (g*drop) W + b; softmax; label-smoothed cross-entropy (keras semantics)
// ---------------------------------------------------------------------------
// one workgroup (64 threads) per sample; `feat` is the (dropped-out) GAP feature vector
__global__ void head_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                const float* __restrict__ b, const float* __restrict__ ytrue,
                                float* __restrict__ probs, float* __restrict__ loss, int f, int c) {
    extern __shared__ float sm[];  // [c] logits
    const int n = blockIdx.x;
    for (int j = threadIdx.x; j < c; j += blockDim.x) {
        float acc = b[j];
        for (int i = 0; i < f; ++i) acc = fmaf(feat[(size_t)n * f + i], w[(size_t)i * c + j], acc);
        sm[j] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float mx = sm[0];
        for (int j = 1; j < c; ++j) mx = fmaxf(mx, sm[j]);
        float den = 0.f;
        for (int j = 0; j < c; ++j) den += expf(sm[j] - mx);
        float l = 0.f;
        for (int j = 0; j < c; ++j) {
            const float pr = expf(sm[j] - mx) / den;
            probs[(size_t)n * c + j] = pr;
            if (ytrue != nullptr) {
                // keras categorical_crossentropy: clip to [1e-7, 1-1e-7] then -sum y log p
                const float pc = fminf(fmaxf(pr, 1e-7f), 1.f - 1e-7f);
                l -= ytrue[(size_t)n * c + j] * logf(pc);
            }
        }
        if (loss != nullptr) loss[n] = l;
    }
}

// Distillation head: the head above plus the soft-target term at temperature T.
//   p = softmax(z), p_T = softmax(z/T), q_T = softmax(lt/T), lt = log(max(tprobs, FLT_MIN))
//   hard = -sum y log(clip(p)),  kd = T^2 sum q_T (log q_T - log p_T),  loss = (1-alpha) hard + alpha kd
// One workgroup = one wave per sample.  Lane l owns the classes l, l+64, ...: it writes their logits and teacher
// logs to LDS and is the only lane that reads them back, and the three maxima, three sums and the two loss terms
// cross the lanes by butterfly, so no class is walked serially.  Both logs of kd are log-softmax values
// (exponent minus log-sum-exp).
__global__ __launch_bounds__(64) void head_distill_fwd_kernel(
    const float* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ b,
    const float* __restrict__ ytrue, const float* __restrict__ tprobs, float inv_t, float t2, float alpha,
    float* __restrict__ probs, float* __restrict__ soft, float* __restrict__ loss, float* __restrict__ kd, int f,
    int c) {
    extern __shared__ float sm[];  // [c] logits, [c] teacher logs
    float* lt = sm + c;
    const int n = blockIdx.x;
    const size_t row = (size_t)n * c;
    float mz = -INFINITY, ml = -INFINITY;
    for (int j = threadIdx.x; j < c; j += 64) {
        float acc = b[j];
        for (int i = 0; i < f; ++i) acc = fmaf(feat[(size_t)n * f + i], w[(size_t)i * c + j], acc);
        const float l = logf(fmaxf(tprobs[row + j], FLT_MIN));
        sm[j] = acc;
        lt[j] = l;
        mz = fmaxf(mz, acc);
        ml = fmaxf(ml, l);
    }
    mz = wave_max_all(mz);
    ml = wave_max_all(ml);
    float den = 0.f, den_t = 0.f, den_q = 0.f;
    for (int j = threadIdx.x; j < c; j += 64) {
        const float dz = sm[j] - mz;
        den += expf(dz);
        den_t += expf(dz * inv_t);
        den_q += expf((lt[j] - ml) * inv_t);
    }
    den = wave_sum_all(den);
    den_t = wave_sum_all(den_t);
    den_q = wave_sum_all(den_q);
    const float lse_t = logf(den_t), lse_q = logf(den_q);
    float hard = 0.f, kl = 0.f;
    for (int j = threadIdx.x; j < c; j += 64) {
        const float dz = sm[j] - mz;
        const float pr = expf(dz) / den;
        probs[row + j] = pr;
        // keras categorical_crossentropy: clip to [1e-7, 1-1e-7] then -sum y log p
        const float pc = fminf(fmaxf(pr, 1e-7f), 1.f - 1e-7f);
        hard -= ytrue[row + j] * logf(pc);
        const float et = dz * inv_t, eq = (lt[j] - ml) * inv_t;
        const float qt = expf(eq) / den_q;
        soft[row + j] = expf(et) / den_t - qt;
        kl += qt * ((eq - lse_q) - (et - lse_t));
    }
    hard = wave_sum_all(hard);
    kl = wave_sum_all(kl) * t2;
    if (threadIdx.x == 0) {
        loss[n] = (1.f - alpha) * hard + alpha * kl;
        if (kd != nullptr) kd[n] = kl;
    }
}

// Weighted head: class weights cw (null = none) and the focal modulating factor.
//   p = softmax(z), s = sum_j cw_j y_j (1 without cw), m_j = (1 - p_j)^gamma (1 at gamma == 0),
//   loss = s sum_j -y_j m_j log(clip(p_j))
// One workgroup = one wave per sample, laid out as head_distill_fwd_kernel: lane l owns the classes l, l+64, ...,
// writes their logits to LDS and is the only lane that reads them back; the maximum and the three sums cross the
// lanes by butterfly.  p_j <= 1 holds for what this kernel computes (the denominator contains the numerator and
// float sums of non-negative terms are monotone); the fmaxf keeps powf's base non-negative all the same.
__global__ __launch_bounds__(64) void head_focal_fwd_kernel(
    const float* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ b,
    const float* __restrict__ ytrue, const float* __restrict__ cw, float gamma, float* __restrict__ probs,
    float* __restrict__ loss, float* __restrict__ sw, int f, int c) {
    extern __shared__ float sm[];  // [c] logits
    const int n = blockIdx.x;
    const size_t row = (size_t)n * c;
    float mz = -INFINITY;
    for (int j = threadIdx.x; j < c; j += 64) {
        float acc = b[j];
        for (int i = 0; i < f; ++i) acc = fmaf(feat[(size_t)n * f + i], w[(size_t)i * c + j], acc);
        sm[j] = acc;
        mz = fmaxf(mz, acc);
    }
    mz = wave_max_all(mz);
    float den = 0.f;
    for (int j = threadIdx.x; j < c; j += 64) den += expf(sm[j] - mz);
    den = wave_sum_all(den);
    float l = 0.f, s = 0.f;
    for (int j = threadIdx.x; j < c; j += 64) {
        const float pr = expf(sm[j] - mz) / den;
        probs[row + j] = pr;
        const float yv = ytrue[row + j];
        // keras categorical_crossentropy: clip to [1e-7, 1-1e-7] then -sum y log p; the factor takes the unclipped p
        const float pc = fminf(fmaxf(pr, 1e-7f), 1.f - 1e-7f);
        const float m = gamma == 0.f ? 1.f : powf(fmaxf(1.f - pr, 0.f), gamma);
        l -= yv * m * logf(pc);
        if (cw != nullptr) s = fmaf(cw[j], yv, s);
    }
    l = wave_sum_all(l);
    s = cw != nullptr ? wave_sum_all(s) : 1.f;
    if (threadIdx.x == 0) {
        loss[n] = s * l;
        if (sw != nullptr) sw[n] = s;
    }
}

// The weighted head's backward, unclipped as head_bwd_kernel's:
//   l_j = log(max(p_j, FLT_MIN)), q_j = max(1 - p_j, 0), r_j = q_j^(gamma-1)   (powf(0, 0) = 1)
//   u_j = y_j (gamma r_j p_j l_j - r_j q_j)   (-y_j at gamma == 0),  dlogits_k = s (u_k - p_k sum_j u_j) inv_n
// One wave per sample; lane l owns u of the classes l, l+64, ... in LDS until dlogits replaces it, and after the
// barrier every lane reads the whole row for dfeat = dlogits W^T (as head_bwd_kernel); (dW, db) by outer_sum_kernel.
__global__ __launch_bounds__(64) void head_focal_bwd_kernel(
    const float* __restrict__ probs, const float* __restrict__ ytrue, const float* __restrict__ cw, float gamma,
    const float* __restrict__ w, float* __restrict__ dlogits, float* __restrict__ dfeat, int f, int c,
    float inv_n) {
    extern __shared__ float sm[];  // [c] u, then dlogits
    const int n = blockIdx.x;
    const size_t row = (size_t)n * c;
    float su = 0.f, s = 0.f;
    for (int j = threadIdx.x; j < c; j += 64) {
        const float pr = probs[row + j], yv = ytrue[row + j];
        float u = -yv;
        if (gamma != 0.f) {
            const float q = fmaxf(1.f - pr, 0.f);
            const float r = powf(q, gamma - 1.f);
            u = yv * (gamma * r * pr * logf(fmaxf(pr, FLT_MIN)) - r * q);
        }
        sm[j] = u;
        su += u;
        if (cw != nullptr) s = fmaf(cw[j], yv, s);
    }
    su = wave_sum_all(su);
    s = cw != nullptr ? wave_sum_all(s) : 1.f;
    for (int j = threadIdx.x; j < c; j += 64) {
        const float d = s * (sm[j] - probs[row + j] * su) * inv_n;
        sm[j] = d;
        dlogits[row + j] = d;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < f; i += 64) {
        float acc = 0.f;
        for (int j = 0; j < c; ++j) acc = fmaf(sm[j], w[(size_t)i * c + j], acc);
        dfeat[(size_t)n * f + i] = acc;
    }
}

// dlogits = (probs - ytrue) * inv_n, or with kDistill
//   [(1-alpha)(probs - ytrue) + alpha T soft] * inv_n   (hard_w = 1-alpha, soft_w = alpha T);
// dfeat = dlogits W^T; (dW, db) by outer_sum_kernel
template <bool kDistill>
__global__ void head_bwd_kernel(const float* __restrict__ probs, const float* __restrict__ ytrue,
                                const float* __restrict__ soft, float hard_w, float soft_w,
                                const float* __restrict__ w, float* __restrict__ dlogits,
                                float* __restrict__ dfeat, int f, int c, float inv_n) {
    extern __shared__ float sm[];  // [c]
    const int n = blockIdx.x;
    for (int j = threadIdx.x; j < c; j += blockDim.x) {
        float d = probs[(size_t)n * c + j] - ytrue[(size_t)n * c + j];
        if (kDistill) d = hard_w * d + soft_w * soft[(size_t)n * c + j];
        d *= inv_n;
        sm[j] = d;
        dlogits[(size_t)n * c + j] = d;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < f; i += blockDim.x) {
        float acc = 0.f;
        for (int j = 0; j < c; ++j) acc = fmaf(sm[j], w[(size_t)i * c + j], acc);
        dfeat[(size_t)n * f + i] = acc;
    }
}

__global__ __launch_bounds__(kBlock) void mul_kernel(const float* __restrict__ a,
                                                     const float* __restrict__ b,
                                                     float* __restrict__ out, size_t count) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < count;
         i += (size_t)gridDim.x * kBlock)
        out[i] = a[i] * b[i];
}

// ---------------------------------------------------------------------------
// AdamW (keras 3): per-tensor clipnorm, L2-regulariser gradient, decoupled weight decay,
// bias-corrected Adam, EMA of the updated weights.  Flat buffers + a segment table.
// ---------------------------------------------------------------------------
// norms: one workgroup per tensor: sum over (g + 2*l2*w)^2
// squared gradient norm of tensor t in kNormSplit contiguous slices: grid = (kNormSplit, ntensors)
constexpr int kNormSplit = 32;
__global__ __launch_bounds__(kBlock) void adam_norm_kernel(const float* __restrict__ p,
                                                           const float* __restrict__ g,
                                                           const long long* __restrict__ offs,
                                                           const float* __restrict__ l2,
                                                           double* __restrict__ partial) {
    __shared__ double red[4];
    const int t = blockIdx.y;
    const long long b = offs[t], e = offs[t + 1];
    const long long per = (e - b + kNormSplit - 1) / kNormSplit;
    const long long s0 = b + per * blockIdx.x, s1 = s0 + per < e ? s0 + per : e;
    const float l2c = 2.f * l2[t];
    double acc[1] = {0.0};
#pragma unroll 4
    for (long long i = s0 + threadIdx.x; i < s1; i += kBlock) {
        const float gv = fmaf(l2c, p[i], g[i]);
        acc[0] += (double)gv * gv;
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) partial[(size_t)t * kNormSplit + blockIdx.x] = acc[0];
}

struct AdamArgs {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema;  // may be null
    const long long* offs;
    const float* l2;
    const double* norm_partial;
    float* norms;
    float lr, beta1, beta2, eps, wd, clipnorm, alpha, ema_decay;
    int ema_copy;
};

__global__ __launch_bounds__(kBlock) void adam_step_kernel(AdamArgs a) {
    const int t = blockIdx.y;
    const long long b = a.offs[t], e = a.offs[t + 1];
    const float l2c = 2.f * a.l2[t];
    // keras clip_by_norm: g * clip / max(norm, clip)
    double sq = 0.0;
    for (int k = 0; k < kNormSplit; ++k) sq += a.norm_partial[(size_t)t * kNormSplit + k];
    const float norm = (float)sqrt(sq);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.norms[t] = norm;
    const float cf = a.clipnorm > 0.f ? a.clipnorm / fmaxf(norm, a.clipnorm) : 1.f;
    for (long long i = b + (long long)blockIdx.x * kBlock + threadIdx.x; i < e;
         i += (long long)gridDim.x * kBlock) {
        float w = a.p[i];
        const float gv = fmaf(l2c, w, a.g[i]) * cf;
        w -= w * a.wd * a.lr;  // decoupled decay first (keras _apply_weight_decay)
        float m = a.m[i], v = a.v[i];
        m += (gv - m) * (1.f - a.beta1);
        v += (gv * gv - v) * (1.f - a.beta2);
        w -= m * a.alpha / (sqrtf(v) + a.eps);
        a.p[i] = w;
        a.m[i] = m;
        a.v[i] = v;
        if (a.ema != nullptr) a.ema[i] = a.ema_copy ? w : a.ema_decay * a.ema[i] + (1.f - a.ema_decay) * w;
    }
}

__global__ __launch_bounds__(kBlock) void ema_kernel(float* __restrict__ ema,
                                                     const float* __restrict__ w, size_t count,
                                                     float decay, int copy) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < count;
         i += (size_t)gridDim.x * kBlock)
        ema[i] = copy ? w[i] : decay * ema[i] + (1.f - decay) * w[i];
}

__global__ __launch_bounds__(kBlock) void cast_f32_bf16_kernel(const float* __restrict__ in,
                                                               uint16_t* __restrict__ out, size_t count) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (size_t)gridDim.x * kBlock)
        out[i] = lf::bf16_down(in[i]);
}

__global__ __launch_bounds__(kBlock) void cast_bf16_f32_kernel(const uint16_t* __restrict__ in,
                                                               float* __restrict__ out, size_t count) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (size_t)gridDim.x * kBlock)
        out[i] = lf::bf16_up(in[i]);
}

inline unsigned plane_grid(int hw_items) { return lf::stream_grid((size_t)hw_items, kBlock, 64); }
inline bool aligned(const void* p, size_t bytes) { return (reinterpret_cast<size_t>(p) & (bytes - 1)) == 0; }

// temperature > 0 and finite, 0 <= alpha <= 1 (NaN fails every comparison)
inline bool distill_args_ok(float temperature, float alpha) {
    return temperature > 0.f && temperature <= FLT_MAX && alpha >= 0.f && alpha <= 1.f;
}

// gamma == 0, or 1 <= gamma <= 8 (NaN fails every comparison).  x -> x^gamma is not Lipschitz at 0 for gamma < 1
// and 1 - p has no relative accuracy left as p -> 1, so (0, 1) has no rounding bound to offer.
inline bool focal_gamma_ok(float gamma) { return gamma == 0.f || (gamma >= 1.f && gamma <= 8.f); }

// What every head's backward ends with: dW[f][c] = sum_n feat[n][f] dlogits[n][c]; db[c] = sum_n dlogits[n][c]
int head_weight_grads(const char* what, const float* feat, const float* dlogits, float* dw, float* db, int n, int f,
                      int c, hipStream_t st) {
    outer_sum_kernel<<<(unsigned)(((size_t)(f + 1) * c + 63) / 64), kBlock, 0, st>>>(feat, dlogits, dw, db,
                                                                                   n, f, c);
    return lf::check_launch(what);
}

// The backward pass of both heads: dlogits and dfeat per sample, then (dW, db) over the batch.
template <bool kDistill>
int head_bwd_launch(const char* what, const float* feat, const float* w, const float* probs, const float* ytrue,
                    const float* soft, float hard_w, float soft_w, float* dlogits, float* dfeat, float* dw,
                    float* db, int n, int f, int c, float inv_n, lf_stream_t stream) {
    hipStream_t st = lf::as_stream(stream);
    head_bwd_kernel<kDistill><<<n, 64, (size_t)c * sizeof(float), st>>>(probs, ytrue, soft, hard_w, soft_w, w,
                                                                       dlogits, dfeat, f, c, inv_n);
    return head_weight_grads(what, feat, dlogits, dw, db, n, f, c, st);
}

// lf_input_stage_f32 (mix8 == nullptr) and lf_input_stage_mix_f32: the contrast means, then the stage's kernel
int input_stage_launch(const char* who, const uint8_t* in, float* out, int n, int h, int w, const float* aug4,
                       const float* mix8, const float* mean3, const float* denom3, float* means_ws,
                       lf_stream_t stream) {
    LF_REQUIRE(in && out && aug4 && means_ws, "%s: null buffer", who);
    LF_REQUIRE(n > 0 && h > 1 && w > 1, "%s: bad dims n=%d h=%d w=%d", who, n, h, w);
    LF_REQUIRE((mean3 == nullptr) == (denom3 == nullptr), "%s: mean/denom must both be set", who);
    LF_REQUIRE(n <= 65535, "%s: batch too large", who);
    float m[3], d[3];
    lf::norm_consts(mean3, denom3, m, d);
    hipStream_t s = lf::as_stream(stream);
    const dim3 grid(plane_grid(h * w), n);
    aug_means_kernel<<<dim3(kMeanSplit, n), kBlock, 0, s>>>(in, aug4, means_ws, h, w);
    if (mix8 == nullptr)
        input_aug_kernel<<<grid, kBlock, 0, s>>>(in, out, aug4, means_ws, h, w, m[0], m[1], m[2], d[0], d[1], d[2]);
    else
        input_mix_kernel<<<grid, kBlock, 0, s>>>(in, out, aug4, mix8, means_ws, n, h, w, m[0], m[1], m[2], d[0], d[1],
                                                 d[2]);
    return lf::check_launch(who);
}

// LF_OK when a BN entry's workspace holds the kBnSplit partial pairs of its c channels
int bn_workspace_ok(const char* who, size_t ws_bytes, int c) {
    if (ws_bytes >= lf_bn_workspace(c)) return LF_OK;
    lf::set_error("%s: workspace %zu < %zu", who, ws_bytes, lf_bn_workspace(c));
    return LF_ERR_WORKSPACE;
}

// what the plane-sum route of BatchNorm's backward (plane_g, plane_m) asks of its arguments
int bn_plane_rules(const char* who, const float* plane_g, const float* plane_m, const float* alpha_nc,
                   const float* add_nc, int relu) {
    LF_REQUIRE(plane_g != nullptr || plane_m == nullptr, "%s: plane_m needs plane_g", who);
    LF_REQUIRE(plane_g == nullptr || relu != 0 || (alpha_nc == nullptr && add_nc == nullptr),
               "%s: plane sums without a mask take no alpha / add", who);
    LF_REQUIRE(plane_g == nullptr || add_nc == nullptr || plane_m != nullptr,
               "%s: add_nc with plane sums needs plane_m", who);
    return LF_OK;
}

// the g / y route to BatchNorm's backward sums: kBnSplit slices per channel, then the finalizer
void bn_bwd_sums_launch(const BnBwdArgs& a, float* part, const BnBwdOut& o, hipStream_t s) {
    auto reduce = a.hw % 4 == 0 ? bn_bwd_reduce_kernel<4> : bn_bwd_reduce_kernel<1>;
    reduce<<<dim3(kBnSplit, a.c), kBlock, 0, s>>>(a, part);
    bn_bwd_finalize_kernel<<<(a.c + 63) / 64, 64, 0, s>>>(part, a.c, 0, o);
}

// The rules both storage types of the residual tail share; the bf16 entries add their shape and alignment rules.
template <typename T, int V, bool Keep = false>
int tail_fwd_launch(const char* who, const TailArgs<T>& t, uint8_t* route, T* p, int n, lf_stream_t stream,
                    T* y_at, T* sc_at) {
    LF_REQUIRE(t.y && t.sc && p, "%s: null buffer", who);
    LF_REQUIRE((t.sc_scale == nullptr) == (t.sc_shift == nullptr), "%s: sc_scale/sc_shift", who);
    LF_REQUIRE((t.a_scale == nullptr) == (t.a_shift == nullptr), "%s: a_scale/a_shift", who);
    tail_fwd_kernel<T, V, Keep><<<dim3(n * t.c, plane_grid((t.h / 2) * (t.w / V))), kBlock, 0,
                                  lf::as_stream(stream)>>>(t, route, p, y_at, sc_at);
    return lf::check_launch(who);
}

// Kept: y_at / sc_at stand in for y / sc_y (tail_bwd_kernel), so either of a pair satisfies the rules.
template <typename T, int V, bool Kept = false>
int tail_bwd_launch(const char* who, const T* dp, const uint8_t* route, const T* y, const float* a_scale,
                    const float* a_shift, const float* drop, T* dr, float* ds, float* plane_sums, const T* sc_y,
                    float* sc_sums, int n, int c, int h, int w, lf_stream_t stream, const T* y_at,
                    const T* sc_at) {
    const bool has_y = y != nullptr || y_at != nullptr, has_sc = sc_y != nullptr || sc_at != nullptr;
    LF_REQUIRE(has_sc == (sc_sums != nullptr), "%s: sc_y and sc_sums go together", who);
    LF_REQUIRE(dp && route && dr, "%s: null buffer", who);
    LF_REQUIRE(plane_sums == nullptr || (has_y && a_scale != nullptr),
               "%s: plane_sums needs y and a_scale/a_shift", who);
    LF_REQUIRE(has_y == (ds != nullptr || plane_sums != nullptr), "%s: y goes with ds / plane_sums", who);
    LF_REQUIRE((a_scale == nullptr) == (a_shift == nullptr), "%s: a_scale/a_shift", who);
    tail_bwd_kernel<T, V, Kept><<<n * c, kBlock, 0, lf::as_stream(stream)>>>(
        dp, route, y, a_scale, a_shift, drop, dr, ds, plane_sums, sc_y, sc_sums, c, h, w, y_at, sc_at);
    return lf::check_launch(who);
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int lf_input_stage_f32(const uint8_t* in, float* out, int n, int h, int w, const float* aug4,
                       const float* mean3, const float* denom3, float* means_ws,
                       lf_stream_t stream) {
    return input_stage_launch("lf_input_stage", in, out, n, h, w, aug4, nullptr, mean3, denom3, means_ws, stream);
}

int lf_input_stage_mix_f32(const uint8_t* in, float* out, int n, int h, int w, const float* aug4,
                           const float* mix8, const float* mean3, const float* denom3, float* means_ws,
                           lf_stream_t stream) {
    LF_REQUIRE(mix8, "lf_input_stage_mix: null buffer");
    return input_stage_launch("lf_input_stage_mix", in, out, n, h, w, aug4, mix8, mean3, denom3, means_ws, stream);
}

int lf_mix_targets_f32(const float* y, const float* mix8, float* out, int n, int c, lf_stream_t stream) {
    LF_REQUIRE(y && mix8 && out, "lf_mix_targets: null buffer");
    LF_REQUIRE(n > 0 && n <= 65535 && c > 0 && c <= kHeadMaxClasses, "lf_mix_targets: bad dims n=%d c=%d", n, c);
    LF_REQUIRE(out + (size_t)n * c <= y || y + (size_t)n * c <= out, "lf_mix_targets: out overlaps y");
    mix_targets_kernel<<<(unsigned)(((size_t)n * c + kBlock - 1) / kBlock), kBlock, 0, lf::as_stream(stream)>>>(
        y, mix8, out, n, c);
    return lf::check_launch("lf_mix_targets");
}

int lf_scale_shift_act_f32(const float* x, float* out, int n, int c, int hw, const float* scale,
                           const float* shift, int relu, lf_stream_t stream) {
    LF_REQUIRE(x && out && scale && shift, "lf_scale_shift_act: null buffer");
    LF_REQUIRE(n > 0 && c > 0 && hw > 0 && (long long)n * c < (1LL << 31),
               "lf_scale_shift_act: bad dims n=%d c=%d hw=%d", n, c, hw);
    hipStream_t s = lf::as_stream(stream);
    const int planes = n * c;
    if ((hw & 3) == 0)
        scale_shift_act_kernel<4><<<dim3(planes, plane_grid(hw / 4)), kBlock, 0, s>>>(x, out, c, hw / 4,
                                                                                 scale, shift, relu);
    else
        scale_shift_act_kernel<1><<<dim3(planes, plane_grid(hw)), kBlock, 0, s>>>(x, out, c, hw, scale,
                                                                             shift, relu);
    return lf::check_launch("lf_scale_shift_act");
}

size_t lf_bn_workspace(int c) { return c > 0 ? (size_t)c * kBnSplit * 2 * sizeof(float) : 0; }

int lf_bn_train_stats_f32(const float* y, int n, int c, int hw, const float* gamma,
                          const float* beta, float* moving_mean, float* moving_var, float momentum,
                          float eps, float* mean, float* invstd, float* scale, float* shift,
                          void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(y && gamma && beta && moving_mean && moving_var && mean && invstd && scale && shift &&
                   workspace,
               "lf_bn_train_stats: null buffer");
    LF_REQUIRE(n > 0 && c > 0 && hw > 0 && c <= 65535, "lf_bn_train_stats: bad dims n=%d c=%d hw=%d", n, c, hw);
    if (int err = bn_workspace_ok("lf_bn_train_stats", ws_bytes, c)) return err;
    hipStream_t s = lf::as_stream(stream);
    float* part = static_cast<float*>(workspace);
    auto stats = hw % 4 == 0 ? bn_stats_kernel<4> : bn_stats_kernel<1>;
    stats<<<dim3(kBnSplit, c), kBlock, 0, s>>>(y, n, c, hw, part);
    bn_finalize_kernel<<<(c + 63) / 64, 64, 0, s>>>(y, hw, part, c, (double)n * hw, gamma, beta,
                                                   moving_mean, moving_var, momentum, eps, mean,
                                                   invstd, scale, shift);
    return lf::check_launch("lf_bn_train_stats");
}

int lf_bn_train_stats_tiles_f32(const float* tile_part, long long tiles, int n, int c, int hw,
                                const float* gamma, const float* beta, float* moving_mean,
                                float* moving_var, float momentum, float eps, float* mean,
                                float* invstd, float* scale, float* shift, void* workspace,
                                size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(tile_part && gamma && beta && moving_mean && moving_var && mean && invstd && scale &&
                   shift && workspace,
               "lf_bn_train_stats_tiles: null buffer");
    LF_REQUIRE(n > 0 && c > 0 && hw > 0 && c <= 65535 && tiles > 0,
               "lf_bn_train_stats_tiles: bad dims n=%d c=%d hw=%d tiles=%lld", n, c, hw, tiles);
    if (int err = bn_workspace_ok("lf_bn_train_stats_tiles", ws_bytes, c)) return err;
    hipStream_t s = lf::as_stream(stream);
    float* part = static_cast<float*>(workspace);
    bn_tile_reduce_kernel<<<dim3(kBnSplit, c), kBlock, 0, s>>>(tile_part, tiles, part);
    // the tile sums were taken about moving_mean as it still is here (updated by this kernel)
    bn_finalize_kernel<<<(c + 63) / 64, 64, 0, s>>>(moving_mean, 1, part, c, (double)n * hw, gamma,
                                                   beta, moving_mean, moving_var, momentum, eps,
                                                   mean, invstd, scale, shift);
    return lf::check_launch("lf_bn_train_stats_tiles");
}

int lf_bn_infer_scale_shift_f32(int c, const float* gamma, const float* beta,
                                const float* moving_mean, const float* moving_var, float eps,
                                float* scale, float* shift, lf_stream_t stream) {
    LF_REQUIRE(gamma && beta && moving_mean && moving_var && scale && shift, "lf_bn_infer: null buffer");
    LF_REQUIRE(c > 0, "lf_bn_infer: bad c=%d", c);
    bn_infer_kernel<<<(c + 63) / 64, 64, 0, lf::as_stream(stream)>>>(c, gamma, beta, moving_mean,
                                                                   moving_var, eps, scale, shift);
    return lf::check_launch("lf_bn_infer");
}

int lf_bn_bwd_f32(const float* g, const float* alpha_nc, const float* add_nc, const float* y,
                  const float* mean, const float* invstd, const float* scale, const float* shift,
                  int relu, const float* gamma, float* dy, float* dgamma, float* dbeta,
                  const float* plane_g, const float* plane_m, int have_sums, int n, int c, int hw,
                  void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(g && y && mean && invstd && scale && shift && gamma && dy && dgamma && dbeta && workspace,
               "lf_bn_bwd: null buffer");
    LF_REQUIRE(!have_sums || plane_g == nullptr, "lf_bn_bwd: have_sums excludes plane sums");
    if (int err = bn_plane_rules("lf_bn_bwd", plane_g, plane_m, alpha_nc, add_nc, relu)) return err;
    LF_REQUIRE(n > 0 && c > 0 && hw > 0 && c <= 65535 && (long long)n * c < (1LL << 31),
               "lf_bn_bwd: bad dims n=%d c=%d hw=%d", n, c, hw);
    if (int err = bn_workspace_ok("lf_bn_bwd", ws_bytes, c)) return err;
    const BnBwdArgs a{g, alpha_nc, add_nc, y, mean, invstd, scale, shift, relu, n, c, hw};
    const BnBwdOut o{mean, invstd, scale, shift, gamma, 0.f, dgamma, dbeta, nullptr};
    hipStream_t s = lf::as_stream(stream);
    const int v = hw % 4 == 0 ? 4 : 1;
    if (have_sums) {
        // dgamma / dbeta already hold the two channel sums (lf_bn_bwd_sums*_f32)
    } else if (plane_g != nullptr) {
        bn_bwd_planes_kernel<<<c, kBlock, 0, s>>>(plane_g, plane_m, alpha_nc, add_nc, n, c, o);
    } else {
        bn_bwd_sums_launch(a, static_cast<float*>(workspace), o, s);
    }
    auto apply = v == 4 ? bn_bwd_apply_kernel<4> : bn_bwd_apply_kernel<1>;
    apply<<<dim3(n * c, plane_grid(hw / v)), kBlock, 0, s>>>(a, gamma, dgamma, dbeta, 1.0f / ((float)n * (float)hw),
                                                            dy);
    return lf::check_launch("lf_bn_bwd");
}

int lf_bn_bwd_sums_f32(const float* g, const float* alpha_nc, const float* add_nc, const float* y,
                       const float* mean, const float* invstd, const float* scale,
                       const float* shift, int relu, const float* gamma, float* dgamma, float* dbeta,
                       float* coef, const float* plane_g, const float* plane_m, int n, int c, int hw,
                       void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(mean && invstd && scale && shift && gamma && dgamma && dbeta && coef && workspace,
               "lf_bn_bwd_sums: null buffer");
    LF_REQUIRE(plane_g != nullptr || (g != nullptr && y != nullptr), "lf_bn_bwd_sums: g / y missing");
    LF_REQUIRE(n > 0 && c > 0 && hw > 0 && c <= 65535 && (long long)n * c < (1LL << 31),
               "lf_bn_bwd_sums: bad dims n=%d c=%d hw=%d", n, c, hw);
    if (int err = bn_plane_rules("lf_bn_bwd_sums", plane_g, plane_m, alpha_nc, add_nc, relu)) return err;
    if (int err = bn_workspace_ok("lf_bn_bwd_sums", ws_bytes, c)) return err;
    hipStream_t s = lf::as_stream(stream);
    // every route forms the coefficients where it forms the sums
    const BnBwdOut o{mean, invstd, scale, shift, gamma, 1.0f / ((float)n * (float)hw), dgamma, dbeta, coef};
    if (plane_g != nullptr) {
        bn_bwd_planes_kernel<<<c, kBlock, 0, s>>>(plane_g, plane_m, alpha_nc, add_nc, n, c, o);
    } else {
        const BnBwdArgs a{g, alpha_nc, add_nc, y, mean, invstd, scale, shift, relu, n, c, hw};
        bn_bwd_sums_launch(a, static_cast<float*>(workspace), o, s);
    }
    return lf::check_launch("lf_bn_bwd_sums");
}

int lf_bn_bwd_sums_tiles_f32(const float* tile_part, long long tiles, const float* mean,
                             const float* invstd, const float* scale, const float* shift,
                             const float* gamma, float* dgamma, float* dbeta, float* coef, int n,
                             int c, int hw, void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(tile_part && mean && invstd && scale && shift && gamma && dgamma && dbeta && coef &&
                   workspace,
               "lf_bn_bwd_sums_tiles: null buffer");
    LF_REQUIRE(n > 0 && c > 0 && hw > 0 && c <= 65535 && tiles > 0,
               "lf_bn_bwd_sums_tiles: bad dims n=%d c=%d hw=%d tiles=%lld", n, c, hw, tiles);
    if (int err = bn_workspace_ok("lf_bn_bwd_sums_tiles", ws_bytes, c)) return err;
    hipStream_t s = lf::as_stream(stream);
    float* part = static_cast<float*>(workspace);
    const BnBwdOut o{mean, invstd, scale, shift, gamma, 1.0f / ((float)n * (float)hw), dgamma, dbeta, coef};
    bn_tile_reduce_kernel<<<dim3(kBnSplit, c), kBlock, 0, s>>>(tile_part, tiles, part);
    bn_bwd_finalize_kernel<<<(c + 63) / 64, 64, 0, s>>>(part, c, 1, o);
    return lf::check_launch("lf_bn_bwd_sums_tiles");
}

int lf_gap_f32(const float* x, float* out, int planes, int hw, int c, const float* scale,
               const float* shift, int relu, float* mask_sums, lf_stream_t stream) {
    LF_REQUIRE(x && out, "lf_gap: null buffer");
    LF_REQUIRE(mask_sums == nullptr || scale != nullptr, "lf_gap: mask_sums needs scale/shift");
    LF_REQUIRE(planes > 0 && hw > 0 && c > 0, "lf_gap: bad dims planes=%d hw=%d c=%d", planes, hw, c);
    LF_REQUIRE((scale == nullptr) == (shift == nullptr), "lf_gap: scale/shift must both be set");
    auto kernel = hw % 4 == 0 ? gap_kernel<float, 4> : gap_kernel<float, 1>;
    kernel<<<planes, kBlock, 0, lf::as_stream(stream)>>>(x, out, hw, c, scale, shift, relu, mask_sums);
    return lf::check_launch("lf_gap");
}

int lf_gap_stats_bf16(const uint16_t* x, float* out, float* mask_sums, int n, int c, int hw, const float* scale,
                      const float* shift, int relu, lf_stream_t stream) {
    LF_REQUIRE(x && out, "lf_gap_stats_bf16: null buffer");
    LF_REQUIRE(n > 0 && c > 0 && hw > 0 && hw % 4 == 0, "lf_gap_stats_bf16: bad dims n=%d c=%d hw=%d (hw %% 4 == 0)",
               n, c, hw);
    LF_REQUIRE((scale == nullptr) == (shift == nullptr), "lf_gap_stats_bf16: scale/shift must both be set");
    LF_REQUIRE(mask_sums == nullptr || scale != nullptr, "lf_gap_stats_bf16: mask_sums needs scale/shift");
    LF_REQUIRE(aligned(x, 8), "lf_gap_stats_bf16: x must be 8-byte aligned");
    auto kernel = hw % 8 == 0 && aligned(x, 16) ? gap_kernel<uint16_t, 8> : gap_kernel<uint16_t, 4>;
    kernel<<<n * c, kBlock, 0, lf::as_stream(stream)>>>(x, out, hw, c, scale, shift, relu, mask_sums);
    return lf::check_launch("lf_gap_stats_bf16");
}

int lf_bcast_planes_f32(const float* v, float* out, int planes, int hw, float scale,
                        lf_stream_t stream) {
    LF_REQUIRE(v && out, "lf_bcast_planes: null buffer");
    LF_REQUIRE(planes > 0 && hw > 0, "lf_bcast_planes: bad dims planes=%d hw=%d", planes, hw);
    bcast_planes_kernel<float, 1><<<dim3(planes, plane_grid(hw)), kBlock, 0, lf::as_stream(stream)>>>(v, out, hw,
                                                                                                     scale);
    return lf::check_launch("lf_bcast_planes");
}

int lf_bcast_planes_bf16(const float* v, uint16_t* out, int planes, int hw, float scale, lf_stream_t stream) {
    LF_REQUIRE(v && out, "lf_bcast_planes_bf16: null buffer");
    LF_REQUIRE(planes > 0 && hw > 0 && hw % 4 == 0, "lf_bcast_planes_bf16: bad dims planes=%d hw=%d (hw %% 4 == 0)",
               planes, hw);
    LF_REQUIRE(aligned(out, 8), "lf_bcast_planes_bf16: out must be 8-byte aligned");
    bcast_planes_kernel<uint16_t, 4><<<dim3(planes, plane_grid(hw / 4)), kBlock, 0, lf::as_stream(stream)>>>(
        v, out, hw, scale);
    return lf::check_launch("lf_bcast_planes_bf16");
}

int lf_se_fwd_f32(const float* m, const float* w1, const float* b1, const float* w2,
                  const float* b2, float* z1, float* s, int n, int c, int cr, lf_stream_t stream) {
    LF_REQUIRE(m && w1 && b1 && w2 && b2 && z1 && s, "lf_se_fwd: null buffer");
    LF_REQUIRE(n > 0 && c > 0 && cr > 0 && c + cr <= 8192, "lf_se_fwd: bad dims n=%d c=%d cr=%d", n, c, cr);
    se_fwd_kernel<<<n, kBlock, (size_t)(c + cr) * sizeof(float), lf::as_stream(stream)>>>(
        m, w1, b1, w2, b2, z1, s, c, cr);
    return lf::check_launch("lf_se_fwd");
}

size_t lf_se_bwd_workspace(int n, int c, int cr) {
    return (n > 0 && c > 0 && cr > 0) ? (size_t)n * (c + cr) * sizeof(float) : 0;
}

int lf_se_bwd_f32(const float* ds, const float* m, const float* z1, const float* s,
                  const float* w1, const float* w2, float* dm, float* dw1, float* db1, float* dw2,
                  float* db2, int n, int c, int cr, float dm_scale, void* workspace,
                  size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(ds && m && z1 && s && w1 && w2 && dm && dw1 && db1 && dw2 && db2 && workspace,
               "lf_se_bwd: null buffer");
    LF_REQUIRE(n > 0 && c > 0 && cr > 0 && c + cr <= 8192, "lf_se_bwd: bad dims n=%d c=%d cr=%d", n, c, cr);
    if (ws_bytes < lf_se_bwd_workspace(n, c, cr)) {
        lf::set_error("lf_se_bwd: workspace too small");
        return LF_ERR_WORKSPACE;
    }
    hipStream_t st = lf::as_stream(stream);
    float* dpre2 = static_cast<float*>(workspace);
    float* dpre1 = dpre2 + (size_t)n * c;
    se_bwd_sample_kernel<<<n, kBlock, (size_t)(c + cr) * sizeof(float), st>>>(ds, s, z1, w1, w2, dpre2,
                                                                              dpre1, dm, c, cr, dm_scale);
    // dw1[c][cr] = sum_n m[n][c] dpre1[n][cr]; dw2[cr][c] = sum_n z1[n][cr] dpre2[n][c]
    outer_sum_kernel<<<(unsigned)(((size_t)(c + 1) * cr + 63) / 64), kBlock, 0, st>>>(m, dpre1, dw1, db1,
                                                                                    n, c, cr);
    outer_sum_kernel<<<(unsigned)(((size_t)(cr + 1) * c + 63) / 64), kBlock, 0, st>>>(z1, dpre2, dw2,
                                                                                    db2, n, cr, c);
    return lf::check_launch("lf_se_bwd");
}

int lf_block_tail_fwd_f32(const float* y, const float* a_scale, const float* a_shift,
                          const float* s, const float* sc, const float* sc_scale,
                          const float* sc_shift, int sc_relu, const float* drop, uint8_t* route,
                          float* p, int n, int c, int h, int w, lf_stream_t stream) {
    LF_REQUIRE(route, "lf_block_tail_fwd: null buffer");
    LF_REQUIRE(n > 0 && c > 0 && h > 1 && w > 1 && (long long)n * c < (1LL << 31),
               "lf_block_tail_fwd: bad dims n=%d c=%d h=%d w=%d", n, c, h, w);
    LF_REQUIRE((w & 1) == 0, "lf_block_tail_fwd: width must be even");
    const TailArgs<float> t{y, a_scale, a_shift, s, sc, sc_scale, sc_shift, drop, sc_relu, c, h, w};
    auto launch = w % 4 == 0 ? tail_fwd_launch<float, 4> : tail_fwd_launch<float, 2>;
    return launch("lf_block_tail_fwd", t, route, p, n, stream, nullptr, nullptr);
}

int lf_block_tail_fwd_keep_f32(const float* y, const float* a_scale, const float* a_shift, const float* s,
                               const float* sc, const float* sc_scale, const float* sc_shift, int sc_relu,
                               const float* drop, uint8_t* route, float* p, float* y_at, float* sc_at, int n, int c,
                               int h, int w, lf_stream_t stream) {
    LF_REQUIRE(route, "lf_block_tail_fwd_keep: null buffer");
    LF_REQUIRE(n > 0 && c > 0 && h > 1 && w > 1 && (long long)n * c < (1LL << 31),
               "lf_block_tail_fwd_keep: bad dims n=%d c=%d h=%d w=%d", n, c, h, w);
    LF_REQUIRE((w & 1) == 0, "lf_block_tail_fwd_keep: width must be even");
    const TailArgs<float> t{y, a_scale, a_shift, s, sc, sc_scale, sc_shift, drop, sc_relu, c, h, w};
    auto launch = w % 4 == 0 ? tail_fwd_launch<float, 4, true> : tail_fwd_launch<float, 2, true>;
    return launch("lf_block_tail_fwd_keep", t, route, p, n, stream, y_at, sc_at);
}

int lf_block_tail_fwd_train_bf16(const uint16_t* y, const float* a_scale, const float* a_shift, const float* s,
                                 const uint16_t* sc, const float* sc_scale, const float* sc_shift, int sc_relu,
                                 const float* drop, uint8_t* route, uint16_t* pooled, int n, int c, int h, int w,
                                 lf_stream_t stream) {
    LF_REQUIRE(n > 0 && c > 0 && h > 1 && w > 3 && h % 2 == 0 && w % 4 == 0 && (long long)n * c < (1LL << 31),
               "lf_block_tail_fwd_train_bf16: bad dims n=%d c=%d h=%d w=%d (h even, w %% 4 == 0)", n, c, h, w);
    LF_REQUIRE(aligned(y, 8) && aligned(sc, 8) && aligned(pooled, 4) && aligned(route, 2),
               "lf_block_tail_fwd_train_bf16: misaligned buffer");
    const TailArgs<uint16_t> t{y, a_scale, a_shift, s, sc, sc_scale, sc_shift, drop, sc_relu, c, h, w};
    const bool v8 = w % 8 == 0 && aligned(y, 16) && aligned(sc, 16) && aligned(pooled, 8) && aligned(route, 4);
    auto launch = v8 ? tail_fwd_launch<uint16_t, 8> : tail_fwd_launch<uint16_t, 4>;
    return launch("lf_block_tail_fwd_train_bf16", t, route, pooled, n, stream, nullptr, nullptr);
}

int lf_block_tail_bwd_f32(const float* dp, const uint8_t* route, const float* y,
                          const float* a_scale, const float* a_shift, const float* drop, float* dr,
                          float* ds, float* plane_sums, const float* sc_y, float* sc_sums, int n,
                          int c, int h, int w, lf_stream_t stream) {
    LF_REQUIRE(n > 0 && c > 0 && h > 1 && w > 1, "lf_block_tail_bwd: bad dims n=%d c=%d h=%d w=%d", n, c, h, w);
    LF_REQUIRE((w & 1) == 0, "lf_block_tail_bwd: width must be even (float2 rows)");
    auto launch = w % 4 == 0 ? tail_bwd_launch<float, 4> : tail_bwd_launch<float, 2>;
    return launch("lf_block_tail_bwd", dp, route, y, a_scale, a_shift, drop, dr, ds, plane_sums, sc_y, sc_sums, n, c, h,
                  w, stream, nullptr, nullptr);
}

int lf_block_tail_bwd_kept_f32(const float* dp, const uint8_t* route, const float* y, const float* y_at,
                               const float* a_scale, const float* a_shift, const float* drop, float* dr, float* ds,
                               float* plane_sums, const float* sc_y, const float* sc_at, float* sc_sums, int n, int c,
                               int h, int w, lf_stream_t stream) {
    LF_REQUIRE(n > 0 && c > 0 && h > 1 && w > 1, "lf_block_tail_bwd_kept: bad dims n=%d c=%d h=%d w=%d", n, c, h, w);
    LF_REQUIRE((w & 1) == 0, "lf_block_tail_bwd_kept: width must be even (float2 rows)");
    auto launch = w % 4 == 0 ? tail_bwd_launch<float, 4, true> : tail_bwd_launch<float, 2, true>;
    return launch("lf_block_tail_bwd_kept", dp, route, y, a_scale, a_shift, drop, dr, ds, plane_sums, sc_y, sc_sums, n,
                  c, h, w, stream, y_at, sc_at);
}

int lf_block_tail_bwd_bf16(const uint16_t* dp, const uint8_t* route, const uint16_t* y, const float* a_scale,
                           const float* a_shift, const float* drop, uint16_t* dr, float* ds, float* plane_sums,
                           const uint16_t* sc_y, float* sc_sums, int n, int c, int h, int w, lf_stream_t stream) {
    LF_REQUIRE(n > 0 && c > 0 && h > 1 && w > 3 && h % 2 == 0 && w % 4 == 0,
               "lf_block_tail_bwd_bf16: bad dims n=%d c=%d h=%d w=%d (h even, w %% 4 == 0)", n, c, h, w);
    LF_REQUIRE(aligned(dr, 8) && aligned(dp, 4) && aligned(route, 2), "lf_block_tail_bwd_bf16: misaligned buffer");
    auto launch = w % 8 == 0 && aligned(dr, 16) && aligned(dp, 8) && aligned(route, 4) ? tail_bwd_launch<uint16_t, 8>
                                                                                      : tail_bwd_launch<uint16_t, 4>;
    return launch("lf_block_tail_bwd_bf16", dp, route, y, a_scale, a_shift, drop, dr, ds, plane_sums, sc_y, sc_sums, n,
                  c, h, w, stream, nullptr, nullptr);
}

int lf_head_fwd_f32(const float* feat, const float* w, const float* b, const float* ytrue,
                    float* probs, float* loss, int n, int f, int c, lf_stream_t stream) {
    LF_REQUIRE(feat && w && b && probs, "lf_head_fwd: null buffer");
    LF_REQUIRE(n > 0 && f > 0 && c > 0 && c <= kHeadMaxClasses, "lf_head_fwd: bad dims n=%d f=%d c=%d", n, f, c);
    LF_REQUIRE((ytrue == nullptr) == (loss == nullptr), "lf_head_fwd: ytrue and loss go together");
    head_fwd_kernel<<<n, 64, (size_t)c * sizeof(float), lf::as_stream(stream)>>>(feat, w, b, ytrue, probs,
                                                                               loss, f, c);
    return lf::check_launch("lf_head_fwd");
}

int lf_head_bwd_f32(const float* feat, const float* w, const float* probs, const float* ytrue,
                    float* dlogits, float* dfeat, float* dw, float* db, int n, int f, int c,
                    float inv_n, lf_stream_t stream) {
    LF_REQUIRE(feat && w && probs && ytrue && dlogits && dfeat && dw && db, "lf_head_bwd: null buffer");
    LF_REQUIRE(n > 0 && f > 0 && c > 0 && c <= kHeadMaxClasses, "lf_head_bwd: bad dims n=%d f=%d c=%d", n, f, c);
    return head_bwd_launch<false>("lf_head_bwd", feat, w, probs, ytrue, nullptr, 0.f, 0.f, dlogits, dfeat, dw, db, n,
                                  f, c, inv_n, stream);
}

int lf_head_distill_fwd_f32(const float* feat, const float* w, const float* b, const float* ytrue,
                            const float* tprobs, float temperature, float alpha, float* probs, float* soft,
                            float* loss, float* kd, int n, int f, int c, lf_stream_t stream) {
    LF_REQUIRE(feat && w && b && ytrue && tprobs && probs && soft && loss, "lf_head_distill_fwd: null buffer");
    LF_REQUIRE(n > 0 && f > 0 && c > 0 && c <= kHeadMaxClasses, "lf_head_distill_fwd: bad dims n=%d f=%d c=%d", n, f,
               c);
    LF_REQUIRE(distill_args_ok(temperature, alpha), "lf_head_distill_fwd: bad temperature=%g (> 0, finite) or "
               "alpha=%g (0..1)", (double)temperature, (double)alpha);
    head_distill_fwd_kernel<<<n, 64, 2 * (size_t)c * sizeof(float), lf::as_stream(stream)>>>(
        feat, w, b, ytrue, tprobs, 1.f / temperature, temperature * temperature, alpha, probs, soft, loss, kd, f, c);
    return lf::check_launch("lf_head_distill_fwd");
}

int lf_head_distill_bwd_f32(const float* feat, const float* w, const float* probs, const float* ytrue,
                            const float* soft, float temperature, float alpha, float* dlogits, float* dfeat,
                            float* dw, float* db, int n, int f, int c, float inv_n, lf_stream_t stream) {
    LF_REQUIRE(feat && w && probs && ytrue && soft && dlogits && dfeat && dw && db,
               "lf_head_distill_bwd: null buffer");
    LF_REQUIRE(n > 0 && f > 0 && c > 0 && c <= kHeadMaxClasses, "lf_head_distill_bwd: bad dims n=%d f=%d c=%d", n, f,
               c);
    LF_REQUIRE(distill_args_ok(temperature, alpha), "lf_head_distill_bwd: bad temperature=%g (> 0, finite) or "
               "alpha=%g (0..1)", (double)temperature, (double)alpha);
    return head_bwd_launch<true>("lf_head_distill_bwd", feat, w, probs, ytrue, soft, 1.f - alpha,
                                 alpha * temperature, dlogits, dfeat, dw, db, n, f, c, inv_n, stream);
}

int lf_head_focal_fwd_f32(const float* feat, const float* w, const float* b, const float* ytrue, const float* cw,
                          float gamma, float* probs, float* loss, float* sw, int n, int f, int c,
                          lf_stream_t stream) {
    LF_REQUIRE(feat && w && b && ytrue && probs && loss, "lf_head_focal_fwd: null buffer");
    LF_REQUIRE(n > 0 && f > 0 && c > 0 && c <= kHeadMaxClasses, "lf_head_focal_fwd: bad dims n=%d f=%d c=%d", n, f,
               c);
    LF_REQUIRE(focal_gamma_ok(gamma), "lf_head_focal_fwd: bad gamma=%g (0, or 1..8)", (double)gamma);
    head_focal_fwd_kernel<<<n, 64, (size_t)c * sizeof(float), lf::as_stream(stream)>>>(feat, w, b, ytrue, cw, gamma,
                                                                                     probs, loss, sw, f, c);
    return lf::check_launch("lf_head_focal_fwd");
}

int lf_head_focal_bwd_f32(const float* feat, const float* w, const float* probs, const float* ytrue,
                          const float* cw, float gamma, float* dlogits, float* dfeat, float* dw, float* db, int n,
                          int f, int c, float inv_n, lf_stream_t stream) {
    LF_REQUIRE(feat && w && probs && ytrue && dlogits && dfeat && dw && db, "lf_head_focal_bwd: null buffer");
    LF_REQUIRE(n > 0 && f > 0 && c > 0 && c <= kHeadMaxClasses, "lf_head_focal_bwd: bad dims n=%d f=%d c=%d", n, f,
               c);
    LF_REQUIRE(focal_gamma_ok(gamma), "lf_head_focal_bwd: bad gamma=%g (0, or 1..8)", (double)gamma);
    hipStream_t st = lf::as_stream(stream);
    head_focal_bwd_kernel<<<n, 64, (size_t)c * sizeof(float), st>>>(probs, ytrue, cw, gamma, w, dlogits, dfeat, f, c,
                                                                  inv_n);
    return head_weight_grads("lf_head_focal_bwd", feat, dlogits, dw, db, n, f, c, st);
}

int lf_mul_f32(const float* a, const float* b, float* out, size_t count, lf_stream_t stream) {
    LF_REQUIRE(a && b && out, "lf_mul: null buffer");
    LF_REQUIRE(count > 0, "lf_mul: empty");
    mul_kernel<<<lf::stream_grid(count, kBlock), kBlock, 0, lf::as_stream(stream)>>>(a, b, out, count);
    return lf::check_launch("lf_mul");
}

size_t lf_adamw_workspace(int ntensors) {
    return ntensors > 0 ? (size_t)ntensors * kNormSplit * sizeof(double) : 0;
}

int lf_adamw_step_f32(float* param, const float* grad, float* m, float* v, float* ema,
                      const long long* offsets, const float* l2, int ntensors, long long max_count,
                      float lr, float beta1, float beta2, float eps, float weight_decay,
                      float clipnorm, long long step, float ema_decay, int ema_copy,
                      float* norms_out, void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(param && grad && m && v && offsets && l2 && norms_out && workspace,
               "lf_adamw_step: null buffer");
    if (ws_bytes < lf_adamw_workspace(ntensors)) {
        lf::set_error("lf_adamw_step: workspace %zu < %zu", ws_bytes, lf_adamw_workspace(ntensors));
        return LF_ERR_WORKSPACE;
    }
    LF_REQUIRE(ntensors > 0 && ntensors <= 65535 && max_count > 0 && step >= 1,
               "lf_adamw_step: bad ntensors=%d max_count=%lld step=%lld", ntensors, max_count, step);
    hipStream_t st = lf::as_stream(stream);
    double* partial = static_cast<double*>(workspace);
    adam_norm_kernel<<<dim3(kNormSplit, ntensors), kBlock, 0, st>>>(param, grad, offsets, l2, partial);
    AdamArgs a;
    a.p = param; a.g = grad; a.m = m; a.v = v; a.ema = ema; a.offs = offsets; a.l2 = l2;
    a.norm_partial = partial;
    a.norms = norms_out;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay;
    a.clipnorm = clipnorm;
    const double b1p = pow((double)beta1, (double)step), b2p = pow((double)beta2, (double)step);
    a.alpha = (float)((double)lr * sqrt(1.0 - b2p) / (1.0 - b1p));
    a.ema_decay = ema_decay;
    a.ema_copy = ema_copy;
    const unsigned gx = lf::stream_grid((size_t)max_count, kBlock, 64);
    adam_step_kernel<<<dim3(gx, ntensors), kBlock, 0, st>>>(a);
    return lf::check_launch("lf_adamw_step");
}

int lf_ema_update_f32(float* ema, const float* w, size_t count, float decay, int copy,
                      lf_stream_t stream) {
    LF_REQUIRE(ema && w, "lf_ema_update: null buffer");
    LF_REQUIRE(count > 0, "lf_ema_update: empty");
    ema_kernel<<<lf::stream_grid(count, kBlock), kBlock, 0, lf::as_stream(stream)>>>(ema, w, count, decay,
                                                                                 copy);
    return lf::check_launch("lf_ema_update");
}

int lf_cast_f32_bf16(const float* in, uint16_t* out, size_t count, lf_stream_t stream) {
    LF_REQUIRE(in && out && count > 0, "lf_cast_f32_bf16: null / empty buffer");
    cast_f32_bf16_kernel<<<lf::stream_grid(count, kBlock), kBlock, 0, lf::as_stream(stream)>>>(in, out, count);
    return lf::check_launch("lf_cast_f32_bf16");
}

int lf_cast_bf16_f32(const uint16_t* in, float* out, size_t count, lf_stream_t stream) {
    LF_REQUIRE(in && out && count > 0, "lf_cast_bf16_f32: null / empty buffer");
    cast_bf16_f32_kernel<<<lf::stream_grid(count, kBlock), kBlock, 0, lf::as_stream(stream)>>>(in, out, count);
    return lf::check_launch("lf_cast_bf16_f32");
}

}  // extern "C"
