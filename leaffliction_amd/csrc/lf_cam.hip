// libleafhip — class activation maps of leaf_cnn's head and their heat-map overlay.
//
// leaf_cnn ends in MaxPool -> GlobalAveragePooling2D -> Dense (srcs/model/cnn.py:96-101), so with F the last
// stage's pooled output [N][K][h][w] and W the dense kernel [K][C]
//     logit_c = b_c + mean_{y,x} cam_c(y,x),    cam_c(y,x) = sum_k W[k][c] * F[k][y][x]
// holds exactly (Zhou et al., "Learning Deep Features for Discriminative Localization", CVPR 2016).
//
// Both kernels are bandwidth kernels: cam_maps_kernel reads the features once whatever the number of class slots
// (K*M FMAs per loaded value are far under the ridge, so no MFMA), cam_overlay_kernel reads and writes the picture
// once with the few KB of map in LDS.  No atomics anywhere: the sums over k are folded in a fixed order and a
// maximum does not depend on its order, so two launches give the same bits.
#include "lf_common.h"
#include "lf_wave.h"

namespace {

using lf::Vec;
using lf::widen;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxSlots = 8;
constexpr int kMaxK = 512;          // the M weight columns [K][8] take at most 16 KB of LDS
constexpr int kOverlayIters = 4;    // pixel groups per thread: the map is staged once per 256 * 4 groups
constexpr int kOverlayLdsMap = 8192;  // maps of up to this many values (32 KB) are staged in LDS

// One workgroup per image.  A lane owns V consecutive pixels (one 16-byte load of fp32, one 8-byte load of bf16;
// V = 1: any h*w), the 64 lanes of a wave a tile of 64*V pixels, and the four waves split the channels into four
// consecutive slices: wave s sums its slice as one ascending fmaf chain per (slot, pixel), the four partial sums
// meet in LDS and are added as ((s0 + s1) + s2) + s3.  An image of more than 64*V pixels is walked in equal tiles.
// MP = the slot count rounded up to 1, 4 or 8: slots past m carry zero weights and are not stored.
// A class value outside [0, C) is clamped into it here, so that w is never read outside; the launcher refuses
// such values before the launch when it is given a host copy of `classes`.
// Dynamic LDS: part[kWaves][MP][64*V] floats, then the weight columns wl[K][MP].
template <typename T, int V, int MP>
__global__ __launch_bounds__(kBlock) void cam_maps_kernel(const T* __restrict__ feat, const float* __restrict__ w,
                                                          const int* __restrict__ classes, float* __restrict__ cam,
                                                          float* __restrict__ peak, int K, int hw, int C, int m) {
    constexpr int TP = 64 * V;                                        // pixels per tile
    constexpr int R = MP * TP / kBlock > 0 ? MP * TP / kBlock : 1;    // values a thread folds per tile
    extern __shared__ float lds[];
    float* part = lds;
    float* wl = lds + kWaves * MP * TP;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t n = blockIdx.x;

    for (int i = tid; i < K * MP; i += kBlock) {
        const int k = i / MP, j = i % MP;
        float v = 0.f;
        if (j < m) {
            const int c = min(max(classes[n * m + j], 0), C - 1);
            v = w[(size_t)k * C + c];
        }
        wl[i] = v;
    }
    __syncthreads();

    const int groups = hw / V;
    const int tiles = (groups + 63) / 64;
    const int per_tile = (groups + tiles - 1) / tiles;
    const int ks = (K + kWaves - 1) / kWaves;
    const int k0 = min(K, wv * ks), k1 = min(K, k0 + ks);
    const T* fn = feat + n * (size_t)K * hw;
    float pm[R];
#pragma unroll
    for (int r = 0; r < R; ++r) pm[r] = 0.f;

    for (int t = 0; t < tiles; ++t) {
        const int g0 = t * per_tile;
        const int gcount = min(per_tile, groups - g0);
        float acc[MP][V];
#pragma unroll
        for (int j = 0; j < MP; ++j)
#pragma unroll
            for (int e = 0; e < V; ++e) acc[j][e] = 0.f;
        if (lane < gcount) {
            const T* p = fn + (size_t)k0 * hw + (size_t)(g0 + lane) * V;
#pragma unroll 8
            for (int k = k0; k < k1; ++k, p += hw) {
                const Vec<T, V> f = *reinterpret_cast<const Vec<T, V>*>(p);
                const Vec<float, MP> wk = *reinterpret_cast<const Vec<float, MP>*>(wl + k * MP);
#pragma unroll
                for (int j = 0; j < MP; ++j)
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[j][e] = fmaf(wk[j], widen(f[e]), acc[j][e]);
            }
        }
#pragma unroll
        for (int j = 0; j < MP; ++j) {
            Vec<float, V> a;
#pragma unroll
            for (int e = 0; e < V; ++e) a[e] = acc[j][e];
            *reinterpret_cast<Vec<float, V>*>(part + (wv * MP + j) * TP + lane * V) = a;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + kBlock * r;
            const int j = i / TP, px = i % TP;
            if (i < MP * TP && j < m && px < gcount * V) {
                float s = part[j * TP + px];
#pragma unroll
                for (int sv = 1; sv < kWaves; ++sv) s += part[(sv * MP + j) * TP + px];
                cam[(n * m + j) * (size_t)hw + (size_t)g0 * V + px] = s;
                pm[r] = fmaxf(pm[r], s);
            }
        }
        __syncthreads();
    }

    // peak: thread tid folded slot (tid + kBlock * r) / TP in round r, the same slot in every lane of a wave
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float v = lf::wave_max_all(pm[r]);
        if (lane == 0) part[r * kWaves + wv] = v;
    }
    __syncthreads();
    if (tid < m) {
        float v;
        if constexpr (TP >= kBlock) {   // round r = slot r, in all four waves
            v = fmaxf(fmaxf(part[tid * kWaves], part[tid * kWaves + 1]),
                      fmaxf(part[tid * kWaves + 2], part[tid * kWaves + 3]));
        } else {                        // TP = 64: wave s folded slot s + 4 r in round r
            v = part[(tid / kWaves) * kWaves + tid % kWaves];
        }
        peak[n * m + tid] = v;
    }
}

// The colour ramp of the overlay (a "jet" ramp cut to its upper three quarters) and the blend of one byte.
__device__ __forceinline__ float ramp(float t4, float centre) {
    return fminf(fmaxf(1.5f - fabsf(t4 - centre), 0.f), 1.f);
}
// floor(u + 0.5) of u >= 0 is the conversion's truncation; u < 255.5 as a <= 1 up to rounding
__device__ __forceinline__ unsigned blend(float a255, float keep, float colour, unsigned byte) {
    return min((unsigned)(a255 * colour + keep * (float)byte + 0.5f), 255u);
}

// out = the picture with slot `slot`'s map laid over it: the map is upsampled bilinearly (pixel centres aligned,
// edges clamped), scaled by the slot's peak and blended in with weight alpha * t; t = 0 keeps the byte.  A thread
// finishes PX = 4 pixels of one row (three dwords) where W % 4 == 0, one pixel bytewise otherwise.  STAGE: the map
// is copied to LDS once per workgroup (a larger map is read through the caches).
template <bool VEC4, bool STAGE>
__global__ __launch_bounds__(kBlock) void cam_overlay_kernel(const uint8_t* __restrict__ img,
                                                             const float* __restrict__ cam,
                                                             const float* __restrict__ peak,
                                                             uint8_t* __restrict__ out, int H, int W, int h, int w,
                                                             int m, int slot, float alpha,
                                                             unsigned blocks_per_image) {
    constexpr int PX = VEC4 ? 4 : 1;
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const size_t n = blockIdx.x / blocks_per_image;
    const unsigned b = blockIdx.x % blocks_per_image;
    const float* src = cam + (n * m + slot) * (size_t)h * w;
    if (STAGE) {
        for (int i = tid; i < h * w; i += kBlock) lds[i] = src[i];
        __syncthreads();
    }
    auto at = [&](int i) -> float {
        if constexpr (STAGE)
            return lds[i];
        else
            return src[i];
    };
    const float pk = peak[n * m + slot];
    const float inv_pk = pk > 0.f ? 1.f / pk : 0.f;   // t = max(v, 0) / peak as one multiplication (within an ulp of t)
    const float rx = (float)w / (float)W, ry = (float)h / (float)H;
    const size_t pixels = (size_t)H * W, groups = pixels / PX;
    const uint8_t* in_n = img + n * pixels * 3;
    uint8_t* out_n = out + n * pixels * 3;

    for (int it = 0; it < kOverlayIters; ++it) {
        const size_t g = ((size_t)b * kOverlayIters + it) * kBlock + tid;
        if (g >= groups) break;
        const size_t p = g * PX;
        const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
        const float sy = fminf(fmaxf(((float)y + 0.5f) * ry - 0.5f, 0.f), (float)(h - 1));
        const int y0 = (int)sy, y1 = min(y0 + 1, h - 1);
        const float fy = sy - (float)y0;
        unsigned bytes[3 * PX];
        if constexpr (VEC4) {
            const unsigned* ip = reinterpret_cast<const unsigned*>(in_n + p * 3);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const unsigned word = ip[d];
#pragma unroll
                for (int q = 0; q < 4; ++q) bytes[d * 4 + q] = (word >> (8 * q)) & 0xffu;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q) bytes[q] = in_n[p * 3 + q];
        }
#pragma unroll
        for (int e = 0; e < PX; ++e) {
            const float sx = fminf(fmaxf(((float)(x + e) + 0.5f) * rx - 0.5f, 0.f), (float)(w - 1));
            const int x0 = (int)sx, x1 = min(x0 + 1, w - 1);
            const float fx = sx - (float)x0;
            const float top = at(y0 * w + x0) * (1.f - fx) + at(y0 * w + x1) * fx;
            const float bot = at(y1 * w + x0) * (1.f - fx) + at(y1 * w + x1) * fx;
            const float v = top * (1.f - fy) + bot * fy;
            const float t = fmaxf(v, 0.f) * inv_pk;
            const float a = alpha * t, t4 = 4.f * t, a255 = a * 255.f, keep = 1.f - a;
            bytes[e * 3 + 0] = blend(a255, keep, ramp(t4, 3.f), bytes[e * 3 + 0]);
            bytes[e * 3 + 1] = blend(a255, keep, ramp(t4, 2.f), bytes[e * 3 + 1]);
            bytes[e * 3 + 2] = blend(a255, keep, ramp(t4, 1.f), bytes[e * 3 + 2]);
        }
        if constexpr (VEC4) {
            unsigned* op = reinterpret_cast<unsigned*>(out_n + p * 3);
#pragma unroll
            for (int d = 0; d < 3; ++d)
                op[d] = bytes[d * 4] | (bytes[d * 4 + 1] << 8) | (bytes[d * 4 + 2] << 16) | (bytes[d * 4 + 3] << 24);
        } else {
#pragma unroll
            for (int q = 0; q < 3; ++q) out_n[p * 3 + q] = (uint8_t)bytes[q];
        }
    }
}

inline bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

template <typename T, int V>
int launch_cam_maps(const void* feat, const float* w, const int* classes, float* cam, float* peak, int n, int k,
                    int hw, int c, int m, hipStream_t s) {
    const int mp = m == 1 ? 1 : (m <= 4 ? 4 : 8);
    const size_t lds = ((size_t)kWaves * mp * 64 * V + (size_t)k * mp) * sizeof(float);
    const T* f = static_cast<const T*>(feat);
    if (mp == 1)
        cam_maps_kernel<T, V, 1><<<n, kBlock, lds, s>>>(f, w, classes, cam, peak, k, hw, c, m);
    else if (mp == 4)
        cam_maps_kernel<T, V, 4><<<n, kBlock, lds, s>>>(f, w, classes, cam, peak, k, hw, c, m);
    else
        cam_maps_kernel<T, V, 8><<<n, kBlock, lds, s>>>(f, w, classes, cam, peak, k, hw, c, m);
    return lf::check_launch("lf_cam_maps");
}

}  // namespace

extern "C" {

int lf_cam_maps(const void* feat, int feat_bf16, const float* w, const int32_t* classes,
                const int32_t* classes_host, float* cam, float* peak, int n, int k, int h, int wd, int c, int m,
                lf_stream_t stream) {
    LF_REQUIRE(feat && w && classes && cam && peak, "lf_cam_maps: null buffer");
    LF_REQUIRE(n > 0 && k > 0 && h > 0 && wd > 0 && c > 0, "lf_cam_maps: bad dims n=%d k=%d h=%d w=%d c=%d", n, k, h,
               wd, c);
    LF_REQUIRE(m >= 1 && m <= kMaxSlots, "lf_cam_maps: m=%d class slots (1..%d)", m, kMaxSlots);
    LF_REQUIRE(k <= kMaxK, "lf_cam_maps: k=%d channels (at most %d)", k, kMaxK);
    LF_REQUIRE((long long)h * wd <= (1 << 24), "lf_cam_maps: map of %d x %d is too large", h, wd);
    if (classes_host != nullptr)
        for (long long i = 0; i < (long long)n * m; ++i)
            LF_REQUIRE(classes_host[i] >= 0 && classes_host[i] < c,
                       "lf_cam_maps: class %d of image %lld, slot %lld is outside [0, %d)", classes_host[i], i / m,
                       i % m, c);
    const int hw = h * wd;
    hipStream_t s = lf::as_stream(stream);
    if (feat_bf16) {
        if (hw % 4 == 0 && aligned(feat, 8))
            return launch_cam_maps<uint16_t, 4>(feat, w, classes, cam, peak, n, k, hw, c, m, s);
        return launch_cam_maps<uint16_t, 1>(feat, w, classes, cam, peak, n, k, hw, c, m, s);
    }
    if (hw % 4 == 0 && aligned(feat, 16))
        return launch_cam_maps<float, 4>(feat, w, classes, cam, peak, n, k, hw, c, m, s);
    return launch_cam_maps<float, 1>(feat, w, classes, cam, peak, n, k, hw, c, m, s);
}

int lf_cam_overlay_u8(const uint8_t* img, const float* cam, const float* peak, uint8_t* out, int n, int hh, int ww,
                      int h, int wd, int m, int slot, float alpha, lf_stream_t stream) {
    LF_REQUIRE(img && cam && peak && out, "lf_cam_overlay: null buffer");
    LF_REQUIRE(n > 0 && hh > 0 && ww > 0 && h > 0 && wd > 0, "lf_cam_overlay: bad dims n=%d H=%d W=%d h=%d w=%d", n, hh,
               ww, h, wd);
    LF_REQUIRE(m >= 1 && m <= kMaxSlots && slot >= 0 && slot < m, "lf_cam_overlay: slot %d of m=%d (m in 1..%d)", slot,
               m, kMaxSlots);
    LF_REQUIRE(alpha >= 0.f && alpha <= 1.f, "lf_cam_overlay: alpha=%g outside [0, 1]", (double)alpha);
    LF_REQUIRE((long long)h * wd <= (1 << 24), "lf_cam_overlay: map of %d x %d is too large", h, wd);
    const bool vec = ww % 4 == 0 && aligned(img, 4) && aligned(out, 4);
    const bool stage = h * wd <= kOverlayLdsMap;
    const size_t groups = (size_t)hh * ww / (vec ? 4 : 1);
    const size_t per_block = (size_t)kBlock * kOverlayIters;
    const size_t bpi = (groups + per_block - 1) / per_block;
    LF_REQUIRE(bpi * (size_t)n < ((size_t)1 << 31), "lf_cam_overlay: batch of %d images of %d x %d is too large", n, hh,
               ww);
    const size_t lds = stage ? (size_t)h * wd * sizeof(float) : 0;
    auto kernel = vec ? (stage ? cam_overlay_kernel<true, true> : cam_overlay_kernel<true, false>)
                      : (stage ? cam_overlay_kernel<false, true> : cam_overlay_kernel<false, false>);
    kernel<<<(unsigned)(bpi * n), kBlock, lds, lf::as_stream(stream)>>>(img, cam, peak, out, hh, ww, h, wd, m, slot,
                                                                         alpha, (unsigned)bpi);
    return lf::check_launch("lf_cam_overlay");
}

}  // extern "C"
