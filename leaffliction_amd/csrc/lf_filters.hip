// libleafhip — the saliency ("blur") filter of srcs/transform/filters/blur.py:18-79 on batches
// of uint8 images resident in HBM.
//
// The filter is a chain of small per-pixel / 3x3-neighbourhood passes over byte and float
// planes (gray, Canny edges, plus-shaped morphology, Sobel magnitude, brown-region mask, colour
// difference against a 15x15 Gaussian, three min-max normalisations, a 5x5 Gaussian, the leaf
// mask).  Every pass is HBM/L2-bound integer or float32 work; nothing here is GEMM-shaped.
// OpenCV semantics (parity unpinned, see oracle/cv_ops.py) are restated step by step, so this
// translation unit is compiled with -ffp-contract=off; the one fused multiply-add OpenCV itself
// uses (convertTo inside cv2.normalize) is written as an explicit fmaf.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "lf_common.h"
#include "lf_draw.h"

namespace {

// ===========================================================================
// Shared by the filters below: borders and Sobel, the OpenCV pixel rules (8-bit HSV, 8-bit L*a*b*, the plant
// predicate), Canny, min / max reductions, bit planes (morphology, runs, connected components), host utilities.
// ===========================================================================
constexpr int kBlock = 256;
constexpr int kPxPerThread = 8;  // passes that end in a per-image min / max: fewer, fatter workgroups
constexpr int kHystThreads = 1024;
constexpr int kFuseT = 1024;     // the fused one-workgroup-per-image kernels
constexpr int kMaskT = 256;      // make_mask_post_kernel, brown_spots_kernel
constexpr unsigned kInfBits = 0x7f800000u;
constexpr int kLabCbrtSize = 256 * 3 / 2 * 8;   // LAB_CBRT_TAB_SIZE_B
constexpr int kSeMax = 32;
constexpr int kFlagFallback = 1, kFlagBound = 4;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- contours (make_mask's trace, lf_roi_u8, lf_shape_stats)
// One shoelace term c = x0 * y1 - x1 * y0; twice the signed area of a polygon is the sum over its edges.
__device__ __forceinline__ long long shoelace_term(int x0, int y0, int x1, int y1) {
    return (long long)x0 * y1 - (long long)x1 * y0;
}

// cv2.boundingRect of the first min(max(cnt, 0), cap) points of `pts` (x, y), by the whole workgroup of T threads:
// lo / hi = the least / greatest x and y; bad = cnt outside [0, cap] or a point outside the h x w image.  Returns
// the number of points read; nothing outside them is.  B lives in LDS and is valid after the call.
struct ContourBox {
    int lo[2], hi[2], bad;
};

template <int T>
__device__ int contour_bbox(ContourBox& B, const int* __restrict__ pts, int cnt, int cap, int h, int w) {
    if (threadIdx.x == 0) {
        B.lo[0] = B.lo[1] = INT_MAX;
        B.hi[0] = B.hi[1] = INT_MIN;
        B.bad = cnt < 0 || cnt > cap;
    }
    __syncthreads();
    const int m = min(max(cnt, 0), cap);
    int lx = INT_MAX, ly = INT_MAX, hx = INT_MIN, hy = INT_MIN, bad = 0;
    for (int i = threadIdx.x; i < m; i += T) {
        const int x = pts[2 * i], y = pts[2 * i + 1];
        bad |= x < 0 || x >= w || y < 0 || y >= h;
        lx = min(lx, x);
        ly = min(ly, y);
        hx = max(hx, x);
        hy = max(hy, y);
    }
    atomicMin(&B.lo[0], lx);
    atomicMin(&B.lo[1], ly);
    atomicMax(&B.hi[0], hx);
    atomicMax(&B.hi[1], hy);
    if (bad) atomicOr(&B.bad, 1);
    __syncthreads();
    return m;
}

// BORDER_REFLECT_101 for p in [-1, len]
__device__ __forceinline__ int reflect101i(int p, int len) {
    if (len == 1) return 0;
    if (p < 0) return -p;
    if (p >= len) return 2 * len - 2 - p;
    return p;
}

struct Sob {
    int dx, dy;
};

// 3x3 Sobel from the three (already border-mapped) rows / columns.
__device__ __forceinline__ Sob sobel_at(const uint8_t* g, int w, int y0, int y1, int y2, int x0, int x1,
                                        int x2) {
    const uint8_t* r0 = g + (size_t)y0 * w;
    const uint8_t* r1 = g + (size_t)y1 * w;
    const uint8_t* r2 = g + (size_t)y2 * w;
    const int a = r0[x0], b = r0[x1], c = r0[x2];
    const int d = r1[x0], f = r1[x2];
    const int k = r2[x0], l = r2[x1], m = r2[x2];
    Sob s;
    s.dx = (c + 2 * f + m) - (a + 2 * d + k);
    s.dy = (k + 2 * l + m) - (a + 2 * b + c);
    return s;
}

__device__ __forceinline__ unsigned gray_px_f(int r, int g, int b) {   // cv2 RGB2GRAY, 14-bit fixed point (lf_augment.hip)
    return (unsigned)(r * 4899 + g * 9617 + b * 1868 + 8192) >> 14;
}

// ---- pixel rules.  The tables live in LDS; the whole workgroup fills them and synchronises afterwards.
struct HsvTabs {   // the divisor tables of OpenCV's 8-bit RGB2HSV
    int sdiv[256], hdiv[256];
    __device__ __forceinline__ void fill(int nthreads) {
        for (int i = threadIdx.x; i < 256; i += nthreads) {
            sdiv[i] = i ? __double2int_rn(__ddiv_rn(1044480.0, (double)i)) : 0;
            hdiv[i] = i ? __double2int_rn(__ddiv_rn(737280.0, __dmul_rn(6.0, (double)i))) : 0;
        }
    }
};

struct LabTabs {   // sRGBGammaTab_b and LabCbrtTab_b of color_lab.cpp, as lab_tables_host builds them
    uint16_t gam[256], cbr[kLabCbrtSize];
    __device__ __forceinline__ void fill(const uint16_t* __restrict__ lab_tabs, int nthreads) {
        for (int i = threadIdx.x; i < 256; i += nthreads) gam[i] = lab_tabs[i];
        for (int i = threadIdx.x; i < kLabCbrtSize; i += nthreads) cbr[i] = lab_tabs[256 + i];
    }
};

// 8-bit HSV (color_hsv: H in [0, 180))
__device__ __forceinline__ void hsv_px(const HsvTabs& T, int r, int g, int b, int& hh, int& s, int& v) {
    v = max(r, max(g, b));
    const int vmin = min(r, min(g, b)), diff = v - vmin;
    const int vr = v == r ? -1 : 0, vg = v == g ? -1 : 0;
    s = (__mul24(diff, T.sdiv[v]) + (1 << 11)) >> 12;
    hh = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + ((~vg) & (r - g + 4 * diff))));
    hh = (__mul24(hh, T.hdiv[diff]) + (1 << 11)) >> 12;
    hh += hh < 0 ? 180 : 0;
}

// 8-bit L*a*b* (color_lab RGB2Lab_b)
__device__ __forceinline__ void lab_px(const LabTabs& T, int r, int g, int b, int& L, int& la, int& lb) {
    const int R = T.gam[r], G = T.gam[g], B = T.gam[b];
    const int fx = T.cbr[(R * 1777 + G * 1541 + B * 778 + 2048) >> 12];
    const int fy = T.cbr[(R * 871 + G * 2929 + B * 296 + 2048) >> 12];
    const int fz = T.cbr[(R * 73 + G * 448 + B * 3575 + 2048) >> 12];
    L = clampi((296 * fy - 1336934 + 16384) >> 15, 0, 255);
    la = clampi((500 * (fx - fy) + 4194304 + 16384) >> 15, 0, 255);
    lb = clampi((200 * (fy - fz) + 4194304 + 16384) >> 15, 0, 255);
}

// the HSV brown test of blur.py:47-53, brown.py and mask.py's brown extension
__device__ __forceinline__ bool brown_hsv(const HsvTabs& T, int r, int g, int b, int hue_lo, int hue_hi, int s_min,
                                          int v_max) {
    int hh, s, v;
    hsv_px(T, r, g, b, hh, s, v);
    return hh >= hue_lo && hh <= hue_hi && s >= s_min && v <= v_max;
}

// The per-pixel predicate of _create_inclusive_mask for pixel (y, x) = q of an h x w image: tex = gray - blurred
// gray, is_edge(q) = whether pixel q is a Canny edge (the 3x3 ellipse dilation of the edges is taken here).
template <typename IsEdge>
__device__ __forceinline__ bool plant_px(const HsvTabs& H, const LabTabs& T, int r, int g, int b, int tex, int y,
                                         int x, int h, int w, int hue_lo, int hue_hi, IsEdge is_edge) {
    int hh, s, v, L, la, lb;
    hsv_px(H, r, g, b, hh, s, v);
    lab_px(T, r, g, b, L, la, lb);
    const bool strong_green = hh >= hue_lo && hh <= hue_hi && s >= 30 && v >= 30;
    // uint8 planes: r + 15 wraps (mask.py:759-763)
    const bool dominant = g > ((r + 15) & 255) || g > ((b + 15) & 255) ||
                          (g > ((r + 5) & 255) && g > ((b + 5) & 255) && s >= 20);
    const bool lab_green = la <= 125 && lb >= 120 && L >= 20 && L <= 240;
    const int q = y * w + x;
    const bool edge = is_edge(q) || (x > 0 && is_edge(q - 1)) || (x < w - 1 && is_edge(q + 1)) ||
                      (y > 0 && is_edge(q - w)) || (y < h - 1 && is_edge(q + w));
    const bool background = (s <= 25 && v >= 50 && v <= 220) ||
                            (hh >= 120 && hh <= 160 && s >= 20 && r > g && b > g) ||
                            (s <= 15 && (tex < 0 ? -tex : tex) < 10);
    return (strong_green || dominant || lab_green || edge) && !background;
}

// ---- per-image min / max of non-negative floats through their bit patterns (monotone as uint)
struct MinMax {
    unsigned lo = kInfBits, hi = 0u;
    __device__ __forceinline__ void take(float v) {
        lo = min(lo, __float_as_uint(v));
        hi = max(hi, __float_as_uint(v));
    }
    __device__ __forceinline__ void reduce_wave() {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo = min(lo, (unsigned)__shfl_xor((int)lo, off, 64));
            hi = max(hi, (unsigned)__shfl_xor((int)hi, off, 64));
        }
    }
};

// kBlock threads, many workgroups per image: wave shuffle, then the four waves through LDS, one atomic pair per
// workgroup.
__device__ __forceinline__ void minmax_publish(MinMax r, unsigned* mn, unsigned* mx) {
    __shared__ unsigned wlo[kBlock / 64], whi[kBlock / 64];
    r.reduce_wave();
    unsigned lo = r.lo, hi = r.hi;
    if ((threadIdx.x & 63) == 0) {
        wlo[threadIdx.x >> 6] = lo;
        whi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < kBlock / 64; ++k) {
            lo = min(lo, wlo[k]);
            hi = max(hi, whi[k]);
        }
        atomicMin(mn, lo);
        atomicMax(mx, hi);
    }
}

// kFuseT threads, one workgroup per image: the result in lohi[0..1]
__device__ __forceinline__ void minmax_block(MinMax r, unsigned* wscratch, unsigned* lohi) {
    r.reduce_wave();
    unsigned lo = r.lo, hi = r.hi;
    __syncthreads();   // wscratch may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) {
        wscratch[2 * (threadIdx.x >> 6)] = lo;
        wscratch[2 * (threadIdx.x >> 6) + 1] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kFuseT / 64; ++k) {
            lo = min(lo, wscratch[2 * k]);
            hi = max(hi, wscratch[2 * k + 1]);
        }
        lohi[0] = lo;
        lohi[1] = hi;
    }
    __syncthreads();
}

// cv2.normalize(.., 0, 255, NORM_MINMAX): scale / shift in double, applied as float32 fma.
__device__ __forceinline__ void norm_coeffs(unsigned mn_bits, unsigned mx_bits, float& a, float& b) {
    const double smin = (double)__uint_as_float(mn_bits), smax = (double)__uint_as_float(mx_bits);
    const double span = smax - smin;
    const double scale = 255.0 * (span > DBL_EPSILON ? 1.0 / span : 0.0);
    const double shift = 0.0 - smin * scale;
    a = (float)scale;
    b = (float)shift;
}

__device__ __forceinline__ uint8_t trunc_u8(float v) {  // numpy float32 -> uint8 astype, in range
    const int i = (int)v;
    return (uint8_t)(i < 0 ? 0 : (i > 255 ? 255 : i));
}

// ---- Canny
// Non-maximum suppression + double threshold for the pixel (y, x) of magnitude m: the map value 1 (no edge),
// 0 (weak), 2 (strong).  grad() is the pixel's (dx, dy), asked for only above the low threshold; at(y, x) is the
// magnitude of a neighbour.
template <typename Grad, typename At>
__device__ __forceinline__ uint8_t canny_px(int m, int y, int x, int low, int high, Grad grad, At at) {
    if (m <= low) return 1;
    const Sob d = grad();
    const int xs = d.dx, ys = d.dy;
    const int ax = xs < 0 ? -xs : xs;
    const int ay = (ys < 0 ? -ys : ys) << 15;
    const int tg22x = __mul24(ax, 13573);  // tan(22.5 deg) in 15-bit fixed point
    bool keep;
    if (ay < tg22x) {
        keep = m > at(y, x - 1) && m >= at(y, x + 1);
    } else {
        const int tg67x = tg22x + (ax << 16);
        if (ay > tg67x) {
            keep = m > at(y - 1, x) && m >= at(y + 1, x);
        } else {
            const int s = (xs ^ ys) < 0 ? 1 : -1;
            keep = m > at(y - 1, x - s) && m > at(y + 1, x + s);
        }
    }
    return keep ? (m > high ? 2 : 0) : 1;
}

// The multi-launch form, on the stored magnitude and (dx, dy) planes.
__global__ __launch_bounds__(kBlock) void canny_nms_kernel(const int32_t* __restrict__ mag2,
                                                           const uint32_t* __restrict__ dxdy,
                                                           uint8_t* __restrict__ map, int h, int w,
                                                           int low, int high) {
    const unsigned n = blockIdx.y;
    const int hw = h * w;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= hw) return;
    const int32_t* mg = mag2 + (size_t)n * hw;
    const int y = p / w, x = p - y * w;
    auto grad = [&]() -> Sob {
        const unsigned pk = dxdy[(size_t)n * hw + p];
        return Sob{(int)(short)(pk & 0xffffu), (int)(short)(pk >> 16)};
    };
    auto at = [&](int yy, int xx) -> int {  // the magnitude buffer has a zero frame
        return (yy < 0 || yy >= h || xx < 0 || xx >= w) ? 0 : mg[yy * w + xx];
    };
    map[(size_t)n * hw + p] = canny_px(mg[p], y, x, low, high, grad, at);
}

// Hysteresis: one workgroup per image sweeps the map until no weak pixel next to a strong one
// is left; the map lives in LDS when it fits.  Ends with the edge image (0 / 255) in place.
__global__ __launch_bounds__(kHystThreads) void canny_hysteresis_kernel(uint8_t* __restrict__ map,
                                                                        int h, int w, int in_lds) {
    extern __shared__ uint8_t lds_map[];
    __shared__ int changed;
    const int hw = h * w;
    uint8_t* gm = map + (size_t)blockIdx.x * hw;
    uint8_t* m = gm;
    if (in_lds) {
        for (int p = threadIdx.x; p < hw; p += kHystThreads) lds_map[p] = gm[p];
        m = lds_map;
    }
    do {
        __syncthreads();
        if (threadIdx.x == 0) changed = 0;
        __syncthreads();
        bool any = false;
        for (int p = threadIdx.x; p < hw; p += kHystThreads) {
            if (m[p] != 0) continue;
            const int y = p / w, x = p - y * w;
            bool strong = false;
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= h) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= w) continue;
                    strong = strong || m[yy * w + xx] == 2;
                }
            }
            if (strong) {
                m[p] = 2;
                any = true;
            }
        }
        if (any) changed = 1;
        __syncthreads();
    } while (changed);
    for (int p = threadIdx.x; p < hw; p += kHystThreads) gm[p] = m[p] == 2 ? 255 : 0;
}

// ===========================================================================
// Round 3: the per-image middle of both filters in ONE workgroup per image, planes resident in LDS.
//
// Both multi-launch chains spend their time in launches and in round trips of small planes through L2 / HBM (13
// launches and 20 bytes of intermediates per pixel for the saliency filter).  A 224 x 224 gray plane is 50 KB: the gray
// plane, the Canny map and the bit planes of the brown regions of one image fit the 160 KB of a CU together, and
// everything the old kernels kept in 4-byte planes (squared gradient, (dx, dy), gradient magnitude, colour
// difference, saliency) is cheaper to RECOMPUTE from the gray plane in LDS / the two RGB images in L2 than to store.
// What stays outside: the two Gaussian blurs (the i8-MFMA kernel of lf_blur_mfma.hip) and the final masking pass.
// The arithmetic is the old kernels' (the bit-exact tests are unchanged).
// ===========================================================================
// Canny's non-maximum suppression + double threshold on a gray plane in LDS: map = 1 (no edge), 0 (weak),
// 2 (strong).  L1: |dx| + |dy| (cv2.Canny default), else dx^2 + dy^2 against squared thresholds.  The gradient of a
// neighbour is recomputed from the plane (8 LDS bytes) instead of being read from a 4-byte plane in memory.
template <bool L1>
__device__ __forceinline__ void canny_nms_lds(const uint8_t* gray, uint8_t* emap, int h, int w, int low, int high) {
    const int hw = h * w;
    auto sob = [&](int y, int x) -> Sob {
        return sobel_at(gray, w, clampi(y - 1, 0, h - 1), y, clampi(y + 1, 0, h - 1), clampi(x - 1, 0, w - 1), x,
                        clampi(x + 1, 0, w - 1));
    };
    auto mag = [&](const Sob s) -> int {
        return L1 ? (s.dx < 0 ? -s.dx : s.dx) + (s.dy < 0 ? -s.dy : s.dy) : __mul24(s.dx, s.dx) + __mul24(s.dy, s.dy);
    };
    auto at = [&](int yy, int xx) -> int {  // the magnitude buffer has a zero frame
        return (yy < 0 || yy >= h || xx < 0 || xx >= w) ? 0 : mag(sob(yy, xx));
    };
    const float inv_w = 1.0f / (float)w;
    for (int p = threadIdx.x; p < hw; p += kFuseT) {
        int y = (int)((float)p * inv_w);
        int x = p - __mul24(y, w);
        if (x < 0) { --y; x += w; } else if (x >= w) { ++y; x -= w; }
        const Sob s = sob(y, x);
        emap[p] = canny_px(mag(s), y, x, low, high, [&]() -> Sob { return s; }, at);
    }
    __syncthreads();
}

// Hysteresis on the map in LDS (1 = no edge, 0 = weak, 2 = strong; 2 = edge afterwards): a weak pixel with a strong
// 8-neighbour becomes strong, until nothing changes.  On bit planes — strong bits S, weak bits W, one 32-pixel word
// per thread and sweep: S |= W & dilate3x3(S) — instead of one pixel per thread with nine byte reads: a sweep over a
// 224 x 224 map is 1,792 words, and noisy images need dozens of sweeps (the byte sweeps were most of the fused
// kernels' time: 0.4 ms per image).  Rows are `wpr` words wide (two per 64-pixel segment, as the ballots deliver them).
__device__ __forceinline__ void canny_hysteresis_lds(uint8_t* m, unsigned* sb, unsigned* wb, int h, int w, int wpr,
                                                     int* changed) {
    const int spr = wpr / 2;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int seg = wv; seg < h * spr; seg += kFuseT / 64) {
        const int y = seg / spr, sx = seg - y * spr, x = sx * 64 + lane;
        const uint8_t v = x < w ? m[y * w + x] : 1;
        const unsigned long long s = __ballot(v == 2), wk = __ballot(v == 0);
        if (lane == 0) {
            sb[y * wpr + 2 * sx] = (unsigned)s;
            sb[y * wpr + 2 * sx + 1] = (unsigned)(s >> 32);
            wb[y * wpr + 2 * sx] = (unsigned)wk;
            wb[y * wpr + 2 * sx + 1] = (unsigned)(wk >> 32);
        }
    }
    do {
        __syncthreads();
        if (threadIdx.x == 0) *changed = 0;
        __syncthreads();
        bool any = false;
        for (int i = threadIdx.x; i < h * wpr; i += kFuseT) {
            const unsigned weak = wb[i] & ~sb[i];
            if (weak == 0u) continue;
            const int y = i / wpr, xw = i - y * wpr;
            unsigned nb = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= h) continue;
                const unsigned* row = sb + yy * wpr;
                const unsigned c = row[xw], pv = xw > 0 ? row[xw - 1] : 0u, nx = xw < wpr - 1 ? row[xw + 1] : 0u;
                nb |= c | (c << 1) | (pv >> 31) | (c >> 1) | (nx << 31);
            }
            const unsigned grow = weak & nb;   // (bits past column w are never weak)
            if (grow) {
                sb[i] |= grow;                 // in place: growth is monotone, the fixed point is the same
                any = true;
            }
        }
        if (any) *changed = 1;
        __syncthreads();
    } while (*changed);
    for (int seg = wv; seg < h * spr; seg += kFuseT / 64) {
        const int y = seg / spr, sx = seg - y * spr, x = sx * 64 + lane;
        if (x < w) m[y * w + x] = (sb[y * wpr + (x >> 5)] >> (x & 31) & 1u) ? 2 : 1;
    }
    __syncthreads();
}

// ---- bit planes: one bit per pixel, rows of `wpr` 32-bit words (2 * ceil(w / 64) where ballots deliver them,
// ceil(w / 32) in make_mask and the brown-spot filter)
struct BitView {
    int h, w, wpr;
};

__device__ __forceinline__ unsigned valid_bits(const BitView& G, int xw) {
    const int used = (G.w + 31) >> 5;
    const unsigned last = (G.w & 31) ? ((1u << (G.w & 31)) - 1u) : 0xffffffffu;
    return xw < used - 1 ? 0xffffffffu : (xw == used - 1 ? last : 0u);
}

__device__ __forceinline__ bool bit_at(const BitView& G, const unsigned* pl, int x, int y) {
    if ((unsigned)x >= (unsigned)G.w || (unsigned)y >= (unsigned)G.h) return false;
    return (pl[y * G.wpr + (x >> 5)] >> (x & 31)) & 1u;
}

struct SeRows {   // a structuring element as per-row column ranges relative to its anchor
    int k, ay;
    signed char lo[kSeMax], hi[kSeMax];   // lo > hi: empty row
};

// dst = dilate / erode(src) by an element of k rows anchored at row ay, rows(r, lo, hi) giving row r's column range
// relative to the anchor (lo > hi: empty); pixels outside the image never win, i.e. an erosion is the dilation of
// the complement taken INSIDE the image.  Bits past column w stay 0.  UNROLL: 1 for an element known at run time; k
// for one known at compile time, whose loops then unroll into constant funnel shifts.
template <int UNROLL, typename Rows>
__device__ __forceinline__ void morph_plane(const BitView& G, const unsigned* src, unsigned* dst, int k, int ay, Rows rows,
                                            bool erode, int nthreads) {
    const int h = G.h, wpr = G.wpr;
    for (int i = threadIdx.x; i < h * wpr; i += nthreads) {
        const int y = i / wpr, xw = i - y * wpr;
        unsigned out = 0;
#pragma unroll UNROLL
        for (int r = 0; r < k; ++r) {
            int lo, hi;
            rows(r, lo, hi);
            const int yy = y + r - ay;
            if (yy < 0 || yy >= h || lo > hi) continue;
            auto word = [&](int x) -> unsigned {
                if (x < 0 || x >= wpr) return 0u;
                const unsigned v = src[yy * wpr + x];
                return erode ? ~v & valid_bits(G, x) : v;
            };
            const unsigned cur = word(xw), prev = word(xw - 1), next = word(xw + 1);
#pragma unroll UNROLL
            for (int j = lo; j <= hi; ++j)   // the row moved by j columns: a 32-bit funnel over the neighbouring word
                out |= __funnelshift_r(j >= 0 ? cur : prev, j >= 0 ? next : cur, j & 31);
        }
        dst[i] = (erode ? ~out : out) & valid_bits(G, xw);
    }
    __syncthreads();
}

// any element, as the host lays it out (ellipse_rows)
__device__ void morph_se(const BitView& G, const unsigned* src, unsigned* dst, const SeRows& se, bool erode,
                         int nthreads) {
    morph_plane<1>(G, src, dst, se.k, se.ay, [&](int r, int& lo, int& hi) { lo = se.lo[r], hi = se.hi[r]; }, erode,
                   nthreads);
}

// cv2.getStructuringElement(MORPH_ELLIPSE, (K, K)) at compile time, for the kernels whose elements never change (the
// 224 x 224 benchmark path runs them; with run-time rows inclusive_mask measured 10 % slower): the half-width of
// each row, as ellipse_rows(K) computes it
template <int K>
struct EllipseRows;
template <>
struct EllipseRows<3> {
    static constexpr int dx[3] = {0, 1, 0};
};
template <>
struct EllipseRows<5> {
    static constexpr int dx[5] = {0, 2, 2, 2, 0};
};
template <>
struct EllipseRows<7> {
    static constexpr int dx[7] = {0, 2, 3, 3, 3, 2, 0};
};
template <>
struct EllipseRows<9> {
    static constexpr int dx[9] = {0, 3, 3, 4, 4, 4, 3, 3, 0};
};

template <int K>
__device__ void morph_ellipse(const BitView& G, const unsigned* src, unsigned* dst, bool erode, int nthreads) {
    morph_plane<K>(G, src, dst, K, K / 2, [](int r, int& lo, int& hi) { hi = EllipseRows<K>::dx[r], lo = -hi; }, erode,
                   nthreads);
}

// next run of ones in row y at or after column x: [start, end] inclusive; false when none
__device__ bool next_run(const BitView& G, const unsigned* pl, int y, int x, int& start, int& end) {
    const unsigned* row = pl + y * G.wpr;
    const int w = G.w;
    while (x < w) {
        const unsigned wd = row[x >> 5] >> (x & 31);
        if (wd == 0u) {
            x = (x | 31) + 1;
            continue;
        }
        x += __builtin_ctz(wd);
        break;
    }
    if (x >= w) return false;
    start = x;
    while (x < w) {
        const unsigned wd = ~(row[x >> 5] >> (x & 31));   // zeros above the shifted-in part end the run too
        const int room = 32 - (x & 31);
        const int ones = wd == 0u ? 32 : __builtin_ctz(wd);
        if (ones < room) {
            x += ones;
            break;
        }
        x += room;
    }
    end = (x > w ? w : x) - 1;
    return true;
}

// plane[word] = pred(y, x) for every pixel
template <typename F>
__device__ void build_plane(const BitView& G, unsigned* dst, int nthreads, F pred) {
    for (int i = threadIdx.x; i < G.h * G.wpr; i += nthreads) {
        const int y = i / G.wpr, xw = i - y * G.wpr;
        unsigned m = 0;
        const int xe = min(32, G.w - 32 * xw);
        for (int b = 0; b < xe; ++b)
            if (pred(y, 32 * xw + b)) m |= 1u << b;
        dst[i] = m;
    }
    __syncthreads();
}

// ---- connected components of a bit plane: run-length union-find
struct Run {
    unsigned short x0, x1, y, pad;
};

// one workgroup of `nt` threads per image: the planes live in LDS, runs / parents / areas in the image's slice of
// the workspace
struct Post : BitView {
    unsigned *A, *B, *C, *D;
    int* rowstart;   // LDS [h + 1]
    Run* rn;
    int* par;
    int* area;
    int max_runs, nt;
    int* nruns;    // LDS
    int* status;   // LDS
    int* flag;     // LDS [2]
    unsigned long long* best;   // LDS
};

struct PostLds {
    unsigned long long best;
    int nruns, status, flag[2];
};

// the view of workgroup blockIdx.x: `nplanes` (2 or 4) bit planes and the row index carved from `planes`; clears
// the status word (synchronise before the first walk)
__device__ __forceinline__ Post post_view(unsigned* planes, int nplanes, PostLds& S, Run* runs, int* parent,
                                          int* area, int runs_per_image, int h, int w, int wpr, int nt) {
    Post P;
    P.h = h;
    P.w = w;
    P.wpr = wpr;
    const int plane = h * wpr;
    P.A = planes;
    P.B = P.A + plane;
    P.C = nplanes > 2 ? P.B + plane : nullptr;
    P.D = nplanes > 2 ? P.C + plane : nullptr;
    P.rowstart = reinterpret_cast<int*>(planes + nplanes * plane);
    const size_t n = blockIdx.x;
    P.rn = runs + n * runs_per_image;
    P.par = parent + n * runs_per_image;
    P.area = area + n * runs_per_image;
    P.max_runs = runs_per_image;
    P.nt = nt;
    P.nruns = &S.nruns;
    P.status = &S.status;
    P.flag = S.flag;
    P.best = &S.best;
    if (threadIdx.x == 0) S.status = 0;
    return P;
}

// Lock-free union-find on the parent array.  Every walk has a hard step bound; hitting one sets kFlagBound in the
// status word.
__device__ __forceinline__ int ld_par(int* p, int x) {
    return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ int bfind(const Post& P, int x) {
    for (int i = 0; i <= P.max_runs; ++i) {
        const int px = ld_par(P.par, x);
        if (px == x) return x;
        x = px;
    }
    atomicOr(P.status, kFlagBound);
    return x;
}
__device__ void bunion(const Post& P, int a, int b) {
    for (int i = 0; i <= P.max_runs; ++i) {
        a = bfind(P, a);
        b = bfind(P, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(P.par + b, a);   // roots only move to a smaller index: a root is its first run
        if (old == b) return;
        b = old;
    }
    atomicOr(P.status, kFlagBound);
}

// runs of `src`, their connected components (par[k] = root = the component's first run in raster order) and areas.
// FLAT = false leaves out the last pass, which writes every run's root into par[k]: for a kernel that asks for each
// root once, through paint_runs<false> (with it inclusive_mask measured 8 % slower at 224 x 224).
template <bool FLAT = true>
__device__ void label_runs(const Post& P, const unsigned* src, bool conn8) {
    const int h = P.h;
    for (int y = threadIdx.x; y < h; y += P.nt) {
        int c = 0, x = 0, s, e;
        while (next_run(P, src, y, x, s, e)) {
            ++c;
            x = e + 1;
        }
        P.rowstart[y + 1] = c;
    }
    if (threadIdx.x == 0) P.rowstart[0] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int y = 0; y < h; ++y) P.rowstart[y + 1] += P.rowstart[y];
        *P.nruns = P.rowstart[h];
    }
    __syncthreads();
    for (int y = threadIdx.x; y < h; y += P.nt) {
        int k = P.rowstart[y], x = 0, s, e;
        while (next_run(P, src, y, x, s, e)) {
            P.rn[k] = Run{(unsigned short)s, (unsigned short)e, (unsigned short)y, 0};
            P.par[k] = k;
            P.area[k] = 0;
            ++k;
            x = e + 1;
        }
    }
    __threadfence();
    __syncthreads();
    const int g = conn8 ? 1 : 0;
    for (int y = 1 + threadIdx.x; y < h; y += P.nt) {
        int a = P.rowstart[y - 1], b = P.rowstart[y];
        const int a_end = P.rowstart[y], b_end = P.rowstart[y + 1];
        while (a < a_end && b < b_end) {
            const Run ra = P.rn[a], rb = P.rn[b];
            if ((int)ra.x0 <= (int)rb.x1 + g && (int)ra.x1 + g >= (int)rb.x0) bunion(P, a, b);
            if (ra.x1 < rb.x1) ++a;
            else ++b;
        }
    }
    __threadfence();
    __syncthreads();
    const int nr = *P.nruns;
    for (int k = threadIdx.x; k < nr; k += P.nt) {
        const int root = bfind(P, k);
        atomicAdd(P.area + root, (int)P.rn[k].x1 - (int)P.rn[k].x0 + 1);
    }
    __threadfence();
    __syncthreads();
    if (!FLAT) return;
    for (int k = threadIdx.x; k < nr; k += P.nt) P.par[k] = bfind(P, k);   // flatten: par[k] is the root
    __threadfence();
    __syncthreads();
}

// dst = the runs whose component passes keep(root); each thread owns whole rows
template <bool FLAT = true, typename F>
__device__ void paint_runs(const Post& P, unsigned* dst, bool clear, F keep) {
    for (int y = threadIdx.x; y < P.h; y += P.nt) {
        unsigned* row = dst + y * P.wpr;
        if (clear)
            for (int i = 0; i < P.wpr; ++i) row[i] = 0u;
        for (int k = P.rowstart[y]; k < P.rowstart[y + 1]; ++k) {
            if (!keep(FLAT ? ld_par(P.par, k) : bfind(P, k))) continue;
            const Run r = P.rn[k];
            for (int x = r.x0; x <= (int)r.x1;) {
                const int b = x & 31, len = min(32 - b, (int)r.x1 - x + 1);
                row[x >> 5] |= (len == 32 ? 0xffffffffu : ((1u << len) - 1u)) << b;
                x += len;
            }
        }
    }
    __syncthreads();
}

// ---- host utilities
constexpr size_t kAlign = 256;
inline size_t up(size_t v) { return (v + kAlign - 1) & ~(kAlign - 1); }

// A workspace layout is written once, as the take() calls of its constructor: the size query runs them on a null
// base and reads `off`, the launcher runs them on the caller's buffer.
struct Carver {
    void* base;
    size_t off = 0;
    template <typename T>
    T* take(size_t bytes) {
        T* p = base ? reinterpret_cast<T*>(static_cast<uint8_t*>(base) + off) : nullptr;
        off += up(bytes);
        return p;
    }
};

// Raises Kernel's dynamic-LDS limit to `want` bytes, once; what a launch may ask for: `want`, or `otherwise` when
// the runtime refused.
template <auto Kernel>
size_t dynamic_lds_cap(size_t want, size_t otherwise) {
    static const size_t cap = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) == hipSuccess
                                  ? want
                                  : otherwise;
    return cap;
}

// one workgroup sweeps a whole image; the map lives in LDS when it fits
void launch_canny_hysteresis(uint8_t* map, int n, int h, int w, hipStream_t s) {
    const int hw = h * w;
    const int in_lds = (size_t)hw <= dynamic_lds_cap<canny_hysteresis_kernel>(156 * 1024, 60 * 1024);
    canny_hysteresis_kernel<<<n, kHystThreads, in_lds ? (size_t)((hw + 15) & ~15) : 0, s>>>(map, h, w, in_lds);
}

// dynamic LDS of the two fused kernels, or 0 when an image does not fit a CU (the multi-launch chains then run)
constexpr size_t kFusedLdsCap = 140 * 1024;
size_t fused_lds_bytes(int h, int w, bool with_bits) {
    if (w % 4 != 0 || h < 1) return 0;
    const size_t plane = ((size_t)h * w + 15) & ~(size_t)15;
    const size_t wpr = 2 * (size_t)((w + 63) / 64);
    const size_t need = 2 * plane + (with_bits ? 3 : 2) * (size_t)h * wpr * 4;   // + strong / weak (/ brown) bit planes
    return need <= kFusedLdsCap ? need : 0;
}

// dynamic LDS of a Post: the bit planes and the row index
size_t post_lds_bytes(int nplanes, int h, int wpr) { return (size_t)nplanes * h * wpr * 4 + (size_t)(h + 1) * 4; }

// getStructuringElement(MORPH_ELLIPSE, (k, k)) with the default anchor (k / 2, k / 2)
static SeRows ellipse_rows(int k) {
    SeRows se{};
    se.k = k;
    se.ay = k / 2;
    const int r = k / 2, c = k / 2;
    const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
    for (int i = 0; i < k; ++i) {
        int j1 = 0, j2 = 0;
        const int dy = i - r;
        if (std::abs(dy) <= r) {
            const int dx = (int)nearbyint(c * std::sqrt((r * r - dy * dy) * inv_r2));
            j1 = std::max(c - dx, 0);
            j2 = std::min(c + dx + 1, k);
        }
        se.lo[i] = (signed char)(j1 - c);
        se.hi[i] = (signed char)(j2 - 1 - c);
    }
    return se;
}

static void lab_tables_host(uint16_t* out) {   // color_lab.cpp initLabTabs: sRGBGammaTab_b, LabCbrtTab_b
    for (int i = 0; i < 256; ++i) {
        const float x = (float)i / 255.0f;
        const double xd = (double)x;
        const float lin = (float)(xd <= 0.04045 ? xd / 12.92 : pow((xd + 0.055) / 1.055, 2.4));
        const long v = lrint((double)(2040.0f * lin));
        out[i] = (uint16_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
    }
    const float scale = 1.0f / (255.0f * 8.0f);
    const float lthresh = 216.0f / 24389.0f, lscale = 841.0f / 108.0f, lbias = 16.0f / 116.0f;
    for (int i = 0; i < kLabCbrtSize; ++i) {
        const float y = scale * (float)i;
        float f;
        if (y < lthresh) {
            const float prod = y * lscale;   // two roundings, as numpy's float32 arithmetic in the oracle
            f = prod + lbias;
        } else {
            f = (float)cbrt((double)y);
        }
        const long v = lrint((double)(32768.0f * f));
        out[256 + i] = (uint16_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
    }
}

// the two L*a*b* tables, built once on the host, to `dst` on the device
int upload_lab_tables(uint16_t* dst, hipStream_t s, const char* who) {
    static const std::vector<uint16_t> host_tabs = []() {
        std::vector<uint16_t> t(256 + kLabCbrtSize);
        lab_tables_host(t.data());
        return t;
    }();
    if (hipMemcpyAsync(dst, host_tabs.data(), host_tabs.size() * sizeof(uint16_t), hipMemcpyHostToDevice, s) !=
        hipSuccess) {
        lf::set_error("%s: table upload failed", who);
        return LF_ERR_LAUNCH;
    }
    return LF_OK;
}

// what every labelling kernel wants from its workspace: runs, parents, areas (h * (w / 2 + 1) per image, the most
// a bit plane can hold) and the L*a*b* tables
size_t mask_runs_per_image(int h, int w) { return (size_t)h * (w / 2 + 1); }

struct LabelBufs {
    Run* rn;
    int *parent, *area;
    uint16_t* tabs;
    void carve(Carver& c, int n, int h, int w) {
        const size_t runs = (size_t)n * mask_runs_per_image(h, w);
        rn = c.take<Run>(runs * sizeof(Run));
        parent = c.take<int>(runs * 4);
        area = c.take<int>(runs * 4);
        tabs = c.take<uint16_t>((256 + kLabCbrtSize) * sizeof(uint16_t));
    }
};

// ===========================================================================
// The saliency filter (the header of this file), multi-launch chain: the only path for images that do not fit a
// CU's LDS or whose width is not a multiple of four.
// ===========================================================================
__global__ void minmax_init_kernel(unsigned* mm, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * 6) mm[i] = (i & 1) ? 0u : kInfBits;  // (min, max) x {gradient, colour diff, saliency}
}

// Sobel of the gray plane: dx^2 + dy^2 and (dx, dy) with BORDER_REPLICATE for Canny
// (canny.cpp), sqrt(dx^2 + dy^2) with BORDER_REFLECT_101 for cv2.Sobel + cv2.magnitude.
__global__ __launch_bounds__(kBlock) void sal_sobel_kernel(const uint8_t* __restrict__ gray,
                                                           int32_t* __restrict__ mag2,
                                                           uint32_t* __restrict__ dxdy,
                                                           float* __restrict__ gmag,
                                                           unsigned* __restrict__ mm, int h, int w) {
    const unsigned n = blockIdx.y;
    const int hw = h * w;
    const uint8_t* g = gray + (size_t)n * hw;
    MinMax mmx;
    for (int k = 0; k < kPxPerThread; ++k) {
        const int p = (blockIdx.x * kPxPerThread + k) * kBlock + threadIdx.x;
        if (p >= hw) break;
        const int y = p / w, x = p - y * w;
        const Sob s = sobel_at(g, w, clampi(y - 1, 0, h - 1), y, clampi(y + 1, 0, h - 1),
                               clampi(x - 1, 0, w - 1), x, clampi(x + 1, 0, w - 1));
        mag2[(size_t)n * hw + p] = __mul24(s.dx, s.dx) + __mul24(s.dy, s.dy);  // |d| <= 1020
        dxdy[(size_t)n * hw + p] = ((unsigned)s.dx & 0xffffu) | ((unsigned)s.dy << 16);
        Sob r = s;
        if (x == 0 || y == 0 || x == w - 1 || y == h - 1)
            r = sobel_at(g, w, reflect101i(y - 1, h), y, reflect101i(y + 1, h), reflect101i(x - 1, w), x,
                         reflect101i(x + 1, w));
        const float gm = __fsqrt_rn((float)(__mul24(r.dx, r.dx) + __mul24(r.dy, r.dy)));  // < 2^24: exact
        gmag[(size_t)n * hw + p] = gm;
        mmx.take(gm);
    }
    minmax_publish(mmx, mm + n * 6 + 0, mm + n * 6 + 1);
}

// dilate / erode with the 3x3 MORPH_ELLIPSE element (a plus); outside pixels never win.
template <bool ERODE>
__global__ __launch_bounds__(kBlock) void morph_cross_kernel(const uint8_t* __restrict__ in,
                                                             uint8_t* __restrict__ out, int h, int w) {
    const unsigned n = blockIdx.y;
    const int hw = h * w;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= hw) return;
    const uint8_t* s = in + (size_t)n * hw;
    const int y = p / w, x = p - y * w;
    unsigned v = s[p];
    auto take = [&](unsigned t) { v = ERODE ? min(v, t) : max(v, t); };
    if (y > 0) take(s[p - w]);
    if (y < h - 1) take(s[p + w]);
    if (x > 0) take(s[p - 1]);
    if (x < w - 1) take(s[p + 1]);
    out[(size_t)n * hw + p] = (uint8_t)v;
}

// The planes this filter dilates / erodes hold 0 or 255 only, so max / min are OR / AND and four
// pixels go through as one dword (w % 4 == 0): the left / right neighbours are byte funnels
// with the adjacent dwords.
template <bool ERODE>
__global__ __launch_bounds__(kBlock) void morph_cross_bin4_kernel(const uint32_t* __restrict__ in,
                                                                  uint32_t* __restrict__ out, int h,
                                                                  int w4) {
    const unsigned n = blockIdx.y;
    const int total = h * w4;
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= total) return;
    const uint32_t* s = in + (size_t)n * total;
    const int y = t / w4, g = t - y * w4;
    const unsigned ident = ERODE ? 0xffffffffu : 0u;
    const unsigned c = s[t];
    const unsigned up = y > 0 ? s[t - w4] : ident, dn = y < h - 1 ? s[t + w4] : ident;
    const unsigned pv = g > 0 ? s[t - 1] : ident, nx = g < w4 - 1 ? s[t + 1] : ident;
    const unsigned left = (c << 8) | (pv >> 24), right = (c >> 8) | (nx << 24);
    out[(size_t)n * total + t] = ERODE ? (c & up & dn & left & right) : (c | up | dn | left | right);
}

// brown_regions of blur.py:47-53 as a 0 / 255 plane (OpenCV 8-bit RGB2HSV, H in [0,180)).
__global__ __launch_bounds__(kBlock) void brown_mask_kernel(const uint8_t* __restrict__ rgb,
                                                            const uint8_t* __restrict__ leaf,
                                                            uint8_t* __restrict__ out, size_t npx,
                                                            int hue_lo, int hue_hi, int s_min, int v_max) {
    __shared__ HsvTabs H;
    H.fill(kBlock);
    __syncthreads();
    for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < npx; p += (size_t)gridDim.x * kBlock) {
        const bool brown =
            brown_hsv(H, rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], hue_lo, hue_hi, s_min, v_max) && leaf[p] > 0;
        out[p] = brown ? 255 : 0;
    }
}

// mean over channels of |rgb - blurred| as numpy float32 computes it, + per-image min / max.
__global__ __launch_bounds__(kBlock) void color_diff_kernel(const uint8_t* __restrict__ rgb,
                                                            const uint8_t* __restrict__ blurred,
                                                            float* __restrict__ cdiff,
                                                            unsigned* __restrict__ mm, int hw) {
    const unsigned n = blockIdx.y;
    MinMax mmx;
    for (int k = 0; k < kPxPerThread; ++k) {
        const int p = (blockIdx.x * kPxPerThread + k) * kBlock + threadIdx.x;
        if (p >= hw) break;
        const size_t o = ((size_t)n * hw + p) * 3;
        int acc = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int d = (int)rgb[o + c] - (int)blurred[o + c];
            acc += d < 0 ? -d : d;
        }
        const float v = __fdiv_rn((float)acc, 3.0f);
        cdiff[(size_t)n * hw + p] = v;
        mmx.take(v);
    }
    minmax_publish(mmx, mm + n * 6 + 2, mm + n * 6 + 3);
}

// saliency = 0.4 edges + 0.3 uint8(norm(gradient)) + 0.6 brown + 0.2 norm(colour diff), each
// product and sum rounded to float32 in blur.py's order; + per-image min / max.
__global__ __launch_bounds__(kBlock) void saliency_kernel(const uint8_t* __restrict__ edges,
                                                          const float* __restrict__ gmag,
                                                          const uint8_t* __restrict__ brown,
                                                          const float* __restrict__ cdiff,
                                                          float* __restrict__ sal,
                                                          unsigned* __restrict__ mm, int hw) {
    const unsigned n = blockIdx.y;
    __shared__ float coef[4];
    if (threadIdx.x == 0) {
        norm_coeffs(mm[n * 6 + 0], mm[n * 6 + 1], coef[0], coef[1]);
        norm_coeffs(mm[n * 6 + 2], mm[n * 6 + 3], coef[2], coef[3]);
    }
    __syncthreads();
    const float ga = coef[0], gb = coef[1], ca = coef[2], cb = coef[3];
    MinMax mmx;
    for (int k = 0; k < kPxPerThread; ++k) {
        const int p = (blockIdx.x * kPxPerThread + k) * kBlock + threadIdx.x;
        if (p >= hw) break;
        const size_t i = (size_t)n * hw + p;
        float s = (float)edges[i] * 0.4f;
        s = s + (float)trunc_u8(__fmaf_rn(gmag[i], ga, gb)) * 0.3f;
        if (brown) s = s + (float)brown[i] * 0.6f;
        s = s + __fmaf_rn(cdiff[i], ca, cb) * 0.2f;
        sal[i] = s;
        mmx.take(s);
    }
    minmax_publish(mmx, mm + n * 6 + 4, mm + n * 6 + 5);
}

__global__ __launch_bounds__(kBlock) void saliency_norm_kernel(const float* __restrict__ sal,
                                                               const unsigned* __restrict__ mm,
                                                               uint8_t* __restrict__ out, int hw) {
    const unsigned n = blockIdx.y;
    __shared__ float coef[2];
    if (threadIdx.x == 0) norm_coeffs(mm[n * 6 + 4], mm[n * 6 + 5], coef[0], coef[1]);
    __syncthreads();
    const float a = coef[0], b = coef[1];
    for (int k = 0; k < kPxPerThread; ++k) {
        const int p = (blockIdx.x * kPxPerThread + k) * kBlock + threadIdx.x;
        if (p >= hw) break;
        out[(size_t)n * hw + p] = trunc_u8(__fmaf_rn(sal[(size_t)n * hw + p], a, b));
    }
}

// result[leaf] = blurred saliency, elsewhere 0, replicated to three channels.
__global__ __launch_bounds__(kBlock) void saliency_out_kernel(const uint8_t* __restrict__ sal,
                                                              const uint8_t* __restrict__ leaf,
                                                              uint8_t* __restrict__ out, size_t npx) {
    for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < npx; p += (size_t)gridDim.x * kBlock) {
        const uint8_t v = leaf[p] > 0 ? sal[p] : 0;
        out[3 * p] = v;
        out[3 * p + 1] = v;
        out[3 * p + 2] = v;
    }
}

// One workgroup per image: gray plane, Canny (L2 gradient, 50 / 150), brown regions (closed, dilated twice), the
// three normalisations and the weighted sum of blur.py:30-66 -> the normalised saliency plane (uint8) in `nsal`.
// rgb / blurred: [n][h][w][3]; leaf: [n][h][w]; w % 4 == 0.
__global__ __launch_bounds__(kFuseT) void saliency_fused_kernel(const uint8_t* __restrict__ rgb,
                                                                const uint8_t* __restrict__ blurred,
                                                                const uint8_t* __restrict__ leaf,
                                                                uint8_t* __restrict__ nsal, int h, int w, int use_brown,
                                                                int hue_lo, int hue_hi, int s_min, int v_max) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fl[];
    __shared__ HsvTabs H;
    __shared__ unsigned wscratch[2 * (kFuseT / 64)];
    __shared__ unsigned mm[6];
    __shared__ float coef[6];
    __shared__ int changed;
    const int hw = h * w, plane = (hw + 15) & ~15;
    const int spr = (w + 63) / 64, wpr = 2 * spr;      // 64-pixel segments / 32-bit words per bit row
    const BitView G{h, w, wpr};
    uint8_t* gray = fl;
    uint8_t* emap = fl + plane;
    unsigned* ba = reinterpret_cast<unsigned*>(fl + 2 * plane);
    unsigned* bb = ba + h * wpr;
    unsigned* hs = bb + h * wpr;   // hysteresis: strong / weak bit planes (bb is free until the brown morphology)
    const size_t n = blockIdx.x;
    const uint8_t* src = rgb + n * (size_t)hw * 3;
    const uint8_t* blr = blurred + n * (size_t)hw * 3;
    const uint8_t* lf_ = leaf + n * (size_t)hw;
    H.fill(kFuseT);
    __syncthreads();
    // ---- pass 1: gray plane; brown_regions of blur.py:47-53 as one bit per pixel (a wave = 64 pixels of a row)
    {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        for (int seg = wv; seg < h * spr; seg += kFuseT / 64) {
            const int y = seg / spr, sx = seg - y * spr, x = sx * 64 + lane;
            bool brown = false;
            if (x < w) {
                const int p = y * w + x;
                const int r = src[3 * p], g = src[3 * p + 1], b = src[3 * p + 2];
                gray[p] = (uint8_t)gray_px_f(r, g, b);
                if (use_brown) brown = brown_hsv(H, r, g, b, hue_lo, hue_hi, s_min, v_max) && lf_[p] > 0;
            }
            const unsigned long long m = __ballot(brown);
            if (lane == 0) {
                ba[y * wpr + 2 * sx] = (unsigned)m;
                ba[y * wpr + 2 * sx + 1] = (unsigned)(m >> 32);
            }
        }
    }
    __syncthreads();
    // ---- Canny(gray, 50, 150, L2gradient=True): thresholds compared squared; edges = (emap == 2)
    canny_nms_lds<false>(gray, emap, h, w, 50 * 50, 150 * 150);
    canny_hysteresis_lds(emap, hs, bb, h, w, wpr, &changed);
    // ---- brown: MORPH_CLOSE with the 3x3 ellipse (a plus), then dilate twice
    if (use_brown) {
        morph_ellipse<3>(G, ba, bb, false, kFuseT);
        morph_ellipse<3>(G, bb, ba, true, kFuseT);
        morph_ellipse<3>(G, ba, bb, false, kFuseT);
        morph_ellipse<3>(G, bb, ba, false, kFuseT);
    }
    const float inv_w = 1.0f / (float)w;
    auto rowcol = [&](int p, int& y, int& x) {
        y = (int)((float)p * inv_w);
        x = p - __mul24(y, w);
        if (x < 0) { --y; x += w; } else if (x >= w) { ++y; x -= w; }
    };
    // cv2.Sobel + cv2.magnitude (BORDER_REFLECT_101), float32 sqrt of an exact integer
    auto gmag_at = [&](int y, int x) -> float {
        const Sob r = sobel_at(gray, w, reflect101i(y - 1, h), y, reflect101i(y + 1, h), reflect101i(x - 1, w), x,
                               reflect101i(x + 1, w));
        return __fsqrt_rn((float)(__mul24(r.dx, r.dx) + __mul24(r.dy, r.dy)));
    };
    // ---- pass 2: min / max of the gradient magnitude
    {
        MinMax r;
        for (int p = threadIdx.x; p < hw; p += kFuseT) {
            int y, x;
            rowcol(p, y, x);
            r.take(gmag_at(y, x));
        }
        minmax_block(r, wscratch, mm + 0);
    }
    // mean over channels of |rgb - blurred| as numpy float32 computes it: four pixels (three dwords of each image)
    auto cdiff4 = [&](int q, float* out) {
        const uint32_t* a = reinterpret_cast<const uint32_t*>(src) + 3 * q;
        const uint32_t* b = reinterpret_cast<const uint32_t*>(blr) + 3 * q;
        const unsigned av[3] = {a[0], a[1], a[2]}, bv[3] = {b[0], b[1], b[2]};
        int acc[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const int d = (int)((av[j >> 2] >> (8 * (j & 3))) & 0xffu) - (int)((bv[j >> 2] >> (8 * (j & 3))) & 0xffu);
            acc[j / 3] += d < 0 ? -d : d;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = __fdiv_rn((float)acc[k], 3.0f);
    };
    // ---- pass 3: min / max of the colour difference
    {
        MinMax r;
        for (int q = threadIdx.x; q < hw / 4; q += kFuseT) {
            float v[4];
            cdiff4(q, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) r.take(v[k]);
        }
        minmax_block(r, wscratch, mm + 2);
    }
    if (threadIdx.x == 0) {
        norm_coeffs(mm[0], mm[1], coef[0], coef[1]);
        norm_coeffs(mm[2], mm[3], coef[2], coef[3]);
    }
    __syncthreads();
    // saliency = 0.4 dilate(edges) + 0.3 uint8(norm(gradient)) + 0.6 brown + 0.2 norm(colour diff): each product and
    // sum rounded to float32 in blur.py's order (saliency_kernel above)
    const float ga = coef[0], gb = coef[1], ca = coef[2], cb = coef[3];
    auto sal4 = [&](int q, float* out) {
        float cd[4];
        cdiff4(q, cd);
        int y, x;
        rowcol(4 * q, y, x);   // w % 4 == 0: the four pixels share a row
#pragma unroll
        for (int k = 0; k < 4; ++k, ++x) {
            const int p = 4 * q + k;
            const bool e = emap[p] == 2 || (x > 0 && emap[p - 1] == 2) || (x < w - 1 && emap[p + 1] == 2) ||
                           (y > 0 && emap[p - w] == 2) || (y < h - 1 && emap[p + w] == 2);
            float sv = (e ? 255.0f : 0.0f) * 0.4f;
            sv = sv + (float)trunc_u8(__fmaf_rn(gmag_at(y, x), ga, gb)) * 0.3f;
            if (use_brown) sv = sv + ((ba[y * wpr + (x >> 5)] >> (x & 31) & 1u) ? 255.0f : 0.0f) * 0.6f;
            sv = sv + __fmaf_rn(cd[k], ca, cb) * 0.2f;
            out[k] = sv;
        }
    };
    // ---- pass 4: min / max of the saliency
    {
        MinMax r;
        for (int q = threadIdx.x; q < hw / 4; q += kFuseT) {
            float v[4];
            sal4(q, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) r.take(v[k]);
        }
        minmax_block(r, wscratch, mm + 4);
    }
    if (threadIdx.x == 0) norm_coeffs(mm[4], mm[5], coef[4], coef[5]);
    __syncthreads();
    // ---- pass 5: the normalised saliency plane
    const float na = coef[4], nb = coef[5];
    uint32_t* dst = reinterpret_cast<uint32_t*>(nsal + n * (size_t)hw);
    for (int q = threadIdx.x; q < hw / 4; q += kFuseT) {
        float v[4];
        sal4(q, v);
        unsigned o = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) o |= (unsigned)trunc_u8(__fmaf_rn(v[k], na, nb)) << (8 * k);
        dst[q] = o;
    }
}

struct SaliencyWs {
    uint8_t *pa, *pb, *pc, *pd, *blurred;
    int32_t* mag2;
    uint32_t* dxdy;
    float* gmag;
    unsigned* mm;
    size_t bytes;
    SaliencyWs(void* base, int n, int h, int w) {
        Carver c{base};
        const size_t px = (size_t)n * h * w;
        pa = c.take<uint8_t>(px);            // gray -> brown -> closed -> normalised saliency
        pb = c.take<uint8_t>(px);            // Canny map / edges -> morphology scratch -> blurred saliency
        pc = c.take<uint8_t>(px);            // dilated edges
        pd = c.take<uint8_t>(px);            // dilated brown regions
        blurred = c.take<uint8_t>(3 * px);
        mag2 = c.take<int32_t>(4 * px);
        dxdy = c.take<uint32_t>(4 * px);
        gmag = c.take<float>(4 * px);
        mm = c.take<unsigned>((size_t)n * 6 * sizeof(unsigned));
        bytes = c.off;
    }
};

}  // namespace

extern "C" {

size_t lf_blur_saliency_workspace(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return SaliencyWs(nullptr, n, h, w).bytes;
}

int lf_blur_saliency_u8(const uint8_t* rgb, const uint8_t* leaf_mask, uint8_t* out, int n, int h, int w,
                        int use_brown, int hue_lo, int hue_hi, int s_min, int v_max,
                        const uint16_t* kq15, const uint16_t* kq5, void* workspace, size_t ws_bytes,
                        lf_stream_t stream) {
    LF_REQUIRE(rgb && leaf_mask && out && kq15 && kq5 && workspace, "lf_blur_saliency: null buffer");
    LF_REQUIRE(n > 0 && h > 0 && w > 0, "lf_blur_saliency: bad dims n=%d h=%d w=%d", n, h, w);
    LF_REQUIRE(n <= 65535, "lf_blur_saliency: batch too large for grid.y");
    LF_REQUIRE((size_t)h * w < ((size_t)1 << 30), "lf_blur_saliency: image too large");
    LF_REQUIRE(ws_bytes >= lf_blur_saliency_workspace(n, h, w),
               "lf_blur_saliency: workspace too small (%zu < %zu)", ws_bytes,
               lf_blur_saliency_workspace(n, h, w));
    LF_REQUIRE((reinterpret_cast<size_t>(workspace) & 15) == 0, "lf_blur_saliency: workspace must be 16-byte aligned");
    hipStream_t s = lf::as_stream(stream);
    const int hw = h * w;
    const size_t px = (size_t)n * hw;
    const SaliencyWs ws(workspace, n, h, w);
    uint8_t *pa = ws.pa, *pb = ws.pb, *pc = ws.pc, *pd = ws.pd, *blurred = ws.blurred;
    int32_t* mag2 = ws.mag2;
    uint32_t* dxdy = ws.dxdy;
    float* gmag = ws.gmag;
    unsigned* mm = ws.mm;
    float* cdiff = reinterpret_cast<float*>(mag2);  // mag2 is dead after the NMS pass
    float* sal = reinterpret_cast<float*>(dxdy);    // so is (dx, dy)

    const dim3 grid_px((hw + kBlock - 1) / kBlock, n);
    const dim3 grid_fat((hw + kBlock * kPxPerThread - 1) / (kBlock * kPxPerThread), n);
    int rc;
    // images that fit a CU (two byte planes + the brown bit planes in LDS; 224 x 224 does): the 15 x 15 blur, ONE
    // workgroup per image for everything up to the normalised saliency plane, the 5 x 5 blur, the masking pass
    const size_t fl = fused_lds_bytes(h, w, true);
    if (fl && dynamic_lds_cap<saliency_fused_kernel>(kFusedLdsCap, 0)) {
        rc = lf_gauss_blur_u8(rgb, blurred, n, h, w, 3, kq15, 15, stream);
        if (rc != LF_OK) return rc;
        saliency_fused_kernel<<<n, kFuseT, fl, s>>>(rgb, blurred, leaf_mask, pa, h, w, use_brown, hue_lo, hue_hi,
                                                    s_min, v_max);
        rc = lf_gauss_blur_u8(pa, pb, n, h, w, 1, kq5, 5, stream);
        if (rc != LF_OK) return rc;
        saliency_out_kernel<<<lf::stream_grid(px / 4 + 1, kBlock, lf::kFullGrid), kBlock, 0, s>>>(pb, leaf_mask, out,
                                                                                               px);
        return lf::check_launch("lf_blur_saliency");
    }
    minmax_init_kernel<<<(n * 6 + 255) / 256, 256, 0, s>>>(mm, n);
    rc = lf_rgb2gray_u8(rgb, pa, px, stream);
    if (rc != LF_OK) return rc;
    sal_sobel_kernel<<<grid_fat, kBlock, 0, s>>>(pa, mag2, dxdy, gmag, mm, h, w);
    // cv2.Canny(gray, 50, 150, L2gradient=True): thresholds are compared squared
    canny_nms_kernel<<<grid_px, kBlock, 0, s>>>(mag2, dxdy, pb, h, w, 50 * 50, 150 * 150);
    launch_canny_hysteresis(pb, n, h, w, s);
    // binary planes, 16-byte aligned, so rows of w % 4 == 0 pixels go four at a time
    const bool quad = w % 4 == 0;
    const dim3 grid_q((hw / 4 + kBlock - 1) / kBlock, n);
    auto morph = [&](const uint8_t* src, uint8_t* dst, bool erode) {
        if (quad) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
            uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
            if (erode)
                morph_cross_bin4_kernel<true><<<grid_q, kBlock, 0, s>>>(s4, d4, h, w / 4);
            else
                morph_cross_bin4_kernel<false><<<grid_q, kBlock, 0, s>>>(s4, d4, h, w / 4);
        } else if (erode) {
            morph_cross_kernel<true><<<grid_px, kBlock, 0, s>>>(src, dst, h, w);
        } else {
            morph_cross_kernel<false><<<grid_px, kBlock, 0, s>>>(src, dst, h, w);
        }
    };
    morph(pb, pc, false);
    if (use_brown) {
        brown_mask_kernel<<<lf::stream_grid(px / 4 + 1, kBlock, lf::kFullGrid), kBlock, 0, s>>>(
            rgb, leaf_mask, pa, px, hue_lo, hue_hi, s_min, v_max);
        morph(pa, pb, false);  // MORPH_CLOSE
        morph(pb, pa, true);
        morph(pa, pb, false);  // dilate, iterations=2
        morph(pb, pd, false);
    }
    rc = lf_gauss_blur_u8(rgb, blurred, n, h, w, 3, kq15, 15, stream);
    if (rc != LF_OK) return rc;
    color_diff_kernel<<<grid_fat, kBlock, 0, s>>>(rgb, blurred, cdiff, mm, hw);
    saliency_kernel<<<grid_fat, kBlock, 0, s>>>(pc, gmag, use_brown ? pd : nullptr, cdiff, sal, mm, hw);
    saliency_norm_kernel<<<grid_fat, kBlock, 0, s>>>(sal, mm, pa, hw);
    rc = lf_gauss_blur_u8(pa, pb, n, h, w, 1, kq5, 5, stream);
    if (rc != LF_OK) return rc;
    saliency_out_kernel<<<lf::stream_grid(px / 4 + 1, kBlock, lf::kFullGrid), kBlock, 0, s>>>(pb, leaf_mask, out,
                                                                                           px);
    return lf::check_launch("lf_blur_saliency");
}

}  // extern "C"

// ===========================================================================
// _create_inclusive_mask (srcs/transform/filters/mask.py:727-831): the default strategy of make_mask.
// Per-pixel colour predicates (8-bit HSV and L*a*b*, uint8 channel comparisons that wrap as numpy's
// do), Canny (L1 gradient, 30 / 100) dilated by the 3x3 ellipse, the texture test against a 15x15
// Gaussian of the gray plane -> one BIT per pixel; then, one workgroup per image with the bit planes
// in LDS: open 3x3, close 9x9, close 7x7 (cv2's MORPH_ELLIPSE elements), largest 8-connected
// component (run-length union-find), close 5x5.
// ===========================================================================
namespace {

// Canny's Sobel pass (BORDER_REPLICATE) on its own: the magnitude, |dx| + |dy| (L1, cv2.Canny's default) or
// dx^2 + dy^2, and the packed (dx, dy) that canny_nms_kernel reads.
template <bool L1>
__global__ __launch_bounds__(kBlock) void canny_sobel_kernel(const uint8_t* __restrict__ gray,
                                                             int32_t* __restrict__ mag,
                                                             uint32_t* __restrict__ dxdy, int h, int w) {
    const unsigned n = blockIdx.y;
    const int hw = h * w;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= hw) return;
    const int y = p / w, x = p - y * w;
    const Sob s = sobel_at(gray + (size_t)n * hw, w, clampi(y - 1, 0, h - 1), y, clampi(y + 1, 0, h - 1),
                           clampi(x - 1, 0, w - 1), x, clampi(x + 1, 0, w - 1));
    mag[(size_t)n * hw + p] = L1 ? (s.dx < 0 ? -s.dx : s.dx) + (s.dy < 0 ? -s.dy : s.dy)
                                 : __mul24(s.dx, s.dx) + __mul24(s.dy, s.dy);   // |d| <= 1020
    dxdy[(size_t)n * hw + p] = ((unsigned)s.dx & 0xffffu) | ((unsigned)s.dy << 16);
}

// One wave per 64-pixel segment of a row; bit i of the ballot is pixel x0 + i.
// bits[n][y][2 * seg + {0, 1}]: `wpr` = 2 * ceil(w / 64) words per row.
__global__ __launch_bounds__(kBlock) void inclusive_pred_kernel(
    const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ gray, const uint8_t* __restrict__ blur,
    const uint8_t* __restrict__ edges, const uint16_t* __restrict__ lab_tabs, uint32_t* __restrict__ bits,
    int n_images, int h, int w, int hue_lo, int hue_hi) {
    __shared__ HsvTabs H;
    __shared__ LabTabs T;
    H.fill(kBlock);
    T.fill(lab_tabs, kBlock);
    __syncthreads();
    const int spr = (w + 63) / 64, wpr = 2 * spr;
    const long total = (long)n_images * h * spr;
    const int lane = threadIdx.x & 63;
    for (long seg = (long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); seg < total;
         seg += (long)gridDim.x * (kBlock / 64)) {
        const int sx = (int)(seg % spr);
        const long ry = seg / spr;
        const int y = (int)(ry % h);
        const size_t n = (size_t)(ry / h);
        const int x = sx * 64 + lane;
        bool plant = false;
        if (x < w) {
            const size_t p = (n * h + y) * (size_t)w + x;
            const uint8_t* e = edges + (n * h) * (size_t)w;
            plant = plant_px(H, T, rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], (int)gray[p] - (int)blur[p], y, x, h, w,
                             hue_lo, hue_hi, [&](int q) { return e[q] != 0; });
        }
        const unsigned long long m = __ballot(plant);
        if (lane == 0) {
            uint32_t* o = bits + ((n * h + y) * (size_t)wpr + 2 * sx);
            o[0] = (unsigned)m;
            o[1] = (unsigned)(m >> 32);
        }
    }
}

// gray plane (from memory) -> Canny (L1 gradient, 30 / 100) in LDS -> the per-pixel predicates of
// _create_inclusive_mask -> one bit per pixel.
__global__ __launch_bounds__(kFuseT) void inclusive_fused_kernel(
    const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ gray_g, const uint8_t* __restrict__ blur,
    const uint16_t* __restrict__ lab_tabs, uint32_t* __restrict__ bits, int h, int w, int hue_lo, int hue_hi) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fl[];
    __shared__ HsvTabs H;
    __shared__ LabTabs T;
    __shared__ int changed;
    const int hw = h * w, plane = (hw + 15) & ~15;
    uint8_t* gray = fl;
    uint8_t* emap = fl + plane;
    const size_t n = blockIdx.x;
    H.fill(kFuseT);
    T.fill(lab_tabs, kFuseT);
    {
        const uint32_t* g4 = reinterpret_cast<const uint32_t*>(gray_g + n * (size_t)hw);   // hw % 4 == 0
        for (int q = threadIdx.x; q < hw / 4; q += kFuseT) reinterpret_cast<uint32_t*>(gray)[q] = g4[q];
    }
    __syncthreads();
    const int spr = (w + 63) / 64, wpr = 2 * spr;
    canny_nms_lds<true>(gray, emap, h, w, 30, 100);   // cv2.Canny(gray, 30, 100)
    {
        unsigned* hs = reinterpret_cast<unsigned*>(fl + 2 * plane);
        canny_hysteresis_lds(emap, hs, hs + h * wpr, h, w, wpr, &changed);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint8_t* src = rgb + n * (size_t)hw * 3;
    const uint8_t* bl = blur + n * (size_t)hw;
    for (int seg = wv; seg < h * spr; seg += kFuseT / 64) {
        const int y = seg / spr, sx = seg - y * spr, x = sx * 64 + lane;
        bool plant = false;
        if (x < w) {
            const int q = y * w + x;
            plant = plant_px(H, T, src[3 * q], src[3 * q + 1], src[3 * q + 2], (int)gray[q] - (int)bl[q], y, x, h, w,
                             hue_lo, hue_hi, [&](int p) { return emap[p] == 2; });
        }
        const unsigned long long m = __ballot(plant);
        if (lane == 0) {
            uint32_t* o = bits + ((n * h + y) * (size_t)wpr + 2 * sx);
            o[0] = (unsigned)m;
            o[1] = (unsigned)(m >> 32);
        }
    }
}

// One workgroup per image, the bit planes in LDS: open 3x3, close 9x9, close 7x7, the largest 8-connected
// component, close 5x5 -> the 0 / 255 mask.
__global__ __launch_bounds__(kBlock) void inclusive_morph_kernel(const uint32_t* __restrict__ bits,
                                                                 uint8_t* __restrict__ out, Run* __restrict__ runs,
                                                                 int* __restrict__ parent, int* __restrict__ area,
                                                                 int h, int w, int wpr, int runs_per_image) {
    extern __shared__ unsigned lds_bits[];
    // S.status collects the step bounds of the union-find walks.  It is not reported: lf_inclusive_mask_u8 has no
    // flags output, and a correct walk takes at most runs_per_image hops, so the bound cannot be reached.
    __shared__ PostLds S;
    const size_t n = blockIdx.x;
    const Post P = post_view(lds_bits, 2, S, runs, parent, area, runs_per_image, h, w, wpr, kBlock);
    unsigned *A = P.A, *B = P.B;
    for (int i = threadIdx.x; i < h * wpr; i += kBlock) A[i] = bits[n * h * wpr + i];
    if (threadIdx.x == 0) S.best = 0ull;
    __syncthreads();
    morph_ellipse<3>(P, A, B, true, kBlock);    // MORPH_OPEN 3x3
    morph_ellipse<3>(P, B, A, false, kBlock);
    morph_ellipse<9>(P, A, B, false, kBlock);   // MORPH_CLOSE 9x9
    morph_ellipse<9>(P, B, A, true, kBlock);
    morph_ellipse<7>(P, A, B, false, kBlock);   // MORPH_CLOSE 7x7
    morph_ellipse<7>(P, B, A, true, kBlock);

    // ---- largest 8-connected component of A -> B
    label_runs<false>(P, A, true);
    const int nruns = S.nruns;
    for (int k = threadIdx.x; k < nruns; k += kBlock) {   // largest area; the earliest component among equals
        const int a = __hip_atomic_load(P.area + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a > 0) atomicMax(&S.best, ((unsigned long long)a << 32) | (unsigned)(0x7fffffff - k));
    }
    __syncthreads();
    const int keep = 0x7fffffff - (int)(S.best & 0xffffffffull);
    paint_runs<false>(P, B, true, [&](int root) { return root == keep; });
    morph_ellipse<5>(P, B, A, false, kBlock);   // MORPH_CLOSE 5x5
    morph_ellipse<5>(P, A, B, true, kBlock);
    uint8_t* o = out + n * (size_t)h * w;
    for (int p = threadIdx.x; p < h * w; p += kBlock) {
        const int y = p / w, x = p - y * w;
        o[p] = (B[y * wpr + (x >> 5)] >> (x & 31)) & 1u ? 255 : 0;
    }
}

struct InclusiveWs {
    uint8_t *gray, *blur, *map;
    int32_t* mag;
    uint32_t *dxdy, *bits;
    LabelBufs lb;
    size_t bytes;
    InclusiveWs(void* base, int n, int h, int w) {
        Carver c{base};
        const size_t px = (size_t)n * h * w;
        gray = c.take<uint8_t>(px);
        blur = c.take<uint8_t>(px);       // the 15x15 Gaussian of the gray plane
        map = c.take<uint8_t>(px);        // Canny map -> edges
        mag = c.take<int32_t>(4 * px);    // |dx| + |dy|
        dxdy = c.take<uint32_t>(4 * px);
        bits = c.take<uint32_t>((size_t)n * h * 2 * ((w + 63) / 64) * 4);
        lb.carve(c, n, h, w);
        bytes = c.off;
    }
};

}  // namespace

extern "C" {

size_t lf_inclusive_mask_workspace(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return InclusiveWs(nullptr, n, h, w).bytes;
}

int lf_inclusive_mask_u8(const uint8_t* rgb, uint8_t* mask, int n, int h, int w, int green_lo, int green_hi,
                         const uint16_t* kq15, void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(rgb && mask && kq15 && workspace, "lf_inclusive_mask: null buffer");
    LF_REQUIRE(n > 0 && h > 0 && w > 0, "lf_inclusive_mask: bad dims n=%d h=%d w=%d", n, h, w);
    LF_REQUIRE(n <= 65535, "lf_inclusive_mask: batch too large for grid.y");
    LF_REQUIRE(w <= 65535 && h <= 65535, "lf_inclusive_mask: image too large (%d x %d)", h, w);
    LF_REQUIRE(ws_bytes >= lf_inclusive_mask_workspace(n, h, w), "lf_inclusive_mask: workspace too small (%zu < %zu)",
               ws_bytes, lf_inclusive_mask_workspace(n, h, w));
    LF_REQUIRE((reinterpret_cast<size_t>(workspace) & 15) == 0, "lf_inclusive_mask: workspace must be 16-byte aligned");
    const int wpr = 2 * ((w + 63) / 64);
    const size_t lds = post_lds_bytes(2, h, wpr);
    const size_t lds_cap = dynamic_lds_cap<inclusive_morph_kernel>(150 * 1024, 60 * 1024);
    LF_REQUIRE(lds <= lds_cap, "lf_inclusive_mask: a %d x %d image needs %zu bytes of LDS for its bit planes (limit %zu)",
               h, w, lds, lds_cap);
    hipStream_t s = lf::as_stream(stream);
    const int hw = h * w;
    const size_t px = (size_t)n * hw;
    const InclusiveWs ws(workspace, n, h, w);
    const int hue_lo = std::max(0, green_lo - 10), hue_hi = std::min(179, green_hi + 15);

    int rc = upload_lab_tables(ws.lb.tabs, s, "lf_inclusive_mask");
    if (rc != LF_OK) return rc;
    rc = lf_rgb2gray_u8(rgb, ws.gray, px, stream);
    if (rc != LF_OK) return rc;
    rc = lf_gauss_blur_u8(ws.gray, ws.blur, n, h, w, 1, kq15, 15, stream);
    if (rc != LF_OK) return rc;
    const size_t fl = fused_lds_bytes(h, w, false);
    if (fl && dynamic_lds_cap<inclusive_fused_kernel>(kFusedLdsCap, 0)) {
        // the image fits a CU: Canny and the predicates in one workgroup per image, gray plane and map in LDS
        inclusive_fused_kernel<<<n, kFuseT, fl, s>>>(rgb, ws.gray, ws.blur, ws.lb.tabs, ws.bits, h, w, hue_lo, hue_hi);
    } else {
        const dim3 grid_px((hw + kBlock - 1) / kBlock, n);
        canny_sobel_kernel<true><<<grid_px, kBlock, 0, s>>>(ws.gray, ws.mag, ws.dxdy, h, w);
        canny_nms_kernel<<<grid_px, kBlock, 0, s>>>(ws.mag, ws.dxdy, ws.map, h, w, 30, 100);   // cv2.Canny(gray, 30, 100)
        launch_canny_hysteresis(ws.map, n, h, w, s);
        const long segs = (long)n * h * ((w + 63) / 64);
        const unsigned pgrid = (unsigned)std::min<long>((segs + 3) / 4, 2048);
        inclusive_pred_kernel<<<pgrid, kBlock, 0, s>>>(rgb, ws.gray, ws.blur, ws.map, ws.lb.tabs, ws.bits, n, h, w,
                                                       hue_lo, hue_hi);
    }
    inclusive_morph_kernel<<<n, kBlock, lds, s>>>(ws.bits, mask, ws.lb.rn, ws.lb.parent, ws.lb.area, h, w, wpr,
                                                  (int)mask_runs_per_image(h, w));
    return lf::check_launch("lf_inclusive_mask");
}

}  // extern "C"

// ===========================================================================
// cv2.Canny(gray, low, high, L2gradient) on its own, for planes of any size: the multi-launch chain above (Sobel,
// non-maximum suppression with the double threshold, hysteresis) with the thresholds as arguments.
// ===========================================================================
namespace {

struct CannyWs {
    int32_t* mag;
    uint32_t* dxdy;
    size_t bytes;
    CannyWs(void* base, int n, int h, int w) {
        Carver c{base};
        const size_t px = (size_t)n * h * w;
        mag = c.take<int32_t>(4 * px);
        dxdy = c.take<uint32_t>(4 * px);
        bytes = c.off;
    }
};

// canny.cpp's integer threshold: floor(t) on |dx| + |dy|; with L2gradient floor(min(32767, t)^2) for t > 0
int canny_threshold(double t, int l2) {
    if (l2 && t > 0.0) t = std::min(32767.0, t) * std::min(32767.0, t);
    return (int)std::floor(std::max(-1.0, std::min(t, 2147483647.0)));
}

}  // namespace

extern "C" {

size_t lf_canny_workspace(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return CannyWs(nullptr, n, h, w).bytes;
}

int lf_canny_u8(const uint8_t* gray, uint8_t* edges, int n, int h, int w, double low, double high, int l2gradient,
                void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(gray && edges && workspace, "lf_canny: null buffer");
    LF_REQUIRE(n > 0 && h > 0 && w > 0, "lf_canny: bad dims n=%d h=%d w=%d", n, h, w);
    LF_REQUIRE(n <= 65535, "lf_canny: batch too large for grid.y");
    LF_REQUIRE((size_t)h * w < ((size_t)1 << 30), "lf_canny: image too large");
    LF_REQUIRE(low == low && high == high, "lf_canny: a threshold is NaN");
    LF_REQUIRE(ws_bytes >= lf_canny_workspace(n, h, w), "lf_canny: workspace too small (%zu < %zu)", ws_bytes,
               lf_canny_workspace(n, h, w));
    LF_REQUIRE((reinterpret_cast<size_t>(workspace) & 15) == 0, "lf_canny: workspace must be 16-byte aligned");
    if (low > high) std::swap(low, high);   // as cv2.Canny does
    const int lo = canny_threshold(low, l2gradient), hi = canny_threshold(high, l2gradient);
    hipStream_t s = lf::as_stream(stream);
    const int hw = h * w;
    const CannyWs ws(workspace, n, h, w);
    const dim3 grid_px((hw + kBlock - 1) / kBlock, n);
    if (l2gradient)
        canny_sobel_kernel<false><<<grid_px, kBlock, 0, s>>>(gray, ws.mag, ws.dxdy, h, w);
    else
        canny_sobel_kernel<true><<<grid_px, kBlock, 0, s>>>(gray, ws.mag, ws.dxdy, h, w);
    canny_nms_kernel<<<grid_px, kBlock, 0, s>>>(ws.mag, ws.dxdy, edges, h, w, lo, hi);
    launch_canny_hysteresis(edges, n, h, w, s);
    return lf::check_launch("lf_canny");
}

}  // extern "C"

// ===========================================================================
// make_mask (srcs/transform/filters/mask.py:548-582) for the default strategy (config.yaml:6 "inclusive").
// PARITY UNPINNED like the rest of this file (no cv2 / PlantCV / skimage here).  Readings, step by step:
//  * working image (mask.py:29-50): cv2.resize(INTER_CUBIC) on uint8 as resize.cpp's fixed-point path reads:
//    scale = 1 / (dst / src) in double, fx = (float)((dx + 0.5) * scale - 0.5), sx = floor(fx), fx -= sx, the
//    A = -0.75 weights of interpolateCubic in float, each rounded (cvRound) to Q11, replicated borders, an int
//    horizontal pass, vertical (sum + (1 << 21)) >> 22 saturated to uint8.  That is the scalar VResizeCubic; an
//    OpenCV build whose SIMD vertical pass (VResizeCubicVec_32s8u) converts to float and rounds instead may differ
//    from it by 1 in a few pixels — unverified either way.
//  * candidate: lf_inclusive_mask_u8 on the working image, unchanged.
//  * _postprocess_mask (:53-69): pcv.fill = skimage remove_small_objects (4-connected components of area <
//    fill_size removed); MORPH_CLOSE then MORPH_OPEN (ellipse morph_kernel); findContours(RETR_EXTERNAL,
//    CHAIN_APPROX_SIMPLE) + max contourArea; drawContours(filled).  A component is external when the
//    background pixel left of its first raster pixel is 4-connected to the (zero-padded) frame.  Its outer border
//    is traced Suzuki-Abe from that pixel exactly as OpenCV's icvFetchContour walks it (one lane per component,
//    on the bit plane in LDS), the area is the shoelace of the compressed polygon.  Equal areas: OpenCV lists the
//    external contours in reverse discovery order and max() keeps the first, so the LAST discovered (latest
//    first pixel in raster order) wins — a reading, not checked against cv2.  The filled polygon of an outer
//    border is the component plus everything it encloses: computed as the complement of the 4-connected flood
//    of the frame around that component alone.
//  * selection (:143-155): no contour or contourArea <= 1 -> fallback (:395-411): Otsu (thresh.cpp
//    getThreshVal_Otsu_8u, double, first maximum) of PlantCV's HSV channel, `> t`, the same post-processing.
//  * brown extension (:335-392): dilate(20 x 20 ellipse, anchor (10, 10), iterations=2) search area, the HSV or
//    L*a*b* brown predicate, open + close (brown_morph_kernel), 8-connected components of area >=
//    brown_min_area_px ORed in (no re-fill), the largest external contour of the result.
//  * back to the input size (:526-545): INTER_NEAREST min(floor(d * (1 / (dst / src))), src - 1); the contour
//    (float32(p) / float32(s)) truncated.  Neither when the scale is 1.
// Every sequential walk (border following, union-find, flood) has a hard step bound; hitting one sets bit 2 of
// the image's flag word and the host reports an error.
// ===========================================================================
namespace {

struct MaskArgs {
    int fill_size, channel;   // channel: 0 H, 1 S, 2 V of PlantCV's rgb2gray_hsv
    int use_lab, hue_lo, hue_hi, s_min, v_max, a_min, b_min, brown_min_area;
    SeRows se_morph, se_search, se_brown;
};

__device__ __forceinline__ void cubic_q11(float x, int* c) {   // interpolateCubic, then saturate_cast<short>(c * 2048)
    const float A = -0.75f;
    const float c0 = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    const float c1 = ((A + 2) * x - (A + 3)) * x * x + 1;
    const float c2 = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    const float c3 = 1.f - c0 - c1 - c2;
    c[0] = (int)rintf(c0 * 2048.f);
    c[1] = (int)rintf(c1 * 2048.f);
    c[2] = (int)rintf(c2 * 2048.f);
    c[3] = (int)rintf(c3 * 2048.f);
}

__global__ __launch_bounds__(kBlock) void cubic_resize_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              int n, int h, int w, int oh, int ow, double scale_y,
                                                              double scale_x) {
    const long total = (long)n * oh * ow;
    for (long p = (long)blockIdx.x * kBlock + threadIdx.x; p < total; p += (long)gridDim.x * kBlock) {
        const int dx = (int)(p % ow);
        const long t = p / ow;
        const int dy = (int)(t % oh);
        const size_t img = (size_t)(t / oh);
        float fx = (float)(__dsub_rn(__dmul_rn(dx + 0.5, scale_x), 0.5));
        float fy = (float)(__dsub_rn(__dmul_rn(dy + 0.5, scale_y), 0.5));
        const int sx = (int)floorf(fx), sy = (int)floorf(fy);
        fx -= (float)sx;
        fy -= (float)sy;
        int ax[4], ay[4];
        cubic_q11(fx, ax);
        cubic_q11(fy, ay);
        int xs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) xs[k] = clampi(sx - 1 + k, 0, w - 1);
        const uint8_t* s = src + img * h * w * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int acc = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint8_t* row = s + (size_t)clampi(sy - 1 + r, 0, h - 1) * w * 3 + c;
                int hs = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) hs += (int)row[xs[k] * 3] * ax[k];
                acc += hs * ay[r];
            }
            dst[(size_t)p * 3 + c] = (uint8_t)clampi((acc + (1 << 21)) >> 22, 0, 255);
        }
    }
}

// D = the background 4-connected to the zero-padded frame around `bar`
__device__ void flood_outer(const Post& P, const unsigned* bar, unsigned* D) {
    const int h = P.h, w = P.w, wpr = P.wpr;
    for (int i = threadIdx.x; i < h * wpr; i += P.nt) {
        const int y = i / wpr, xw = i - y * wpr;
        unsigned s = 0;
        if (y == 0 || y == h - 1) s = 0xffffffffu;
        if (xw == 0) s |= 1u;
        if (xw == (w - 1) >> 5) s |= 1u << ((w - 1) & 31);
        D[i] = s & ~bar[i] & valid_bits(P, xw);
    }
    if (threadIdx.x == 0) P.flag[0] = P.flag[1] = 0;
    __syncthreads();
    for (int it = 0;; ++it) {
        int local = 0;
        for (int i = threadIdx.x; i < h * wpr; i += P.nt) {
            const int y = i / wpr, xw = i - y * wpr;
            const unsigned m = ~bar[i] & valid_bits(P, xw), d = D[i];
            unsigned g = d | (d << 1) | (d >> 1);
            if (xw > 0) g |= D[i - 1] >> 31;
            if (xw < wpr - 1) g |= D[i + 1] << 31;
            if (y > 0) g |= D[i - wpr];
            if (y < h - 1) g |= D[i + wpr];
            g &= m;
            g |= ((m + g) ^ m) & m;   // along the runs of m inside the word, upwards ...
            const unsigned rm = __builtin_bitreverse32(m), rg = __builtin_bitreverse32(g);
            g |= __builtin_bitreverse32(((rm + rg) ^ rm) & rm);   // ... and downwards
            if (g != d) {
                D[i] = g;   // monotone: a neighbour reading the old or the new word is fine
                local = 1;
            }
        }
        if (local) P.flag[it & 1] = 1;
        __syncthreads();
        const int changed = P.flag[it & 1];
        if (threadIdx.x == 0) P.flag[(it + 1) & 1] = 0;
        __syncthreads();
        if (!changed) break;
        if (it > h * w) {
            if (threadIdx.x == 0) atomicOr(P.status, kFlagBound);
            break;
        }
    }
}

// OpenCV icvFetchContour, CHAIN_APPROX_SIMPLE, outer border from its first raster pixel (x0, y0).  Returns the
// number of points; area2 = twice contourArea.  out (optional): the first `cap` points, divided by fs if rescale.
__device__ int trace_outer(const Post& P, const unsigned* pl, int x0, int y0, long long& area2, int* out, int cap,
                           bool rescale, float fs) {
    const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
    const int DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};
    int npts = 0, fx = 0, fy = 0, px = 0, py = 0;
    long long a2 = 0;
    auto emit = [&](int x, int y) {
        if (out && npts < cap) {
            out[2 * npts] = rescale ? (int)__fdiv_rn((float)x, fs) : x;
            out[2 * npts + 1] = rescale ? (int)__fdiv_rn((float)y, fs) : y;
        }
        if (npts == 0) {
            fx = x;
            fy = y;
        } else {
            a2 += shoelace_term(px, py, x, y);
        }
        px = x;
        py = y;
        ++npts;
    };
    int s = 4;
    do {
        s = (s - 1) & 7;
    } while (!bit_at(P, pl, x0 + DX[s], y0 + DY[s]) && s != 4);
    if (s == 4) {   // single-pixel component
        emit(x0, y0);
        area2 = 0;
        return 1;
    }
    const int x1 = x0 + DX[s], y1 = y0 + DY[s];
    int x3 = x0, y3 = y0, prev_s = s ^ 4;
    const long long bound = 4ll * P.h * P.w + 16;
    for (long long step = 0;; ++step) {
        int k = s + 1;
        for (; k < 16; ++k)
            if (bit_at(P, pl, x3 + DX[k & 7], y3 + DY[k & 7])) break;
        if (k == 16 || step > bound) {
            atomicOr(P.status, kFlagBound);
            break;
        }
        s = k & 7;
        if (s != prev_s) {
            emit(x3, y3);
            prev_s = s;
        }
        const int x4 = x3 + DX[s], y4 = y3 + DY[s];
        if (x4 == x0 && y4 == y0 && x3 == x1 && y3 == y1) break;
        x3 = x4;
        y3 = y4;
        s = (s + 4) & 7;
    }
    a2 += shoelace_term(px, py, fx, fy);
    area2 = a2 < 0 ? -a2 : a2;
    return npts;
}

// largest external contour of P.A (labels P.A, leaves D = the outer background).  Returns the winning root or -1
// and its doubled area.
__device__ int largest_external(const Post& P, long long& area2) {
    label_runs(P, P.A, true);
    flood_outer(P, P.A, P.D);
    if (threadIdx.x == 0) *P.best = 0ull;
    __syncthreads();
    const int nr = *P.nruns;
    for (int k = threadIdx.x; k < nr; k += P.nt) {
        if (P.par[k] != k) continue;
        const Run r = P.rn[k];
        if (r.x0 > 0 && !bit_at(P, P.D, r.x0 - 1, r.y)) continue;   // inside a hole of another component
        long long a2;
        trace_outer(P, P.A, r.x0, r.y, a2, nullptr, 0, false, 1.f);
        atomicMax(P.best, ((unsigned long long)a2 << 32) | (unsigned)(k + 1));   // equal areas: the later one
    }
    __syncthreads();
    const unsigned long long b = *P.best;
    __syncthreads();
    area2 = (long long)(b >> 32);
    return b ? (int)(b & 0xffffffffull) - 1 : -1;
}

// _postprocess_mask on P.A: fill, close, open, largest contour, its filled polygon back in P.A.  Returns whether a
// contour exists; area2 = twice its area.
__device__ bool postprocess(const Post& P, const MaskArgs& a, long long& area2) {
    label_runs(P, P.A, false);   // pcv.fill: 4-connected components below fill_size go
    paint_runs(P, P.A, true, [&](int root) { return P.area[root] >= a.fill_size; });
    morph_se(P, P.A, P.B, a.se_morph, false, P.nt);   // MORPH_CLOSE
    morph_se(P, P.B, P.A, a.se_morph, true, P.nt);
    morph_se(P, P.A, P.B, a.se_morph, true, P.nt);    // MORPH_OPEN
    morph_se(P, P.B, P.A, a.se_morph, false, P.nt);
    const int best = largest_external(P, area2);
    if (best < 0) return false;
    paint_runs(P, P.B, true, [&](int root) { return root == best; });   // drawContours(filled)
    flood_outer(P, P.B, P.D);
    for (int i = threadIdx.x; i < P.h * P.wpr; i += P.nt) P.A[i] = ~P.D[i] & valid_bits(P, i % P.wpr);
    __syncthreads();
    return true;
}

// PlantCV's rgb2gray_hsv converts with COLOR_BGR2HSV although it is handed RGB: H is taken from the swapped pixel.
// S and V do not change under an R / B swap, so the default channel "s" is unaffected by that mix-up.
__device__ __forceinline__ int channel_px(const HsvTabs& T, const uint8_t* p, int channel) {
    int hh, s, v;
    hsv_px(T, p[2], p[1], p[0], hh, s, v);
    return channel == 0 ? hh : (channel == 1 ? s : v);
}

__device__ __forceinline__ bool brown_px(const HsvTabs& H, const LabTabs& T, const uint8_t* p, const MaskArgs& a) {
    const int r = p[0], g = p[1], b = p[2];
    if (a.use_lab) {
        int L, la, lb;
        lab_px(T, r, g, b, L, la, lb);
        return la >= a.a_min && lb >= a.b_min;
    }
    return brown_hsv(H, r, g, b, a.hue_lo, a.hue_hi, a.s_min, a.v_max);
}

__global__ __launch_bounds__(kMaskT) void make_mask_post_kernel(
    const uint8_t* __restrict__ rgbw, const uint8_t* __restrict__ cand, const uint16_t* __restrict__ lab_tabs,
    Run* __restrict__ runs, int* __restrict__ parent, int* __restrict__ area, int runs_per_image, int h, int w,
    int wpr, int oh, int ow, int rescale, double ify, double ifx, float fscale, MaskArgs a,
    uint8_t* __restrict__ out_mask, int* __restrict__ contour, int* __restrict__ counts, int* __restrict__ flags,
    int cap) {
    extern __shared__ unsigned lds_planes[];
    __shared__ HsvTabs H;
    __shared__ LabTabs T;
    __shared__ PostLds S;
    __shared__ int s_hist[256], s_thresh;
    const size_t n = blockIdx.x;
    const Post P = post_view(lds_planes, 4, S, runs, parent, area, runs_per_image, h, w, wpr, kMaskT);
    H.fill(kMaskT);
    T.fill(lab_tabs, kMaskT);
    for (int i = threadIdx.x; i < 256; i += kMaskT) s_hist[i] = 0;
    const uint8_t* img = rgbw + n * (size_t)h * w * 3;
    const uint8_t* cm = cand + n * (size_t)h * w;
    __syncthreads();

    build_plane(P, P.A, kMaskT, [&](int y, int x) { return cm[y * w + x] > 0; });
    long long area2 = 0;
    const bool found = postprocess(P, a, area2);
    int flag = 0;
    if (!found || area2 <= 2) {   // _score_mask == -1: no best mask -> _create_fallback_mask
        flag |= kFlagFallback;
        for (int p = threadIdx.x; p < h * w; p += kMaskT) atomicAdd(&s_hist[channel_px(H, img + 3 * p, a.channel)], 1);
        __syncthreads();
        if (threadIdx.x == 0) {   // getThreshVal_Otsu_8u
            const double scale = 1.0 / ((double)h * w);
            double mu = 0.0;
            for (int i = 0; i < 256; ++i) mu = __dadd_rn(mu, __dmul_rn((double)i, (double)s_hist[i]));
            mu = __dmul_rn(mu, scale);
            double mu1 = 0.0, q1 = 0.0, max_sigma = 0.0;
            int max_val = 0;
            for (int i = 0; i < 256; ++i) {
                const double p_i = __dmul_rn((double)s_hist[i], scale);
                mu1 = __dmul_rn(mu1, q1);
                q1 = __dadd_rn(q1, p_i);
                const double q2 = __dsub_rn(1.0, q1);
                if (fmin(q1, q2) < (double)FLT_EPSILON || fmax(q1, q2) > __dsub_rn(1.0, (double)FLT_EPSILON)) continue;
                mu1 = __ddiv_rn(__dadd_rn(mu1, __dmul_rn((double)i, p_i)), q1);
                const double mu2 = __ddiv_rn(__dsub_rn(mu, __dmul_rn(q1, mu1)), q2);
                const double d = __dsub_rn(mu1, mu2);
                const double sigma = __dmul_rn(__dmul_rn(__dmul_rn(q1, q2), d), d);
                if (sigma > max_sigma) {
                    max_sigma = sigma;
                    max_val = i;
                }
            }
            s_thresh = max_val;
        }
        __syncthreads();
        const int t = s_thresh;
        build_plane(P, P.A, kMaskT, [&](int y, int x) { return channel_px(H, img + 3 * (y * w + x), a.channel) > t; });
        postprocess(P, a, area2);
    }

    // _extend_mask_with_brown_regions
    morph_se(P, P.A, P.B, a.se_search, false, kMaskT);
    morph_se(P, P.B, P.C, a.se_search, false, kMaskT);
    build_plane(P, P.B, kMaskT, [&](int y, int x) {
        return ((P.C[y * wpr + (x >> 5)] >> (x & 31)) & 1u) && brown_px(H, T, img + 3 * (y * w + x), a);
    });
    morph_se(P, P.B, P.C, a.se_brown, true, kMaskT);   // MORPH_OPEN
    morph_se(P, P.C, P.B, a.se_brown, false, kMaskT);
    morph_se(P, P.B, P.C, a.se_brown, false, kMaskT);  // MORPH_CLOSE
    morph_se(P, P.C, P.B, a.se_brown, true, kMaskT);
    label_runs(P, P.B, true);
    paint_runs(P, P.A, false, [&](int root) { return P.area[root] >= a.brown_min_area; });
    const int best = largest_external(P, area2);
    if (threadIdx.x == 0) {
        int npts = 0;
        if (best >= 0) {
            const Run r = P.rn[best];
            long long a2;
            npts = trace_outer(P, P.A, r.x0, r.y, a2, contour + n * (size_t)cap * 2, cap, rescale != 0, fscale);
        }
        counts[n] = npts;
    }
    __syncthreads();
    uint8_t* o = out_mask + n * (size_t)oh * ow;
    for (int p = threadIdx.x; p < oh * ow; p += kMaskT) {
        const int y = p / ow, x = p - y * ow;
        int sy = y, sx = x;
        if (rescale) {
            sy = min((int)floor(__dmul_rn((double)y, ify)), h - 1);
            sx = min((int)floor(__dmul_rn((double)x, ifx)), w - 1);
        }
        o[p] = (P.A[sy * wpr + (sx >> 5)] >> (sx & 31)) & 1u ? 255 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) flags[n] = flag | S.status;
}

constexpr size_t kMaskLdsCap = 140 * 1024;

struct MakeMaskWs {
    uint8_t *work, *cand, *incl;
    size_t incl_bytes;
    LabelBufs lb;
    size_t bytes;
    MakeMaskWs(void* base, int n, int wh, int ww) {
        Carver c{base};
        const size_t wpx = (size_t)n * wh * ww;
        work = c.take<uint8_t>(3 * wpx);   // the working image
        cand = c.take<uint8_t>(wpx);       // the candidate mask
        incl_bytes = InclusiveWs(nullptr, n, wh, ww).bytes;
        incl = c.take<uint8_t>(incl_bytes);   // the candidate's own workspace
        lb.carve(c, n, wh, ww);
        bytes = c.off;
    }
};

}  // namespace

extern "C" {

size_t lf_make_mask_workspace(int n, int h, int w, int wh, int ww) {
    if (n <= 0 || h <= 0 || w <= 0 || wh <= 0 || ww <= 0) return 0;
    return MakeMaskWs(nullptr, n, wh, ww).bytes;
}

int lf_make_mask_u8(const uint8_t* rgb, uint8_t* mask, int32_t* contour, int32_t* counts, int32_t* flags, int n,
                    int h, int w, int wh, int ww, int rescale, double scale, const lf_make_mask_params* prm, int cap,
                    const uint16_t* kq15, void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(rgb && mask && contour && counts && flags && prm && kq15 && workspace, "lf_make_mask: null buffer");
    LF_REQUIRE(n > 0 && h > 0 && w > 0 && wh > 0 && ww > 0 && cap > 0, "lf_make_mask: bad dims n=%d %dx%d -> %dx%d cap=%d",
               n, h, w, wh, ww, cap);
    LF_REQUIRE(n <= 65535, "lf_make_mask: batch too large for the grid");
    LF_REQUIRE(rescale || (wh == h && ww == w), "lf_make_mask: without rescaling the working size is the input size");
    LF_REQUIRE(!rescale || scale > 0.0, "lf_make_mask: scale must be positive");
    LF_REQUIRE(wh <= 65535 && ww <= 65535, "lf_make_mask: working image too large (%d x %d)", wh, ww);
    const size_t lds = post_lds_bytes(4, wh, (ww + 31) / 32);
    LF_REQUIRE(lds <= kMaskLdsCap,
               "lf_make_mask: a %d x %d working image needs %zu bytes of LDS for its four bit planes (limit %zu, one "
               "workgroup per image)", wh, ww, lds, kMaskLdsCap);
    const int ks[3] = {prm->morph_kernel, 20, prm->brown_morph_kernel};
    for (int k : ks) LF_REQUIRE(k >= 1 && k <= 31, "lf_make_mask: structuring element size %d outside [1, 31]", k);
    LF_REQUIRE(prm->hsv_channel >= 0 && prm->hsv_channel <= 2, "lf_make_mask: hsv_channel must be 0, 1 or 2");
    LF_REQUIRE(ws_bytes >= lf_make_mask_workspace(n, h, w, wh, ww), "lf_make_mask: workspace too small (%zu < %zu)",
               ws_bytes, lf_make_mask_workspace(n, h, w, wh, ww));
    LF_REQUIRE((reinterpret_cast<size_t>(workspace) & 255) == 0, "lf_make_mask: workspace must be 256-byte aligned");
    LF_REQUIRE(lds <= dynamic_lds_cap<make_mask_post_kernel>(kMaskLdsCap, 48 * 1024),
               "lf_make_mask: could not raise the LDS limit of the mask kernel");

    hipStream_t s = lf::as_stream(stream);
    const size_t wpx = (size_t)n * wh * ww;
    const MakeMaskWs ws(workspace, n, wh, ww);

    MaskArgs a{};
    a.fill_size = prm->fill_size;
    a.channel = prm->hsv_channel;
    a.use_lab = prm->use_lab_brown;
    a.hue_lo = prm->brown_hue_lo;
    a.hue_hi = prm->brown_hue_hi;
    a.s_min = prm->brown_s_min;
    a.v_max = prm->brown_v_max;
    a.a_min = prm->lab_a_min;
    a.b_min = prm->lab_b_min;
    a.brown_min_area = prm->brown_min_area_px;
    a.se_morph = ellipse_rows(prm->morph_kernel);
    a.se_search = ellipse_rows(20);
    a.se_brown = ellipse_rows(prm->brown_morph_kernel);

    int rc = upload_lab_tables(ws.lb.tabs, s, "lf_make_mask");
    if (rc != LF_OK) return rc;
    const uint8_t* src = rgb;
    if (rescale) {
        const double sy = 1.0 / ((double)wh / h), sx = 1.0 / ((double)ww / w);
        cubic_resize_kernel<<<lf::stream_grid(wpx, kBlock), kBlock, 0, s>>>(rgb, ws.work, n, h, w, wh, ww, sy, sx);
        rc = lf::check_launch("lf_make_mask (resize)");
        if (rc != LF_OK) return rc;
        src = ws.work;
    }
    rc = lf_inclusive_mask_u8(src, ws.cand, n, wh, ww, prm->green_lo, prm->green_hi, kq15, ws.incl, ws.incl_bytes,
                              stream);
    if (rc != LF_OK) return rc;
    const double ify = 1.0 / ((double)h / wh), ifx = 1.0 / ((double)w / ww);
    make_mask_post_kernel<<<n, kMaskT, lds, s>>>(src, ws.cand, ws.lb.tabs, ws.lb.rn, ws.lb.parent, ws.lb.area,
                                                 (int)mask_runs_per_image(wh, ww), wh, ww, (ww + 31) / 32, h, w,
                                                 rescale, ify, ifx, (float)scale, a, mask, contour, counts, flags, cap);
    return lf::check_launch("lf_make_mask");
}

}  // extern "C"

// ===========================================================================
// apply_brown_filter (srcs/transform/filters/brown.py) for a same-size batch: one workgroup per image, two bit
// planes in LDS, the shared helpers (brown_px, morph_se, label_runs, paint_runs).
//  * leaf = mask > 0; the predicate on the pixel as handed in (no R / B swap): 8-bit HSV (H in [0, 180))
//    lo <= h <= hi, s >= s_min, v <= v_max, or L*a*b* a >= a_min, b >= b_min when use_lab; ANDed with leaf.
//  * MORPH_OPEN then MORPH_CLOSE with getStructuringElement(MORPH_ELLIPSE, (k, k)), default borders: pixels outside
//    the image never win (morph_se's rule).
//  * connectedComponentsWithStats(connectivity=8): the components of area >= min_area are kept.
//  * out = the input with every kept pixel set to (255, 100, 0); stats[n] = {count, brown area, leaf area}.
// The union-find walks carry make_mask's step bounds: hitting one sets bit 2 of flags[n].
// ===========================================================================
namespace {

// The pipeline above up to its labelling, for brown_spots_kernel and lesion_table_kernel: P.A = the predicate
// inside the leaf, opened and closed; its runs, their roots (flattened) and the components' areas.  P.B is scratch.
__device__ void brown_label(const Post& P, const HsvTabs& H, const LabTabs& T, const uint8_t* img, const uint8_t* lm,
                            const MaskArgs& a) {
    const int w = P.w;
    build_plane(P, P.A, kMaskT,
                [&](int y, int x) { return lm[y * w + x] > 0 && brown_px(H, T, img + 3 * (y * w + x), a); });
    morph_se(P, P.A, P.B, a.se_brown, true, kMaskT);   // MORPH_OPEN
    morph_se(P, P.B, P.A, a.se_brown, false, kMaskT);
    morph_se(P, P.A, P.B, a.se_brown, false, kMaskT);  // MORPH_CLOSE
    morph_se(P, P.B, P.A, a.se_brown, true, kMaskT);
    label_runs(P, P.A, true);
}

__global__ __launch_bounds__(kMaskT) void brown_spots_kernel(const uint8_t* __restrict__ rgb,
                                                             const uint8_t* __restrict__ leaf_mask,
                                                             const uint16_t* __restrict__ lab_tabs, Run* __restrict__ runs,
                                                             int* __restrict__ parent, int* __restrict__ area,
                                                             int runs_per_image, int h, int w, int wpr, MaskArgs a,
                                                             uint8_t* __restrict__ out, int* __restrict__ stats,
                                                             int* __restrict__ flags) {
    extern __shared__ unsigned lds_planes[];
    __shared__ HsvTabs H;
    __shared__ LabTabs T;
    __shared__ PostLds S;
    __shared__ int s_count, s_brown, s_leaf;
    const size_t n = blockIdx.x;
    const Post P = post_view(lds_planes, 2, S, runs, parent, area, runs_per_image, h, w, wpr, kMaskT);
    H.fill(kMaskT);
    T.fill(lab_tabs, kMaskT);
    if (threadIdx.x == 0) s_count = s_brown = s_leaf = 0;
    const uint8_t* img = rgb + n * (size_t)h * w * 3;
    const uint8_t* lm = leaf_mask + n * (size_t)h * w;
    __syncthreads();

    int leaf = 0;
    for (int p = threadIdx.x; p < h * w; p += kMaskT) leaf += lm[p] > 0;
    atomicAdd(&s_leaf, leaf);
    brown_label(P, H, T, img, lm, a);
    const int nr = *P.nruns;
    int cnt = 0, px = 0;
    for (int k = threadIdx.x; k < nr; k += kMaskT) {
        if (P.par[k] != k || P.area[k] < a.brown_min_area) continue;
        ++cnt;
        px += P.area[k];
    }
    atomicAdd(&s_count, cnt);
    atomicAdd(&s_brown, px);
    paint_runs(P, P.B, true, [&](int root) { return P.area[root] >= a.brown_min_area; });
    uint8_t* o = out + n * (size_t)h * w * 3;
    for (int p = threadIdx.x; p < h * w; p += kMaskT) {
        const int y = p / w, x = p - y * w;
        const bool keep = (P.B[y * wpr + (x >> 5)] >> (x & 31)) & 1u;
        o[3 * p] = keep ? 255 : img[3 * p];
        o[3 * p + 1] = keep ? 100 : img[3 * p + 1];
        o[3 * p + 2] = keep ? 0 : img[3 * p + 2];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[3 * n] = s_count;
        stats[3 * n + 1] = s_brown;
        stats[3 * n + 2] = s_leaf;
        flags[n] = S.status;
    }
}

struct BrownWs {
    LabelBufs lb;
    size_t bytes;
    BrownWs(void* base, int n, int h, int w) {
        Carver c{base};
        lb.carve(c, n, h, w);
        bytes = c.off;
    }
};

// the kernel's view of lf_brown_params (morph_kernel checked by the caller)
MaskArgs brown_args(const lf_brown_params* prm) {
    MaskArgs a{};
    a.use_lab = prm->use_lab_brown;
    a.hue_lo = prm->hue_lo;
    a.hue_hi = prm->hue_hi;
    a.s_min = prm->s_min;
    a.v_max = prm->v_max;
    a.a_min = prm->lab_a_min;
    a.b_min = prm->lab_b_min;
    a.brown_min_area = prm->min_area_px;
    a.se_brown = ellipse_rows(prm->morph_kernel);
    return a;
}

}  // namespace

extern "C" {

size_t lf_brown_spots_workspace(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return BrownWs(nullptr, n, h, w).bytes;
}

int lf_brown_spots_u8(const uint8_t* rgb, const uint8_t* mask, uint8_t* out, int32_t* stats, int32_t* flags, int n,
                      int h, int w, const lf_brown_params* prm, void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(rgb && mask && out && stats && flags && prm && workspace, "lf_brown_spots: null buffer");
    LF_REQUIRE(n > 0 && h > 0 && w > 0, "lf_brown_spots: bad dims n=%d %dx%d", n, h, w);
    LF_REQUIRE(n <= 65535, "lf_brown_spots: batch too large for the grid");
    LF_REQUIRE(h <= 65535 && w <= 65535, "lf_brown_spots: image too large (%d x %d)", h, w);
    const size_t lds = post_lds_bytes(2, h, (w + 31) / 32);
    LF_REQUIRE(lds <= kMaskLdsCap,
               "lf_brown_spots: a %d x %d image needs %zu bytes of LDS for its two bit planes (limit %zu, one "
               "workgroup per image)", h, w, lds, kMaskLdsCap);
    LF_REQUIRE(prm->morph_kernel >= 1 && prm->morph_kernel <= 31,
               "lf_brown_spots: brown_morph_kernel %d outside [1, 31]", prm->morph_kernel);
    LF_REQUIRE(ws_bytes >= lf_brown_spots_workspace(n, h, w), "lf_brown_spots: workspace too small (%zu < %zu)",
               ws_bytes, lf_brown_spots_workspace(n, h, w));
    LF_REQUIRE((reinterpret_cast<size_t>(workspace) & 255) == 0, "lf_brown_spots: workspace must be 256-byte aligned");
    LF_REQUIRE(lds <= dynamic_lds_cap<brown_spots_kernel>(kMaskLdsCap, 48 * 1024),
               "lf_brown_spots: could not raise the LDS limit of the brown kernel");

    hipStream_t s = lf::as_stream(stream);
    const BrownWs ws(workspace, n, h, w);

    const MaskArgs a = brown_args(prm);
    const int rc = upload_lab_tables(ws.lb.tabs, s, "lf_brown_spots");
    if (rc != LF_OK) return rc;
    brown_spots_kernel<<<n, kMaskT, lds, s>>>(rgb, mask, ws.lb.tabs, ws.lb.rn, ws.lb.parent, ws.lb.area,
                                              (int)mask_runs_per_image(h, w), h, w, (w + 31) / 32, a, out, stats, flags);
    return lf::check_launch("lf_brown_spots");
}

}  // extern "C"

// ===========================================================================
// The lesion table: one row of integers per component lf_brown_spots_u8 keeps (brown_label and the area test, the
// pipeline above), in raster order of the components' first pixels, which is the order of label_runs' roots.  One
// workgroup per image, the same two bit planes in LDS.
//  * a prefix count over the runs gives every kept root its row; its owner writes the area and seeds the bounding box
//    with the root run (the component's topmost row);
//  * a lane per run adds the run's closed forms (sum x, sum y, the box) and what its pixels give (the colour sums and
//    the two neighbour tests) to the row with 64-bit integer adds, minima and maxima: no order to depend on.
// A 4-neighbour that is set in P.A belongs to the pixel's own component, so "not in the lesion" is "not set in P.A".
// ===========================================================================
namespace {

__device__ __forceinline__ long long ld_i64(const long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void add_i64(long long* p, long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kMaskT) void lesion_table_kernel(const uint8_t* __restrict__ rgb,
                                                              const uint8_t* __restrict__ leaf_mask,
                                                              const uint16_t* __restrict__ lab_tabs, Run* __restrict__ runs,
                                                              int* __restrict__ parent, int* __restrict__ area,
                                                              int runs_per_image, int h, int w, int wpr, MaskArgs a,
                                                              long long* __restrict__ table, int* __restrict__ counts,
                                                              int* __restrict__ flags, int cap) {
    extern __shared__ unsigned lds_planes[];
    __shared__ HsvTabs H;
    __shared__ LabTabs T;
    __shared__ PostLds S;
    __shared__ int s_roots[kMaskT];
    __shared__ int s_total;
    constexpr int F = LF_LESION_FIELDS;
    const size_t n = blockIdx.x;
    const Post P = post_view(lds_planes, 2, S, runs, parent, area, runs_per_image, h, w, wpr, kMaskT);
    H.fill(kMaskT);
    T.fill(lab_tabs, kMaskT);
    const uint8_t* img = rgb + n * (size_t)h * w * 3;
    const uint8_t* lm = leaf_mask + n * (size_t)h * w;
    long long* tab = table + n * (size_t)cap * F;
    for (size_t i = threadIdx.x; i < (size_t)cap * F; i += kMaskT) tab[i] = 0;
    __syncthreads();

    brown_label(P, H, T, img, lm, a);

    // rows: thread t owns the runs [k0, k1); the kept roots before k0 are the rows before its first
    const int nr = *P.nruns;
    const int chunk = (nr + kMaskT - 1) / kMaskT;
    const int k0 = min(nr, (int)threadIdx.x * chunk), k1 = min(nr, k0 + chunk);
    int mine = 0;
    for (int k = k0; k < k1; ++k) mine += P.par[k] == k && P.area[k] >= a.brown_min_area;
    s_roots[threadIdx.x] = mine;
    __syncthreads();
    int row = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) row += s_roots[t];
    if (threadIdx.x == kMaskT - 1) s_total = row + mine;
    for (int k = k0; k < k1; ++k) {
        if (P.par[k] != k) continue;
        const int ar = P.area[k];
        int slot = -1;
        if (ar >= a.brown_min_area) {
            if (row < cap) slot = row;
            ++row;
        }
        P.area[k] = slot;   // from here on area[root] is the component's row; -1: not in the table
        if (slot < 0) continue;
        const Run r = P.rn[k];
        long long* o = tab + (size_t)slot * F;
        o[0] = ar;
        o[1] = r.x0;   // least x so far
        o[2] = r.y;    // the root run lies in the component's topmost row
        o[3] = r.x1;   // greatest x so far
        o[4] = r.y;    // greatest y so far
    }
    __threadfence();
    __syncthreads();

    for (int k = threadIdx.x; k < nr; k += kMaskT) {
        const int slot = ld_par(P.area, P.par[k]);
        if (slot < 0) continue;
        const Run r = P.rn[k];
        const int y = r.y, x0 = r.x0, x1 = r.x1;
        int sr = 0, sg = 0, sb = 0, border = 0, margin = 0;
        for (int x = x0; x <= x1; ++x) {
            const size_t p = (size_t)y * w + x;
            sr += img[3 * p];
            sg += img[3 * p + 1];
            sb += img[3 * p + 2];
            const bool inside = x > x0 && x < x1 && bit_at(P, P.A, x, y - 1) && bit_at(P, P.A, x, y + 1);
            border += !inside;
            const bool in_leaf = y > 0 && lm[p - w] > 0 && y < h - 1 && lm[p + w] > 0 && x > 0 && lm[p - 1] > 0 &&
                                 x < w - 1 && lm[p + 1] > 0;
            margin += !in_leaf;
        }
        const long long len = x1 - x0 + 1;
        long long* o = tab + (size_t)slot * F;
        __hip_atomic_fetch_min(o + 1, (long long)x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(o + 3, (long long)x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(o + 4, (long long)y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        add_i64(o + 5, len * (x0 + x1) / 2);
        add_i64(o + 6, len * y);
        add_i64(o + 7, sr);
        add_i64(o + 8, sg);
        add_i64(o + 9, sb);
        add_i64(o + 10, border);
        add_i64(o + 11, margin);
    }
    __threadfence();
    __syncthreads();

    const int total = s_total;
    for (int i = threadIdx.x; i < min(total, cap); i += kMaskT) {   // greatest x, y -> width, height
        long long* o = tab + (size_t)i * F;
        const long long bx = ld_i64(o + 1), by = ld_i64(o + 2), mx = ld_i64(o + 3), my = ld_i64(o + 4);
        o[3] = mx - bx + 1;
        o[4] = my - by + 1;
    }
    if (threadIdx.x == 0) {
        counts[n] = total;
        flags[n] = (total > 0 ? 1 : 0) | (total > cap ? 2 : 0) | (S.status & kFlagBound);
    }
}

}  // namespace

extern "C" {

size_t lf_lesion_table_workspace(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return BrownWs(nullptr, n, h, w).bytes;
}

int lf_lesion_table(const uint8_t* rgb, const uint8_t* mask, int64_t* table, int32_t* counts, int32_t* flags, int n,
                    int h, int w, int cap, const lf_brown_params* prm, void* workspace, size_t ws_bytes,
                    lf_stream_t stream) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the table is written as long long");
    LF_REQUIRE(rgb && mask && table && counts && flags && prm && workspace, "lf_lesion_table: null buffer");
    LF_REQUIRE(n > 0 && h > 0 && w > 0, "lf_lesion_table: bad dims n=%d %dx%d", n, h, w);
    LF_REQUIRE(n <= 65535, "lf_lesion_table: batch too large for the grid");
    LF_REQUIRE(h <= 65535 && w <= 65535, "lf_lesion_table: image too large (%d x %d)", h, w);
    LF_REQUIRE(cap >= 1, "lf_lesion_table: cap %d below 1", cap);
    const size_t lds = post_lds_bytes(2, h, (w + 31) / 32);
    LF_REQUIRE(lds <= kMaskLdsCap,
               "lf_lesion_table: a %d x %d image needs %zu bytes of LDS for its two bit planes (limit %zu, one "
               "workgroup per image)", h, w, lds, kMaskLdsCap);
    LF_REQUIRE(prm->morph_kernel >= 1 && prm->morph_kernel <= 31,
               "lf_lesion_table: brown_morph_kernel %d outside [1, 31]", prm->morph_kernel);
    LF_REQUIRE(ws_bytes >= lf_lesion_table_workspace(n, h, w), "lf_lesion_table: workspace too small (%zu < %zu)",
               ws_bytes, lf_lesion_table_workspace(n, h, w));
    LF_REQUIRE((reinterpret_cast<size_t>(workspace) & 255) == 0, "lf_lesion_table: workspace must be 256-byte aligned");
    LF_REQUIRE(lds <= dynamic_lds_cap<lesion_table_kernel>(kMaskLdsCap, 48 * 1024),
               "lf_lesion_table: could not raise the LDS limit of the lesion kernel");

    hipStream_t s = lf::as_stream(stream);
    const BrownWs ws(workspace, n, h, w);
    const MaskArgs a = brown_args(prm);
    const int rc = upload_lab_tables(ws.lb.tabs, s, "lf_lesion_table");
    if (rc != LF_OK) return rc;
    lesion_table_kernel<<<n, kMaskT, lds, s>>>(rgb, mask, ws.lb.tabs, ws.lb.rn, ws.lb.parent, ws.lb.area,
                                               (int)mask_runs_per_image(h, w), h, w, (w + 31) / 32, a,
                                               reinterpret_cast<long long*>(table), counts, flags, cap);
    return lf::check_launch("lf_lesion_table");
}

}  // extern "C"

// ===========================================================================
// apply_roi_filter (srcs/transform/filters/roi.py) for a batch, from the contour buffer make_mask_u8 leaves on the
// device: one workgroup per image.  PARITY UNPINNED (no cv2 here); the readings:
//  * bbox = cv2.boundingRect of the contour points: x = min, w = max - min + 1, the same for y.  No contour (count
//    0): vis is the input, no canvas, no bbox (bit 0 of flags clear).  Points outside the image or counts > cap set
//    bit 2 (an error; nothing but the copy is written).
//  * letterbox: scale = min(W / max(w, 1), H / max(h, 1)) in double, nw = max(int(w * scale), 1) (truncated), the
//    same for nh; cv2.resize(crop, (nw, nh), INTER_AREA) pasted on a zero canvas at ((H - nh) // 2, (W - nw) // 2).
//  * INTER_AREA as OpenCV 4's resize.cpp reads with inv_scale = dst / src and scale = 1 / inv_scale (double):
//    - equal sizes: a copy;
//    - both scales >= 1, both within DBL_EPSILON of integers kx, ky: resizeAreaFast, the integer sum of the kx x ky
//      block times (float)(1 / (kx * ky)), rounded with cvRound (half to even).  READING: this is the scalar loop;
//      the SIMD 2 x 2 kernel (ResizeAreaFastVec_SIMD_8u) rounds (sum + 2) >> 2, half up, for the pixels it covers,
//      so a tie may come out one higher there;
//    - both scales >= 1 otherwise: resizeArea with the computeResizeAreaTab weights (double positions, float
//      weights), each source row's taps accumulated in float in table order, the rows weighted and summed in
//      float in table order, cvRound;
//    - otherwise INTER_LINEAR with area-mode coefficients: sx = floor(dx * scale), fx = (float)((dx + 1) - (sx + 1)
//      * inv_scale), fx = fx <= 0 ? 0 : fx - floor(fx); sx < 0 -> (0, 0); sx >= src - 1 -> (src - 1, 0); Q11 weights
//      cvRound((1 - fx) * 2048), cvRound(fx * 2048); rows sy, sy + 1 clamped into the image, no clamp of fy.
//      READING: the scalar vertical pass (b0 * S0 + b1 * S1 + (1 << 21)) >> 22; the SIMD VResizeLinearVec_32s8u
//      ((S >> 4) * b >> 16 ... + 2) >> 2 can differ from it by 1.
//  * vis: cv2.rectangle(vis, (x, y), (x + w, y + h), (255, 0, 0), 2), LINE_8, clipped to the image.  drawing.cpp:
//    PolyLine closes the four corners into four ThickLine calls; thickness 2 is even, so each segment is
//    FillConvexPoly of the segment offset by +-1 pixel across it (XY_SHIFT fixed point, exact for whole pixels):
//    rows y - 1 .. y + 1 over x .. x + w for a horizontal side, columns x - 1 .. x + 1 over y .. y + h for a
//    vertical one; the round join at each end is Circle(radius 1, filled), a plus sign, already inside the bands.
//    The four outer corner pixels (x - 1, y - 1) etc. are therefore not drawn.
// ===========================================================================
namespace {

constexpr int kRoiT = 256;
constexpr int kRoiFound = 1, kRoiBad = 4;

// computeResizeAreaTab for destination index d, as a range: [an optional partial tap s1 - 1] full taps s1 .. s2 - 1
// [an optional partial tap s2], in table order
struct AreaAxis {
    int s1, s2, pre, post;
    float a_pre, a_mid, a_post;
    __device__ int taps() const { return pre + (s2 - s1) + post; }
    __device__ void tap(int k, int& s, float& a) const {
        if (pre && k == 0) {
            s = s1 - 1;
            a = a_pre;
            return;
        }
        k -= pre;
        if (k < s2 - s1) {
            s = s1 + k;
            a = a_mid;
        } else {
            s = s2;
            a = a_post;
        }
    }
};

__device__ AreaAxis area_axis(int ssize, double scale, int d) {
    const double f1 = __dmul_rn((double)d, scale), f2 = __dadd_rn(f1, scale);
    const double cell = fmin(scale, __dsub_rn((double)ssize, f1));
    AreaAxis t;
    t.s2 = min((int)floor(f2), ssize - 1);
    t.s1 = min((int)ceil(f1), t.s2);
    t.pre = __dsub_rn((double)t.s1, f1) > 1e-3;
    t.post = __dsub_rn(f2, (double)t.s2) > 1e-3;
    t.a_pre = (float)__ddiv_rn(__dsub_rn((double)t.s1, f1), cell);
    t.a_mid = (float)__ddiv_rn(1.0, cell);
    t.a_post = (float)__ddiv_rn(fmin(fmin(__dsub_rn(f2, (double)t.s2), 1.0), cell), cell);
    return t;
}

// area-mode INTER_LINEAR coordinate: source index, Q11 weights of it and of the next one
__device__ __forceinline__ void area_linear(int ssize, double scale, double inv, int d, bool clamp_end, int& s, int& w0,
                                            int& w1) {
    s = (int)floor(__dmul_rn((double)d, scale));
    float f = (float)__dsub_rn((double)(d + 1), __dmul_rn((double)(s + 1), inv));
    f = f <= 0.f ? 0.f : f - floorf(f);
    if (s < 0) s = 0, f = 0.f;
    if (clamp_end && s >= ssize - 1) s = ssize - 1, f = 0.f;
    w0 = (int)rintf((1.f - f) * 2048.f);
    w1 = (int)rintf(f * 2048.f);
}

__global__ __launch_bounds__(kRoiT) void roi_kernel(const uint8_t* __restrict__ rgb, const int* __restrict__ contour,
                                                    const int* __restrict__ counts, int cap, int h, int w, int rh,
                                                    int rw, uint8_t* __restrict__ canvas, uint8_t* __restrict__ vis,
                                                    int* __restrict__ bbox, int* __restrict__ flags) {
    __shared__ ContourBox B;
    const size_t n = blockIdx.x;
    const int m = contour_bbox<kRoiT>(B, contour + n * (size_t)cap * 2, counts[n], cap, h, w);
    const int *s_lo = B.lo, *s_hi = B.hi, s_bad = B.bad;
    const uint8_t* img = rgb + n * (size_t)h * w * 3;
    const bool found = m > 0 && !s_bad;
    const int bx = found ? s_lo[0] : 0, by = found ? s_lo[1] : 0;
    const int bw = found ? s_hi[0] - s_lo[0] + 1 : 1, bh = found ? s_hi[1] - s_lo[1] + 1 : 1;
    const int x1 = bx + bw, y1 = by + bh;

    uint8_t* v = vis + n * (size_t)h * w * 3;
    for (int p = threadIdx.x; p < h * w; p += kRoiT) {
        const int y = p / w, x = p - y * w;
        const bool edge = found && ((((y >= by - 1 && y <= by + 1) || (y >= y1 - 1 && y <= y1 + 1)) && x >= bx && x <= x1) ||
                                    (((x >= bx - 1 && x <= bx + 1) || (x >= x1 - 1 && x <= x1 + 1)) && y >= by && y <= y1));
        v[3 * p] = edge ? 255 : img[3 * p];
        v[3 * p + 1] = edge ? 0 : img[3 * p + 1];
        v[3 * p + 2] = edge ? 0 : img[3 * p + 2];
    }
    uint8_t* c = canvas + n * (size_t)rh * rw * 3;
    if (!found) {
        for (int p = threadIdx.x; p < rh * rw * 3; p += kRoiT) c[p] = 0;
        if (threadIdx.x == 0) {
            bbox[4 * n] = bbox[4 * n + 1] = bbox[4 * n + 2] = bbox[4 * n + 3] = 0;
            flags[n] = s_bad ? kRoiBad : 0;
        }
        return;
    }
    const double scale = fmin(__ddiv_rn((double)rw, (double)bw), __ddiv_rn((double)rh, (double)bh));
    const int nw = min(max((int)__dmul_rn((double)bw, scale), 1), rw), nh = min(max((int)__dmul_rn((double)bh, scale), 1), rh);
    const int oy = (rh - nh) / 2, ox = (rw - nw) / 2;
    const double ix = __ddiv_rn((double)nw, (double)bw), iy = __ddiv_rn((double)nh, (double)bh);
    const double sx = __ddiv_rn(1.0, ix), sy = __ddiv_rn(1.0, iy);
    const bool copy = nw == bw && nh == bh;
    const bool area = sx >= 1.0 && sy >= 1.0;
    const int kx = (int)rint(sx), ky = (int)rint(sy);
    const bool fast = area && fabs(sx - kx) < DBL_EPSILON && fabs(sy - ky) < DBL_EPSILON;
    auto src = [&](int yy, int xx, int ch) -> int {   // the crop, indices clamped into it
        yy = clampi(yy, 0, bh - 1);
        xx = clampi(xx, 0, bw - 1);
        return img[((size_t)(by + yy) * w + bx + xx) * 3 + ch];
    };
    for (int p = threadIdx.x; p < rh * rw; p += kRoiT) {
        const int y = p / rw, x = p - y * rw, dy = y - oy, dx = x - ox;
        uint8_t* o = c + (size_t)p * 3;
        if (dy < 0 || dy >= nh || dx < 0 || dx >= nw) {
            o[0] = o[1] = o[2] = 0;
            continue;
        }
        if (copy) {
            for (int ch = 0; ch < 3; ++ch) o[ch] = (uint8_t)src(dy, dx, ch);
        } else if (fast) {
            const float inv_area = __fdiv_rn(1.f, (float)(kx * ky));
            for (int ch = 0; ch < 3; ++ch) {
                int sum = 0;
                for (int r = 0; r < ky; ++r)
                    for (int q = 0; q < kx; ++q) sum += src(dy * ky + r, dx * kx + q, ch);
                o[ch] = (uint8_t)clampi((int)rintf(__fmul_rn((float)sum, inv_area)), 0, 255);
            }
        } else if (area) {
            const AreaAxis ax = area_axis(bw, sx, dx), ay = area_axis(bh, sy, dy);
            const int nx = ax.taps(), ny = ay.taps();
            for (int ch = 0; ch < 3; ++ch) {
                float sum = 0.f;
                for (int j = 0; j < ny; ++j) {
                    int ys, xs;
                    float beta, alpha, buf = 0.f;
                    ay.tap(j, ys, beta);
                    for (int k = 0; k < nx; ++k) {
                        ax.tap(k, xs, alpha);
                        buf = __fadd_rn(buf, __fmul_rn((float)src(ys, xs, ch), alpha));
                    }
                    sum = j == 0 ? __fmul_rn(beta, buf) : __fadd_rn(sum, __fmul_rn(beta, buf));
                }
                o[ch] = (uint8_t)clampi((int)rintf(sum), 0, 255);
            }
        } else {
            int xs, a0, a1, ys, b0, b1;
            area_linear(bw, sx, ix, dx, true, xs, a0, a1);
            area_linear(bh, sy, iy, dy, false, ys, b0, b1);
            for (int ch = 0; ch < 3; ++ch) {
                const int r0 = src(ys, xs, ch) * a0 + src(ys, xs + 1, ch) * a1;
                const int r1 = src(ys + 1, xs, ch) * a0 + src(ys + 1, xs + 1, ch) * a1;
                o[ch] = (uint8_t)clampi((r0 * b0 + r1 * b1 + (1 << 21)) >> 22, 0, 255);
            }
        }
    }
    if (threadIdx.x == 0) {
        bbox[4 * n] = bx;
        bbox[4 * n + 1] = by;
        bbox[4 * n + 2] = bw;
        bbox[4 * n + 3] = bh;
        flags[n] = kRoiFound;
    }
}

}  // namespace

extern "C" {

int lf_roi_u8(const uint8_t* rgb, const int32_t* contour, const int32_t* counts, int cap, uint8_t* canvas,
              uint8_t* vis, int32_t* bbox, int32_t* flags, int n, int h, int w, int roi_h, int roi_w,
              lf_stream_t stream) {
    LF_REQUIRE(rgb && contour && counts && canvas && vis && bbox && flags, "lf_roi: null buffer");
    LF_REQUIRE(n > 0 && h > 0 && w > 0 && cap > 0 && roi_h > 0 && roi_w > 0,
               "lf_roi: bad dims n=%d %dx%d cap=%d roi %dx%d", n, h, w, cap, roi_h, roi_w);
    LF_REQUIRE(n <= 65535, "lf_roi: batch too large for the grid");
    roi_kernel<<<n, kRoiT, 0, lf::as_stream(stream)>>>(rgb, contour, counts, cap, h, w, roi_h, roi_w, canvas, vis,
                                                       bbox, flags);
    return lf::check_launch("lf_roi");
}

}  // extern "C"

// ===========================================================================
// lf_shape_stats: the numbers behind srcs/transform/filters/analyze.py (centroid, extreme points, convex hull, PCA
// axes) and the ones pcv.analyze_object computes there and drops (area, hull area, solidity, perimeter), from the
// contour buffer alone: one workgroup per image, no pixel is read.  The definitions are in include/leafhip.h.
//  * Bounds: h, w <= 4096 and cap <= 65536, so |c_i| < 2^25, |(x_i + x_{i+1}) c_i| < 2^38 and every sum over the
//    points is below 2^54: int64 holds them all, and m * sxx - sx^2 (< 2^57) as well.
//  * Determinism: the integer sums may be added in any order; the one float64 sum (the perimeter) and the
//    projection extremes go thread-strided, then down a fixed shuffle tree, then over the waves in order.
//  * Hull: only the lowest and the highest point of a column can be a vertex of the strict hull, and the columns
//    come sorted by x.  Andrew's chain over (x, min y) left to right and over (x, max y) right to left, popping
//    while the cross product is <= 0, is Andrew's chain over the sorted point set: the other point of a column
//    would be pushed and popped again by the next column without touching what lies below it.  Each chain is one
//    lane's walk over LDS; its stack overwrites the column entries it has already read (a stack never holds more
//    than the columns consumed).  Repeated and touching points are nothing special: the column table is a set.
//  * Cost: the two chains are serial walks of one lane each over the bounding box's columns while the rest of the
//    workgroup waits, and the Feret pass is hull_n^2 / 512 distance tests per thread.  Measured only at 256 x 256
//    leaf scenes (boxes about 200 columns wide, 41 hull vertices: 0.1 ms per 1,024 images).  A box near 4,096
//    columns has not been measured; its walks are 20 times longer and would want the chains split over lanes.
// ===========================================================================
namespace {

constexpr int kShapeT = 256;
constexpr int kShapeMaxDim = 4096, kShapeMaxCap = 65536;
constexpr int kShapeInts = 32, kShapeVals = 16;

__device__ __forceinline__ long long wave_sum(long long v) {
    for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// (value, index) of the least (MAX: greatest) value over the wave, the lower index on a tie
template <bool MAX>
__device__ __forceinline__ void wave_arg(double& v, int& i) {
    for (int off = 32; off; off >>= 1) {
        const double ov = __shfl_down(v, off);
        const int oi = __shfl_down(i, off);
        if ((MAX ? ov > v : ov < v) || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

__device__ __forceinline__ int hull_pack(int x, int y) { return (x << 16) | y; }
__device__ __forceinline__ int hull_cross(int a, int b, int x, int y) {   // (b - a) x (p - a), |.| < 2^25
    const int ax = a >> 16, ay = a & 0xffff;
    return ((b >> 16) - ax) * (y - ay) - ((b & 0xffff) - ay) * (x - ax);
}

__global__ __launch_bounds__(kShapeT) void shape_stats_kernel(const int* __restrict__ contour,
                                                              const int* __restrict__ counts, int cap, int h, int w,
                                                              long long* __restrict__ ints, double* __restrict__ vals,
                                                              int* __restrict__ hull, int* __restrict__ flags) {
    __shared__ ContourBox B;
    __shared__ int s_col[2][kShapeMaxDim];          // per column: min y | max y, then the two chain stacks
    __shared__ unsigned long long s_sum[8];
    __shared__ unsigned s_ext[4];
    __shared__ double s_wv[kShapeT / 64][4];
    __shared__ int s_wi[kShapeT / 64][4];
    __shared__ double s_per[kShapeT / 64], s_axis[2];
    __shared__ int s_hn[4], s_over;                  // lower count, upper start, upper count, hull count
    __shared__ unsigned long long s_feret;
    __shared__ long long s_ha2;
    const size_t n = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int* pts = contour + n * (size_t)cap * 2;
    const int hcap = 2 * min(h, w);
    long long* oi = ints + n * kShapeInts;
    double* ov = vals + n * kShapeVals;
    int* oh = hull + n * (size_t)hcap * 2;
    const int m = contour_bbox<kShapeT>(B, pts, counts[n], cap, h, w);
    if (m == 0 || B.bad) {
        for (int i = tid; i < kShapeInts; i += kShapeT) oi[i] = 0;
        for (int i = tid; i < kShapeVals; i += kShapeT) ov[i] = 0.0;
        for (int i = tid; i < 2 * hcap; i += kShapeT) oh[i] = 0;
        if (tid == 0) flags[n] = B.bad ? kRoiBad : 0;
        return;
    }
    const int bx = B.lo[0], by = B.lo[1], bw = B.hi[0] - bx + 1, bh = B.hi[1] - by + 1;
    for (int i = tid; i < bw; i += kShapeT) {
        s_col[0][i] = INT_MAX;
        s_col[1][i] = -1;
    }
    if (tid < 8) s_sum[tid] = 0ull;
    if (tid < 4) s_ext[tid] = (tid & 1) ? 0u : 0xffffffffu;
    if (tid == 0) s_feret = 0ull;
    __syncthreads();

    // ---- the sums over the points, the first extreme points, the column table
    long long a2 = 0, s10 = 0, s01 = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
    double per = 0.0;
    unsigned e_l = 0xffffffffu, e_r = 0u, e_t = 0xffffffffu, e_b = 0u;
    for (int i = tid; i < m; i += kShapeT) {
        const int j = i + 1 < m ? i + 1 : 0;
        const int x = pts[2 * i], y = pts[2 * i + 1], xn = pts[2 * j], yn = pts[2 * j + 1];
        const long long c = shoelace_term(x, y, xn, yn);
        a2 += c;
        s10 += (x + xn) * c;
        s01 += (y + yn) * c;
        sx += x;
        sy += y;
        sxx += x * x;
        sxy += x * y;
        syy += y * y;
        const int dx = xn - x, dy = yn - y;
        per = __dadd_rn(per, __dsqrt_rn((double)(dx * dx + dy * dy)));
        const unsigned fwd = (unsigned)i, rev = (unsigned)(kShapeMaxCap - 1 - i);   // the first index wins
        e_l = min(e_l, ((unsigned)x << 16) | fwd);
        e_r = max(e_r, ((unsigned)x << 16) | rev);
        e_t = min(e_t, ((unsigned)y << 16) | fwd);
        e_b = max(e_b, ((unsigned)y << 16) | rev);
        atomicMin(&s_col[0][x - bx], y);
        atomicMax(&s_col[1][x - bx], y);
    }
    atomicMin(&s_ext[0], e_l);
    atomicMax(&s_ext[1], e_r);
    atomicMin(&s_ext[2], e_t);
    atomicMax(&s_ext[3], e_b);
    const long long part[8] = {a2, s10, s01, sx, sy, sxx, sxy, syy};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long long t = wave_sum(part[k]);
        if (lane == 0) atomicAdd(&s_sum[k], (unsigned long long)t);
    }
    for (int off = 32; off; off >>= 1) per = __dadd_rn(per, __shfl_down(per, off));
    if (lane == 0) s_per[wv] = per;
    __syncthreads();

    // ---- the axes: eigenvectors of [[A, Bc], [Bc, C]] / m^2, A = m sxx - sx^2 and so on, exact in int64
    if (tid == 0) {
        const long long SX = (long long)s_sum[3], SY = (long long)s_sum[4];
        const long long A = m * (long long)s_sum[5] - SX * SX, Bc = m * (long long)s_sum[6] - SX * SY,
                        C = m * (long long)s_sum[7] - SY * SY;
        double vx = 1.0, vy = 0.0;
        if (A != C || Bc != 0) {
            const double d = __dmul_rn(0.5, (double)(A - C)), b = (double)Bc;
            const double r = __dsqrt_rn(__dadd_rn(__dmul_rn(d, d), __dmul_rn(b, b)));
            // (r + d, b) and (b, r - d) are both eigenvectors of the greater eigenvalue: the one without cancellation
            vx = d >= 0.0 ? __dadd_rn(r, d) : b;
            vy = d >= 0.0 ? b : __dsub_rn(r, d);
            const double len = __dsqrt_rn(__dadd_rn(__dmul_rn(vx, vx), __dmul_rn(vy, vy)));
            vx = __ddiv_rn(vx, len);
            vy = __ddiv_rn(vy, len);
            if (vx < 0.0 || (vx == 0.0 && vy < 0.0)) {
                vx = -vx;
                vy = -vy;
            }
        }
        s_axis[0] = vx;
        s_axis[1] = vy;
    }
    // ---- the hull chains, one lane each, while the other waves wait at the barrier
    if (tid == 0) {   // (x, min y), left to right; the stack grows from s_col[0][0]
        int* S = s_col[0];
        int sp = 0;
        for (int k = 0; k < bw; ++k) {
            const int y = S[k];
            if (y == INT_MAX) continue;
            while (sp >= 2 && hull_cross(S[sp - 2], S[sp - 1], bx + k, y) <= 0) --sp;
            S[sp++] = hull_pack(bx + k, y);
        }
        s_hn[0] = sp;
    }
    if (tid == 64) {   // (x, max y), right to left; the stack grows down from s_col[1][bw - 1]
        int* S = s_col[1];
        int sp = 0;
        for (int k = bw - 1; k >= 0; --k) {
            const int y = S[k];
            if (y < 0) continue;
            while (sp >= 2 && hull_cross(S[bw - sp + 1], S[bw - sp], bx + k, y) <= 0) --sp;
            S[bw - 1 - sp++] = hull_pack(bx + k, y);
        }
        s_hn[2] = sp;
    }
    __syncthreads();
    if (tid == 0) {   // join: a chain's last point may be the other's first
        const int nl = s_hn[0], nu = s_hn[2];
        int us = 0, un = nu;
        if (s_col[0][nl - 1] == s_col[1][bw - 1]) us = 1, --un;
        if (un > 0 && s_col[1][bw - nu] == s_col[0][0]) --un;
        s_hn[1] = us;
        s_hn[2] = un;
        // nl + un <= hcap for any point set (two vertices per row and per column at most).  Defence only, against a
        // store past the hull buffer should the chains ever be wrong: the count is cut and the image flagged bad.
        s_hn[3] = min(nl + un, hcap);
        s_over = nl + un > hcap;
        s_ha2 = 0;
    }
    __syncthreads();
    const int nl = s_hn[0], us = s_hn[1], hn = s_hn[3];
    auto hull_at = [&](int k) -> int { return k < nl ? s_col[0][k] : s_col[1][bw - 1 - (k - nl + us)]; };

    // ---- projection extremes, hull area, Feret diameter, the hull itself
    const double vx = s_axis[0], vy = s_axis[1];
    double p0lo = INFINITY, p0hi = -INFINITY, p1lo = INFINITY, p1hi = -INFINITY;
    int i0lo = INT_MAX, i0hi = INT_MAX, i1lo = INT_MAX, i1hi = INT_MAX;
    for (int i = tid; i < m; i += kShapeT) {
        const double x = (double)pts[2 * i], y = (double)pts[2 * i + 1];
        const double p0 = __dadd_rn(__dmul_rn(x, vx), __dmul_rn(y, vy));
        const double p1 = __dsub_rn(__dmul_rn(y, vx), __dmul_rn(x, vy));
        if (p0 < p0lo) p0lo = p0, i0lo = i;
        if (p0 > p0hi) p0hi = p0, i0hi = i;
        if (p1 < p1lo) p1lo = p1, i1lo = i;
        if (p1 > p1hi) p1hi = p1, i1hi = i;
    }
    wave_arg<false>(p0lo, i0lo);
    wave_arg<true>(p0hi, i0hi);
    wave_arg<false>(p1lo, i1lo);
    wave_arg<true>(p1hi, i1hi);
    if (lane == 0) {
        s_wv[wv][0] = p0lo, s_wv[wv][1] = p0hi, s_wv[wv][2] = p1lo, s_wv[wv][3] = p1hi;
        s_wi[wv][0] = i0lo, s_wi[wv][1] = i0hi, s_wi[wv][2] = i1lo, s_wi[wv][3] = i1hi;
    }
    long long ha2 = 0;
    unsigned long long far = 0ull;
    for (int k = tid; k < hn; k += kShapeT) {
        const int a = hull_at(k), b = hull_at(k + 1 < hn ? k + 1 : 0);
        const int ax = a >> 16, ay = a & 0xffff;
        ha2 += shoelace_term(ax, ay, b >> 16, b & 0xffff);
        for (int q = k + 1; q < hn; ++q) {
            const int c = hull_at(q);
            const long long dx = (c >> 16) - ax, dy = (c & 0xffff) - ay;
            far = max(far, (unsigned long long)(dx * dx + dy * dy));
        }
        oh[2 * k] = ax;
        oh[2 * k + 1] = ay;
    }
    for (int i = 2 * hn + tid; i < 2 * hcap; i += kShapeT) oh[i] = 0;
    ha2 = wave_sum(ha2);
    if (lane == 0) atomicAdd((unsigned long long*)&s_ha2, (unsigned long long)ha2);
    atomicMax(&s_feret, far);
    __syncthreads();

    if (tid == 0) {
        for (int q = 0; q < 4; ++q) {   // over the waves in order; the lower index on a tie
            double v = s_wv[0][q];
            int ix = s_wi[0][q];
            for (int k = 1; k < kShapeT / 64; ++k) {
                const double o = s_wv[k][q];
                if (((q & 1) ? o > v : o < v) || (o == v && s_wi[k][q] < ix)) v = o, ix = s_wi[k][q];
            }
            s_wv[0][q] = v;
            s_wi[0][q] = ix;
        }
        double perim = s_per[0];
        for (int k = 1; k < kShapeT / 64; ++k) perim = __dadd_rn(perim, s_per[k]);
        const long long A2 = (long long)s_sum[0], S10 = (long long)s_sum[1], S01 = (long long)s_sum[2];
        const long long SX = (long long)s_sum[3], SY = (long long)s_sum[4], SXX = (long long)s_sum[5],
                        SXY = (long long)s_sum[6], SYY = (long long)s_sum[7];
        const long long HA2 = s_ha2 < 0 ? -s_ha2 : s_ha2, F2 = (long long)s_feret;
        const int il = s_ext[0] & 0xffff, ir = kShapeMaxCap - 1 - (s_ext[1] & 0xffff), it = s_ext[2] & 0xffff,
                  ib = kShapeMaxCap - 1 - (s_ext[3] & 0xffff);
        const long long rec[29] = {m, A2, S10, S01, bx, by, bw, bh,
                                   pts[2 * il], pts[2 * il + 1], pts[2 * ir], pts[2 * ir + 1],
                                   pts[2 * it], pts[2 * it + 1], pts[2 * ib], pts[2 * ib + 1],
                                   bx > 0 && by > 0 && bx + bw < w && by + bh < h,
                                   SX, SY, SXX, SXY, SYY, hn, HA2, F2,
                                   s_wi[0][0], s_wi[0][1], s_wi[0][2], s_wi[0][3]};
#pragma unroll
        for (int k = 0; k < kShapeInts; ++k) oi[k] = k < 29 ? rec[k] : 0;

        const double area = __dmul_rn(0.5, (double)(A2 < 0 ? -A2 : A2)), harea = __dmul_rn(0.5, (double)HA2);
        const double md = (double)m;
        const double cx = A2 ? __ddiv_rn((double)S10, (double)(3 * A2)) : __ddiv_rn((double)SX, md);
        const double cy = A2 ? __ddiv_rn((double)S01, (double)(3 * A2)) : __ddiv_rn((double)SY, md);
        const long long A = m * SXX - SX * SX, Bc = m * SXY - SX * SY, C = m * SYY - SY * SY;
        const double mean = __dmul_rn(0.5, (double)(A + C)), d = __dmul_rn(0.5, (double)(A - C)), b = (double)Bc;
        const double r = __dsqrt_rn(__dadd_rn(__dmul_rn(d, d), __dmul_rn(b, b))), m2 = __dmul_rn(md, md);
        const double pi = 3.141592653589793;
        ov[0] = area;
        ov[1] = perim;
        ov[2] = cx;
        ov[3] = cy;
        ov[4] = harea;
        ov[5] = HA2 ? __ddiv_rn(area, harea) : 0.0;
        ov[6] = perim > 0.0 ? __ddiv_rn(__dmul_rn(__dmul_rn(4.0, pi), area), __dmul_rn(perim, perim)) : 0.0;
        ov[7] = __dsqrt_rn((double)F2);
        ov[8] = __ddiv_rn(__dadd_rn(mean, r), m2);
        ov[9] = fmax(__ddiv_rn(__dsub_rn(mean, r), m2), 0.0);
        ov[10] = vx;
        ov[11] = vy;
        ov[12] = __dsub_rn(s_wv[0][1], s_wv[0][0]);
        ov[13] = __dsub_rn(s_wv[0][3], s_wv[0][2]);
        ov[14] = __ddiv_rn(__dmul_rn(atan2(vy, vx), 180.0), pi);
        ov[15] = 0.0;
        flags[n] = kRoiFound | (s_over ? kRoiBad : 0);
    }
}

}  // namespace

extern "C" {

int lf_shape_stats(const int32_t* contour, const int32_t* counts, int cap, int64_t* ints, double* vals,
                   int32_t* hull, int32_t* flags, int n, int h, int w, lf_stream_t stream) {
    LF_REQUIRE(contour && counts && ints && vals && hull && flags, "lf_shape_stats: null buffer");
    LF_REQUIRE(n > 0 && h > 0 && w > 0 && cap > 0, "lf_shape_stats: bad dims n=%d %dx%d cap=%d", n, h, w, cap);
    LF_REQUIRE(n <= 65535, "lf_shape_stats: batch too large for the grid");
    LF_REQUIRE(h <= kShapeMaxDim && w <= kShapeMaxDim && cap <= kShapeMaxCap,
               "lf_shape_stats: %d x %d with cap %d is over the limits (h, w <= %d, cap <= %d) that keep every sum "
               "inside int64", h, w, cap, kShapeMaxDim, kShapeMaxCap);
    static_assert(sizeof(long long) == sizeof(int64_t), "the integer record is int64");
    shape_stats_kernel<<<n, kShapeT, 0, lf::as_stream(stream)>>>(contour, counts, cap, h, w,
                                                                 reinterpret_cast<long long*>(ints), vals, hull, flags);
    return lf::check_launch("lf_shape_stats");
}

}  // extern "C"


// ===========================================================================
// lf_analyze_overlay_u8: the picture srcs/transform/filters/analyze.py returns, drawn from make_mask's contour,
// lf_shape_stats' records and the Canny edges by the project's own integer drawing rules (include/leafhip.h,
// "Drawing rules"; tests/draw_ref.py is the same reading in numpy).  Three launches on one stream: a copy of the
// input, one workgroup per image for the primitives, a pass over the pixels for the cyan edges.
//  * A segment's pixels: the walk goes along the major axis over [min - 1, max + 1] (the caps of a thick segment
//    reach one pixel past its ends), and at each step tests the five pixels centre - 2 .. centre + 2 across it,
//    centre = floor of the line there.  A pixel within distance 1 of a line whose slope is at most 1 lies within
//    sqrt(2) of it across the minor axis, so within floor - 1 .. floor + 2; the exact integer tests of the rules
//    decide.  A (step, pixel) pair belongs to one thread, so a segment blends each pixel it touches exactly once.
//  * Order: overwrites of one colour may race (every writer stores the same bytes); everything else is separated
//    by a barrier: the contour | the marker | disc, ray, four times | the hull's segments one after another | the
//    two axes one after the other.  __syncthreads orders the workgroup's stores to `out` before its later loads.
//  * Safety: the contour is validated as lf_roi_u8 validates it (a bad one leaves the copy untouched); the records
//    are not trusted: coordinates are clamped to +-16384 (which also keeps c^2 below 2^62), the hull count to its
//    capacity, the axis indices into [0, m); a pixel is stored only after the test against the image's bounds.
//  * Cost: the hull's anti-aliased segments (about 40 of about 20 pixels on a 256 x 256 leaf) run one after another
//    with 256 threads on each, most of them idle.
// ===========================================================================
namespace {

constexpr int kDrawT = 256;
constexpr int kDrawClamp = 16384;
constexpr unsigned kRed = 0x0000ffu, kYellow = 0x00ffffu, kGreen = 0x00ff00u, kMagenta = 0xff00ffu;   // r | g << 8 | b << 16

__device__ __forceinline__ int draw_coord(long long v) {
    return (int)(v < -kDrawClamp ? -kDrawClamp : (v > kDrawClamp - 1 ? kDrawClamp - 1 : v));
}
__device__ __forceinline__ int draw_coord(double v) {   // truncated; NaN goes to the lower bound
    return v >= (double)-kDrawClamp ? (v <= (double)(kDrawClamp - 1) ? (int)v : kDrawClamp - 1) : -kDrawClamp;
}

// floor_div, seg_walk, put_px and draw_thick (the thick segment: every pixel within distance 1) are stated in lf_draw.h,
// which lf_hist_figure_u8 shares
using lf::draw_thick;
using lf::floor_div;
using lf::put_px;
using lf::seg_walk;

// thickness 1, anti-aliased: 0 <= u <= L2 and c^2 < L2, blended with a = 256 - isqrt(65536 c^2 / L2)
__device__ __forceinline__ void draw_aa(uint8_t* img, int h, int w, int ax, int ay, int bx, int by, unsigned k,
                                        int t0, int stride) {
    seg_walk(ax, ay, bx, by, h, w, t0, stride, [&](int x, int y, long long u, long long c, long long L2) {
        const long long c2 = c * c;
        if (L2 == 0 ? (x != ax || y != ay) : (u < 0 || u > L2 || c2 >= L2)) return;
        int s = 0;
        if (L2) {
            const int v = (int)((65536 * c2) / L2);   // below 65536
            s = (int)sqrtf((float)v);
            while (s * s > v) --s;
            while ((s + 1) * (s + 1) <= v) ++s;
        }
        const int a = 256 - s;
        uint8_t* o = img + ((size_t)y * w + x) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            o[ch] = (uint8_t)((a * (int)((k >> (8 * ch)) & 255u) + (256 - a) * (int)o[ch] + 128) >> 8);
    });
}

__global__ __launch_bounds__(kDrawT) void analyze_draw_kernel(const int* __restrict__ contour,
                                                              const int* __restrict__ counts, int cap,
                                                              const long long* __restrict__ ints,
                                                              const double* __restrict__ vals,
                                                              const int* __restrict__ hull, int h, int w,
                                                              uint8_t* out, int* __restrict__ flags) {
    __shared__ ContourBox B;
    const size_t n = blockIdx.x;
    const int tid = threadIdx.x;
    const int* pts = contour + n * (size_t)cap * 2;
    const int m = contour_bbox<kDrawT>(B, pts, counts[n], cap, h, w);
    const bool found = m > 0 && !B.bad;
    if (tid == 0) flags[n] = found ? kRoiFound : (B.bad ? kRoiBad : 0);
    if (!found) return;
    uint8_t* img = out + n * (size_t)h * w * 3;
    const long long* rec = ints + n * kShapeInts;
    const int hcap = 2 * min(h, w);
    const int* hv = hull + n * (size_t)hcap * 2;

    // 1: the contour, a closed polyline of thick segments, a segment per thread
    for (int i = tid; i < m; i += kDrawT) {
        const int j = i + 1 < m ? i + 1 : 0;
        draw_thick(img, h, w, pts[2 * i], pts[2 * i + 1], pts[2 * j], pts[2 * j + 1], kRed, 0, 1);
    }
    __syncthreads();
    // 2: the centroid marker
    const int cx = draw_coord(vals[n * kShapeVals + 2]), cy = draw_coord(vals[n * kShapeVals + 3]);
    draw_thick(img, h, w, cx - 7, cy, cx + 7, cy, kYellow, tid, kDrawT);
    draw_thick(img, h, w, cx, cy - 7, cx, cy + 7, kYellow, tid, kDrawT);
    __syncthreads();
    // 3: left, right, top, bottom: the disc, then the ray from the centroid
    for (int e = 0; e < 4; ++e) {
        const int qx = draw_coord(rec[8 + 2 * e]), qy = draw_coord(rec[9 + 2 * e]);
        if (tid < 49) {
            const int ox = tid % 7 - 3, oy = tid / 7 - 3, x = qx + ox, y = qy + oy;
            if (ox * ox + oy * oy <= 12 && x >= 0 && x < w && y >= 0 && y < h) put_px(img, w, x, y, kYellow);
        }
        __syncthreads();
        draw_aa(img, h, w, cx, cy, qx, qy, kYellow, tid, kDrawT);
        __syncthreads();
    }
    // 4: the hull, a closed anti-aliased polyline, one segment after another
    const int hn = (int)min(max(rec[22], 0ll), (long long)hcap);
    for (int i = 0; i < hn; ++i) {
        const int j = i + 1 < hn ? i + 1 : 0;
        draw_aa(img, h, w, draw_coord((long long)hv[2 * i]), draw_coord((long long)hv[2 * i + 1]),
                draw_coord((long long)hv[2 * j]), draw_coord((long long)hv[2 * j + 1]), kGreen, tid, kDrawT);
        __syncthreads();
    }
    // 5: the axes
    for (int e = 0; e < 2; ++e) {
        const int i = (int)min(max(rec[25 + 2 * e], 0ll), (long long)m - 1);
        const int j = (int)min(max(rec[26 + 2 * e], 0ll), (long long)m - 1);
        draw_thick(img, h, w, pts[2 * i], pts[2 * i + 1], pts[2 * j], pts[2 * j + 1], e ? kMagenta : kYellow, tid, kDrawT);
        __syncthreads();
    }
}

// 6: the Canny edges inside the mask, in cyan, on the images that have a contour
__global__ __launch_bounds__(kBlock) void analyze_edges_kernel(const uint8_t* __restrict__ mask,
                                                               const uint8_t* __restrict__ edges,
                                                               const int* __restrict__ flags, int hw,
                                                               uint8_t* __restrict__ out) {
    const size_t n = blockIdx.y;
    if (!(flags[n] & kRoiFound)) return;
    const uint8_t *mk = mask + n * (size_t)hw, *ed = edges + n * (size_t)hw;
    uint8_t* o = out + n * (size_t)hw * 3;
    for (int p = blockIdx.x * kBlock + threadIdx.x; p < hw; p += gridDim.x * kBlock)
        if (ed[p] && mk[p]) {
            o[3 * (size_t)p] = 0;
            o[3 * (size_t)p + 1] = 255;
            o[3 * (size_t)p + 2] = 255;
        }
}

}  // namespace

extern "C" {

int lf_analyze_overlay_u8(const uint8_t* rgb, const uint8_t* mask, const uint8_t* edges, const int32_t* contour,
                          const int32_t* counts, int cap, const int64_t* ints, const double* vals,
                          const int32_t* hull, uint8_t* out, int32_t* flags, int n, int h, int w,
                          lf_stream_t stream) {
    LF_REQUIRE(rgb && mask && edges && contour && counts && ints && vals && hull && out && flags,
               "lf_analyze_overlay: null buffer");
    LF_REQUIRE(n > 0 && h > 0 && w > 0 && cap > 0, "lf_analyze_overlay: bad dims n=%d %dx%d cap=%d", n, h, w, cap);
    LF_REQUIRE(n <= 65535, "lf_analyze_overlay: batch too large for the grid");
    LF_REQUIRE(h <= kShapeMaxDim && w <= kShapeMaxDim && cap <= kShapeMaxCap,
               "lf_analyze_overlay: %d x %d with cap %d is over lf_shape_stats' limits (h, w <= %d, cap <= %d)", h, w,
               cap, kShapeMaxDim, kShapeMaxCap);
    const size_t bytes = (size_t)n * h * w * 3;
    LF_REQUIRE(rgb + bytes <= out || out + bytes <= rgb, "lf_analyze_overlay: rgb and out overlap");
    hipStream_t s = lf::as_stream(stream);
    if (hipMemcpyAsync(out, rgb, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        lf::set_error("lf_analyze_overlay: the copy of the input failed");
        return LF_ERR_LAUNCH;
    }
    analyze_draw_kernel<<<n, kDrawT, 0, s>>>(contour, counts, cap, reinterpret_cast<const long long*>(ints), vals,
                                             hull, h, w, out, flags);
    const int hw = h * w;
    analyze_edges_kernel<<<dim3(std::min((hw + kBlock - 1) / kBlock, 64), n), kBlock, 0, s>>>(mask, edges, flags, hw,
                                                                                              out);
    return lf::check_launch("lf_analyze_overlay");
}

}  // extern "C"

// ===========================================================================
// The pixel stages of the pseudo-landmarks filter (srcs/transform/filters/landmarks.py): CLAHE, the d = 5 bilateral
// filter, the Shi-Tomasi corner score and the greedy point selection of goodFeaturesToTrack.  PARITY UNPINNED (no
// cv2): the rules are the project's own, all in integers, stated in include/leafhip.h and restated in numpy by
// tests/landmarks_ref.py; the kernels are held to them bit for bit.
// ===========================================================================
namespace {

constexpr int kClaheTiles = 8;       // per axis
constexpr int kGfT = 256;            // good_features_kernel
constexpr size_t kClaheMaxArea = (size_t)1 << 27;   // keeps 1022 * tw * th below 2^31

// p in [0, 2 * len - 2]: the image continued past its last sample by reflect-101
__device__ __forceinline__ int reflect_pad(int p, int len) { return p >= len ? 2 * len - 2 - p : p; }

// One workgroup of 256 threads per (tile, image): the tile's histogram in LDS, clipped and redistributed, its
// inclusive prefix sum, and the LUT -> luts[n][tile][256].
__global__ __launch_bounds__(kBlock) void clahe_lut_kernel(const uint8_t* __restrict__ gray,
                                                           uint8_t* __restrict__ luts, int h, int w, int tw, int th) {
    __shared__ unsigned hist[256];
    __shared__ unsigned cum[2][256];
    __shared__ unsigned excess;
    const int t = threadIdx.x, tile = blockIdx.x;
    const size_t n = blockIdx.y;
    const uint8_t* g = gray + n * (size_t)h * w;
    const int x0 = (tile % kClaheTiles) * tw, y0 = (tile / kClaheTiles) * th;
    hist[t] = 0;
    if (t == 0) excess = 0;
    __syncthreads();
    const int a = tw * th;
    for (int p = t; p < a; p += kBlock) {
        const int yy = p / tw, xx = p - yy * tw;
        atomicAdd(&hist[g[(size_t)reflect_pad(y0 + yy, h) * w + reflect_pad(x0 + xx, w)]], 1u);
    }
    __syncthreads();
    const unsigned clip = (unsigned)max(1, (2 * a) / 256);
    unsigned v = hist[t];
    if (v > clip) {
        atomicAdd(&excess, v - clip);
        v = clip;
    }
    __syncthreads();
    const unsigned ex = excess, r = ex % 256u;
    v += ex / 256u;
    if (r > 0) {
        const unsigned step = max(256u / r, 1u);
        if (t % step == 0 && t / step < r) v += 1;
    }
    cum[0][t] = v;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < 256; d <<= 1) {   // Hillis-Steele inclusive scan
        cum[cur ^ 1][t] = cum[cur][t] + (t >= d ? cum[cur][t - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    const long long l = (2LL * 255 * cum[cur][t] + a) / (2LL * a);
    luts[(n * (kClaheTiles * kClaheTiles) + tile) * 256 + t] = (uint8_t)(l > 255 ? 255 : l);
}

// fx = 2 p + 1 - t (twice the distance from the first tile's centre): the lower tile, clamped with its neighbour into
// [0, 7], and the neighbour's weight a in [0, 2 t) (the lower tile's is 2 t - a).
__device__ __forceinline__ void clahe_axis(int p, int t, int& lo, int& hi, unsigned& a) {
    const int f = 2 * p + 1 - t;
    const int i = f < 0 ? -1 : f / (2 * t);
    a = (unsigned)(f - 2 * t * i);
    lo = clampi(i, 0, kClaheTiles - 1);
    hi = clampi(i + 1, 0, kClaheTiles - 1);
}

__global__ __launch_bounds__(kBlock) void clahe_apply_kernel(const uint8_t* __restrict__ gray,
                                                             const uint8_t* __restrict__ luts,
                                                             uint8_t* __restrict__ out, int h, int w, int tw, int th) {
    const size_t n = blockIdx.y;
    const int hw = h * w;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= hw) return;
    const int y = p / w, x = p - y * w;
    int tx0, tx1, ty0, ty1;
    unsigned ax, ay;
    clahe_axis(x, tw, tx0, tx1, ax);
    clahe_axis(y, th, ty0, ty1, ay);
    const unsigned v = gray[n * hw + p];
    const uint8_t* L = luts + n * (kClaheTiles * kClaheTiles) * 256 + v;
    const unsigned bx = 2u * tw - ax, by = 2u * th - ay;
    const unsigned l00 = L[(ty0 * kClaheTiles + tx0) * 256], l01 = L[(ty0 * kClaheTiles + tx1) * 256];
    const unsigned l10 = L[(ty1 * kClaheTiles + tx0) * 256], l11 = L[(ty1 * kClaheTiles + tx1) * 256];
    const unsigned sum = (l00 * bx + l01 * ax) * by + (l10 * bx + l11 * ax) * ay;   // <= 255 * 4 tw th < 2^31
    out[n * hw + p] = (uint8_t)((sum + 2u * tw * th) / (4u * tw * th));
}

// d = 5: the 21 taps with dx^2 + dy^2 <= 4; wc / ws are Q16 tables (range by |difference|, space by squared distance)
__global__ __launch_bounds__(kBlock) void bilateral_kernel(const uint8_t* __restrict__ gray,
                                                           const int32_t* __restrict__ wc,
                                                           const int32_t* __restrict__ ws, uint8_t* __restrict__ out,
                                                           int h, int w) {
    __shared__ unsigned swc[256];
    __shared__ unsigned sws[5];
    swc[threadIdx.x] = (unsigned)wc[threadIdx.x];
    if (threadIdx.x < 5) sws[threadIdx.x] = (unsigned)ws[threadIdx.x];
    __syncthreads();
    const size_t n = blockIdx.y;
    const int hw = h * w;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= hw) return;
    const uint8_t* g = gray + n * hw;
    const int y = p / w, x = p - y * w;
    const int c = g[p];
    unsigned sw = 0, swv = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = dy < 0 ? (y + dy < 0 ? -(y + dy) : y + dy) : reflect_pad(y + dy, h);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx * dx + dy * dy > 4) continue;
            const int xx = dx < 0 ? (x + dx < 0 ? -(x + dx) : x + dx) : reflect_pad(x + dx, w);
            const int v = g[(size_t)yy * w + xx];
            const int d = v > c ? v - c : c - v;
            const unsigned wt =
                (unsigned)(((unsigned long long)sws[dx * dx + dy * dy] * swc[d] + 32768u) >> 16);   // <= 65536
            sw += wt;
            swv += wt * (unsigned)v;   // <= 21 * 65536 * 255 < 2^29
        }
    }
    out[n * hw + p] = sw ? (uint8_t)((2u * swv + sw) / (2u * sw)) : (uint8_t)c;
}

// floor(sqrt(v)) for 0 <= v < 2^52: the double root, then the integer fix-up
__device__ __forceinline__ long long isqrt_ll(long long v) {
    long long r = (long long)sqrt((double)v);
    if (r * r > v) --r;
    if ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// Shi-Tomasi, block size 3: S = A + C - isqrt((A - C)^2 + 4 B^2) over the 3 x 3 sums of the Sobel products
__global__ __launch_bounds__(kBlock) void corner_score_kernel(const uint8_t* __restrict__ gray,
                                                              int32_t* __restrict__ score, int h, int w) {
    const size_t n = blockIdx.y;
    const int hw = h * w;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= hw) return;
    const uint8_t* g = gray + n * hw;
    const int y = p / w, x = p - y * w;
    int A = 0, B = 0, C = 0;   // A, C <= 9 * 1020^2 < 2^24
    for (int j = -1; j <= 1; ++j) {
        const int yy = reflect101i(y + j, h);
        const int y0 = reflect101i(yy - 1, h), y2 = reflect101i(yy + 1, h);
        for (int i = -1; i <= 1; ++i) {
            const int xx = reflect101i(x + i, w);
            const Sob s = sobel_at(g, w, y0, yy, y2, reflect101i(xx - 1, w), xx, reflect101i(xx + 1, w));
            A += s.dx * s.dx;
            B += s.dx * s.dy;
            C += s.dy * s.dy;
        }
    }
    const long long d = (long long)A - C;
    score[n * hw + p] = (int32_t)((long long)A + C - isqrt_ll(d * d + 4LL * B * B));
}

// ---- point selection.  A candidate's key orders by score descending, then raster position ascending; 0 = dead.
__device__ __forceinline__ unsigned long long gf_key(int s, int pos) {
    return ((unsigned long long)(unsigned)s << 32) | (0xffffffffu - (unsigned)pos);
}
__device__ __forceinline__ int gf_key_pos(unsigned long long k) { return (int)(0xffffffffu - (unsigned)k); }

struct GfLds {
    int smax;
    unsigned count;
    unsigned long long best;
};

// The whole workgroup of T threads selects up to max_points points of one score plane where mask(p) holds, into
// pts (x, y); returns their number (uniform).  keys: (h - 2) * (w - 2) words of scratch.  Bounded: at most
// max_points rounds of one pass over the candidates.
template <int T, typename M>
__device__ int good_features_block(GfLds& L, const int32_t* __restrict__ sc, int h, int w, long long q_num,
                                   long long q_den, int min_dist, int max_points,
                                   unsigned long long* __restrict__ keys, int32_t* __restrict__ pts, M mask) {
    const int t = threadIdx.x, hw = h * w;
    __syncthreads();
    if (t == 0) {
        L.smax = 0;
        L.count = 0;
    }
    __syncthreads();
    int m = 0;
    for (int p = t; p < hw; p += T)
        if (mask(p)) m = max(m, sc[p]);
    if (m > 0) atomicMax(&L.smax, m);
    __syncthreads();
    const int smax = L.smax;
    if (smax <= 0 || max_points <= 0) return 0;
    const long long thr = q_num * smax;
    const int iw = w - 2, inner = (h - 2) * iw;
    for (int q = t; q < inner; q += T) {
        const int y = q / iw + 1, x = q - (y - 1) * iw + 1, p = y * w + x;
        const int s = sc[p];
        if (q_den * s <= thr || !mask(p)) continue;
        // a neighbour that is not live scores below every live pixel, so >= all eight is >= the live ones
        const int32_t *r0 = sc + p - w, *r2 = sc + p + w;
        const int nb = max(max(max(r0[-1], r0[0]), max(r0[1], sc[p - 1])),
                           max(max(sc[p + 1], r2[-1]), max(r2[0], r2[1])));
        if (s >= nb) keys[atomicAdd(&L.count, 1u)] = gf_key(s, p);
    }
    __syncthreads();
    const int cnt = (int)L.count;
    const int md2 = min_dist * min_dist;
    int taken = 0;
    for (; taken < max_points; ++taken) {
        if (t == 0) L.best = 0;
        __syncthreads();
        unsigned long long b = 0;
        for (int i = t; i < cnt; i += T) b = max(b, keys[i]);
        for (int o = 32; o; o >>= 1) b = max(b, __shfl_xor(b, o));
        if ((t & 63) == 0 && b) atomicMax(&L.best, b);
        __syncthreads();
        const unsigned long long best = L.best;
        if (!best) break;   // uniform
        const int bp = gf_key_pos(best), by = bp / w, bx = bp - by * w;
        if (t == 0) {
            pts[2 * taken] = bx;
            pts[2 * taken + 1] = by;
        }
        for (int i = t; i < cnt; i += T) {
            const unsigned long long k = keys[i];
            if (!k) continue;
            const int kp = gf_key_pos(k), ky = kp / w, kx = kp - ky * w;
            if (k == best || (kx - bx) * (kx - bx) + (ky - by) * (ky - by) < md2) keys[i] = 0;
        }
        __syncthreads();
    }
    return taken;
}

__global__ __launch_bounds__(kGfT) void good_features_kernel(const int32_t* __restrict__ score,
                                                             const uint8_t* __restrict__ mask, int h, int w,
                                                             int q_num, int q_den, int min_dist, int max_points,
                                                             unsigned long long* __restrict__ keys,
                                                             int32_t* __restrict__ points,
                                                             int32_t* __restrict__ counts) {
    __shared__ GfLds L;
    const size_t n = blockIdx.x;
    const uint8_t* mk = mask + n * (size_t)h * w;
    int32_t* pts = points + n * (size_t)max_points * 2;
    const int got = good_features_block<kGfT>(L, score + n * (size_t)h * w, h, w, q_num, q_den, min_dist, max_points,
                                              keys + n * (size_t)(h - 2) * (w - 2), pts,
                                              [mk](int p) { return mk[p] != 0; });
    for (int i = 2 * got + threadIdx.x; i < 2 * max_points; i += kGfT) pts[i] = 0;   // rows past the count
    if (threadIdx.x == 0) counts[n] = got;
}

size_t clahe_lut_bytes(int n) { return up((size_t)n * kClaheTiles * kClaheTiles * 256); }
size_t good_features_key_bytes(int n, int h, int w) { return up((size_t)n * (h - 2) * (w - 2) * 8); }

}  // namespace

extern "C" {

#define LF_PLANE_CHECKS(name, n, h, w)                                                                           \
    LF_REQUIRE(n > 0 && n <= 65535, name ": bad batch n=%d", n);                                                  \
    LF_REQUIRE(h >= 8 && w >= 8, name ": a %d x %d image is below the 8 x 8 minimum", h, w);                      \
    LF_REQUIRE((size_t)h * w < ((size_t)1 << 30), name ": image too large")

size_t lf_clahe_workspace(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return clahe_lut_bytes(n);
}

int lf_clahe_u8(const uint8_t* gray, uint8_t* out, int n, int h, int w, void* workspace, size_t ws_bytes,
                lf_stream_t stream) {
    LF_REQUIRE(gray && out && workspace, "lf_clahe: null buffer");
    LF_PLANE_CHECKS("lf_clahe", n, h, w);
    const int wp = (w + 7) & ~7, hp = (h + 7) & ~7;
    LF_REQUIRE((size_t)wp * hp <= kClaheMaxArea, "lf_clahe: a %d x %d image is over the 2^27-pixel limit", h, w);
    LF_REQUIRE(ws_bytes >= lf_clahe_workspace(n, h, w), "lf_clahe: workspace too small (%zu < %zu)", ws_bytes,
               lf_clahe_workspace(n, h, w));
    hipStream_t s = lf::as_stream(stream);
    uint8_t* luts = static_cast<uint8_t*>(workspace);
    const int tw = wp / kClaheTiles, th = hp / kClaheTiles;
    clahe_lut_kernel<<<dim3(kClaheTiles * kClaheTiles, n), kBlock, 0, s>>>(gray, luts, h, w, tw, th);
    clahe_apply_kernel<<<dim3((h * w + kBlock - 1) / kBlock, n), kBlock, 0, s>>>(gray, luts, out, h, w, tw, th);
    return lf::check_launch("lf_clahe");
}

int lf_bilateral_u8(const uint8_t* gray, const int32_t* wc, const int32_t* ws, uint8_t* out, int n, int h, int w,
                    lf_stream_t stream) {
    LF_REQUIRE(gray && wc && ws && out, "lf_bilateral: null buffer");
    LF_PLANE_CHECKS("lf_bilateral", n, h, w);
    LF_REQUIRE(gray != out, "lf_bilateral: in place is not supported");
    bilateral_kernel<<<dim3((h * w + kBlock - 1) / kBlock, n), kBlock, 0, lf::as_stream(stream)>>>(gray, wc, ws, out,
                                                                                                   h, w);
    return lf::check_launch("lf_bilateral");
}

int lf_corner_score_u8(const uint8_t* gray, int32_t* score, int n, int h, int w, lf_stream_t stream) {
    LF_REQUIRE(gray && score, "lf_corner_score: null buffer");
    LF_PLANE_CHECKS("lf_corner_score", n, h, w);
    corner_score_kernel<<<dim3((h * w + kBlock - 1) / kBlock, n), kBlock, 0, lf::as_stream(stream)>>>(gray, score, h,
                                                                                                      w);
    return lf::check_launch("lf_corner_score");
}

size_t lf_good_features_workspace(int n, int h, int w) {
    if (n <= 0 || h < 3 || w < 3) return 0;
    return good_features_key_bytes(n, h, w);
}

int lf_good_features(const int32_t* score, const uint8_t* mask, int32_t* points, int32_t* counts, int n, int h, int w,
                     int q_num, int q_den, int min_dist, int max_points, void* workspace, size_t ws_bytes,
                     lf_stream_t stream) {
    LF_REQUIRE(score && mask && points && counts && workspace, "lf_good_features: null buffer");
    LF_PLANE_CHECKS("lf_good_features", n, h, w);
    LF_REQUIRE(q_num >= 0 && q_den > 0, "lf_good_features: bad quality %d / %d", q_num, q_den);
    LF_REQUIRE(min_dist >= 0 && min_dist <= 16384, "lf_good_features: bad min_dist %d", min_dist);
    LF_REQUIRE(max_points >= 1 && max_points <= (1 << 20), "lf_good_features: bad max_points %d", max_points);
    LF_REQUIRE(ws_bytes >= lf_good_features_workspace(n, h, w), "lf_good_features: workspace too small (%zu < %zu)",
               ws_bytes, lf_good_features_workspace(n, h, w));
    LF_REQUIRE((reinterpret_cast<size_t>(workspace) & 15) == 0, "lf_good_features: workspace must be 16-byte aligned");
    good_features_kernel<<<n, kGfT, 0, lf::as_stream(stream)>>>(score, mask, h, w, q_num, q_den, min_dist, max_points,
                                                               static_cast<unsigned long long*>(workspace), points,
                                                               counts);
    return lf::check_launch("lf_good_features");
}

}  // extern "C"

// ===========================================================================
// apply_landmarks_filter (srcs/transform/filters/landmarks.py) for a same-size batch.  The pixel stages above and the
// gray / Canny / Sobel kernels run on workspace planes; then one workgroup per image, beside brown_spots_kernel and
// with its helpers, does everything that needs bit planes, labels, the contour and drawing.  The rules: "Landmark
// rules" in include/leafhip.h, restated by tests/landmarks_ref.py.  Every walk is bounded: the union-find, flood and
// border walks by their own step bounds, point selection by max_points, the component loop by the component count.
// ===========================================================================
namespace {

constexpr unsigned kLmRed = 0x0000ffu, kLmGreen = 0x00ff00u, kLmBlue = 0xff0000u,
                   kLmBrown = 139u | (69u << 8) | (19u << 16);   // r | g << 8 | b << 16

struct LmArgs {
    MaskArgs a;   // the brown predicate, se_brown, brown_min_area
    int bq, vq, dq, pcap, ccap, gfcap;
};

struct LmLds {
    GfLds gf;
    ContourBox box;
    int m, nb, ncomp, tarea;
    unsigned long long sel, sx, sy;
};

// edges = e1 | e2 | (uint8(minmax-normalised Sobel magnitude) > 40), as 0 / 255
__global__ __launch_bounds__(kBlock) void lm_edges_kernel(const uint8_t* __restrict__ e1,
                                                          const uint8_t* __restrict__ e2,
                                                          const float* __restrict__ gmag,
                                                          const unsigned* __restrict__ mm, uint8_t* __restrict__ out,
                                                          int hw) {
    const unsigned n = blockIdx.y;
    __shared__ float coef[2];
    if (threadIdx.x == 0) norm_coeffs(mm[n * 6 + 0], mm[n * 6 + 1], coef[0], coef[1]);
    __syncthreads();
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= hw) return;
    const size_t i = (size_t)n * hw + p;
    out[i] = (e1[i] | e2[i] || trunc_u8(__fmaf_rn(gmag[i], coef[0], coef[1])) > 40) ? 255 : 0;
}

// discs of radius r (|p - q|^2 <= r^2 + r, an overwrite) at `count` points (kind, x, y), by the whole workgroup
__device__ void lm_discs(uint8_t* img, int h, int w, const int* pts3, int count, int r, unsigned k) {
    const int side = 2 * r + 1, cells = side * side;
    for (int i = threadIdx.x; i < count * cells; i += kMaskT) {
        const int pi = i / cells, o = i - pi * cells;
        const int ox = o % side - r, oy = o / side - r;
        const int x = pts3[3 * pi + 1] + ox, y = pts3[3 * pi + 2] + oy;
        if (ox * ox + oy * oy <= r * r + r && x >= 0 && x < w && y >= 0 && y < h) put_px(img, w, x, y, k);
    }
    __syncthreads();
}

__device__ __forceinline__ double lm_seg_len(const int* cp, int m, int k) {
    const int j = k + 1 < m ? k + 1 : 0;
    const long long dx = cp[2 * j] - cp[2 * k], dy = cp[2 * j + 1] - cp[2 * k + 1];
    return __dsqrt_rn((double)(dx * dx + dy * dy));
}

// resample_contour: bq points along the closed polygon cp[0 .. m), one lane, float64 in numpy's order.  Returns the
// number of points written to pts3 as (0, x, y).
__device__ int lm_resample(const int* cp, int m, int bq, int* pts3) {
    double total = 0.0;
    for (int k = 0; k < m; ++k) total = __dadd_rn(total, lm_seg_len(cp, m, k));
    if (total == 0.0) {
        pts3[0] = 0;
        pts3[1] = cp[0];
        pts3[2] = cp[1];
        return 1;
    }
    const double step = __ddiv_rn(total, (double)bq);
    int j = 0;
    double cj = 0.0, cj1 = lm_seg_len(cp, m, 0);   // cum[j], cum[j + 1]
    for (int i = 0; i < bq; ++i) {
        const double t = __dmul_rn((double)i, step);
        while (j < m && cj1 < t) {   // at most m advances over the whole loop
            ++j;
            cj = cj1;
            if (j < m) cj1 = __dadd_rn(cj, lm_seg_len(cp, m, j));
        }
        int x = cp[0], y = cp[1];
        if (j < m) {
            const int j1 = j + 1 < m ? j + 1 : 0;
            const double dt = __dsub_rn(cj1, cj);
            const double a = dt == 0.0 ? 0.0 : __ddiv_rn(__dsub_rn(t, cj), dt), b = __dsub_rn(1.0, a);
            x = (int)__dadd_rn(__dmul_rn(b, (double)cp[2 * j]), __dmul_rn(a, (double)cp[2 * j1]));
            y = (int)__dadd_rn(__dmul_rn(b, (double)cp[2 * j + 1]), __dmul_rn(a, (double)cp[2 * j1 + 1]));
        }
        pts3[3 * i] = 0;
        pts3[3 * i + 1] = x;
        pts3[3 * i + 2] = y;
    }
    return bq;
}

__global__ __launch_bounds__(kMaskT) void landmarks_kernel(
    const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ leaf_mask, const int* __restrict__ contour,
    const int* __restrict__ counts, int cap, const uint8_t* __restrict__ edges, const int32_t* __restrict__ score_q,
    const int32_t* __restrict__ score_g, const uint16_t* __restrict__ lab_tabs, Run* __restrict__ runs,
    int* __restrict__ parent, int* __restrict__ area, int runs_per_image, int h, int w, int wpr, LmArgs g,
    unsigned long long* __restrict__ keys, int* cbuf, int* gfbuf, uint8_t* out, int* points,
    int* __restrict__ pcounts, int* __restrict__ flags) {
    extern __shared__ unsigned lds_planes[];
    __shared__ HsvTabs H;
    __shared__ LabTabs T;
    __shared__ PostLds S;
    __shared__ LmLds L;
    const size_t n = blockIdx.x;
    const int tid = threadIdx.x, hw = h * w;
    const Post P = post_view(lds_planes, 4, S, runs, parent, area, runs_per_image, h, w, wpr, kMaskT);
    H.fill(kMaskT);
    T.fill(lab_tabs, kMaskT);
    const uint8_t* img = rgb + n * (size_t)hw * 3;
    const uint8_t* lm = leaf_mask + n * (size_t)hw;
    const uint8_t* ed = edges + n * (size_t)hw;
    const int32_t *sq = score_q + n * (size_t)hw, *sg = score_g + n * (size_t)hw;
    const int* cin = contour + n * (size_t)cap * 2;
    unsigned long long* kb = keys + n * (size_t)(h - 2) * (w - 2);
    int* cb = cbuf + n * (size_t)g.ccap * 2;
    int* gp = gfbuf + n * (size_t)g.gfcap * 2;
    int* pts = points + n * (size_t)g.pcap * 3;
    uint8_t* o = out + n * (size_t)hw * 3;

    const int m0 = contour_bbox<kMaskT>(L.box, cin, counts[n], cap, h, w);
    if (m0 <= 0 || L.box.bad) {   // no contour: the copy, no points; a bad record: the error bit
        if (tid == 0) {
            flags[n] = L.box.bad ? kRoiBad : 0;
            pcounts[3 * n] = pcounts[3 * n + 1] = pcounts[3 * n + 2] = 0;
        }
        return;
    }
    auto bit = [&](const unsigned* pl, int p) {
        const int y = p / w, x = p - y * w;
        return ((pl[y * wpr + (x >> 5)] >> (x & 31)) & 1u) != 0;
    };

    // 1: the enhanced mask E = close5(M | close5(brown & M)) in P.A, its largest external contour C'
    build_plane(P, P.A, kMaskT, [&](int y, int x) { return lm[y * w + x] > 0; });
    build_plane(P, P.B, kMaskT,
                [&](int y, int x) { return lm[y * w + x] > 0 && brown_px(H, T, img + 3 * (y * w + x), g.a); });
    morph_ellipse<5>(P, P.B, P.C, false, kMaskT);
    morph_ellipse<5>(P, P.C, P.B, true, kMaskT);
    for (int i = tid; i < h * wpr; i += kMaskT) P.A[i] |= P.B[i];
    __syncthreads();
    morph_ellipse<5>(P, P.A, P.C, false, kMaskT);
    morph_ellipse<5>(P, P.C, P.A, true, kMaskT);
    long long area2 = 0;
    const int best = largest_external(P, area2);
    if (tid == 0) {
        int m = -1;   // E is empty: C' = C
        if (best >= 0) {
            const Run r = P.rn[best];
            long long a2;
            m = trace_outer(P, P.A, r.x0, r.y, a2, cb, g.ccap, false, 1.f);
            if (m > g.ccap) {   // the contour buffer of the workspace is full
                atomicOr(P.status, kFlagBound);
                m = g.ccap;
            }
        }
        L.m = m;
    }
    __syncthreads();
    const int* cp = L.m < 0 ? cin : cb;
    const int m = L.m < 0 ? m0 : L.m;

    // 2: the border points
    if (tid == 0) L.nb = lm_resample(cp, m, g.bq, pts);
    __syncthreads();
    const int nb = L.nb;

    // 3: the vein points: corners of the equalised plane on the dilated edges inside erode3(E), then the fill
    morph_ellipse<3>(P, P.A, P.B, true, kMaskT);
    build_plane(P, P.C, kMaskT, [&](int y, int x) {
        return ed[y * w + x] != 0 && ((P.B[y * wpr + (x >> 5)] >> (x & 31)) & 1u);
    });
    morph_ellipse<3>(P, P.C, P.D, false, kMaskT);
    const int vgot = good_features_block<kMaskT>(L.gf, sq, h, w, 2, 1000, 2, g.vq, kb, gp,
                                                 [&](int p) { return bit(P.D, p); });
    __syncthreads();
    for (int i = tid; i < vgot; i += kMaskT) {
        pts[3 * (nb + i)] = 1;
        pts[3 * (nb + i) + 1] = gp[2 * i];
        pts[3 * (nb + i) + 2] = gp[2 * i + 1];
    }
    int nv = vgot;
    if (vgot < g.vq) {   // evenly spaced set pixels of D in raster order
        for (int y = tid; y < h; y += kMaskT) {
            int c = 0;
            for (int i = 0; i < wpr; ++i) c += __popc(P.D[y * wpr + i]);
            P.rowstart[y + 1] = c;
        }
        if (tid == 0) P.rowstart[0] = 0;
        __syncthreads();
        if (tid == 0)
            for (int y = 0; y < h; ++y) P.rowstart[y + 1] += P.rowstart[y];
        __syncthreads();
        const int cnt = P.rowstart[h], need = g.vq - vgot;
        if (cnt > 0) {
            for (int i = tid; i < need; i += kMaskT) {
                int r = need == 1 ? 0 : (int)(((long long)i * (cnt - 1)) / (need - 1));
                int lo = 0, hi = h - 1;   // the last row whose start is <= r
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (P.rowstart[mid] <= r) lo = mid;
                    else hi = mid - 1;
                }
                r -= P.rowstart[lo];
                int x = 0;
                for (int xw = 0; xw < wpr; ++xw) {
                    unsigned wd = P.D[lo * wpr + xw];
                    const int pc = __popc(wd);
                    if (r >= pc) {
                        r -= pc;
                        continue;
                    }
                    for (; r > 0; --r) wd &= wd - 1;
                    x = 32 * xw + __builtin_ctz(wd);
                    break;
                }
                pts[3 * (nb + vgot + i)] = 1;
                pts[3 * (nb + vgot + i) + 1] = x;
                pts[3 * (nb + vgot + i) + 2] = lo;
            }
            nv = g.vq;
        }
        __syncthreads();
    }

    // 4: the disease points: components of open-close(brown & E), largest first
    build_plane(P, P.B, kMaskT, [&](int y, int x) {
        return ((P.A[y * wpr + (x >> 5)] >> (x & 31)) & 1u) && brown_px(H, T, img + 3 * (y * w + x), g.a);
    });
    morph_se(P, P.B, P.C, g.a.se_brown, true, kMaskT);   // MORPH_OPEN
    morph_se(P, P.C, P.B, g.a.se_brown, false, kMaskT);
    morph_se(P, P.B, P.C, g.a.se_brown, false, kMaskT);  // MORPH_CLOSE
    morph_se(P, P.C, P.B, g.a.se_brown, true, kMaskT);
    label_runs(P, P.B, true);
    const int nr = *P.nruns;
    if (tid == 0) L.ncomp = L.tarea = 0;
    __syncthreads();
    {
        int c = 0, px = 0;
        for (int k = tid; k < nr; k += kMaskT) {
            if (P.par[k] != k || P.area[k] < g.a.brown_min_area) continue;
            ++c;
            px += P.area[k];
        }
        if (c) {
            atomicAdd(&L.ncomp, c);
            atomicAdd(&L.tarea, px);
        }
    }
    __syncthreads();
    const int ncomp = L.ncomp;
    const int quota = min(max(ncomp, L.tarea / 50), 5 * g.dq);
    int placed = 0;
    unsigned long long prev = ~0ull;
    int* dp = pts + 3 * (nb + nv);
    for (int it = 0; it < ncomp && placed < quota; ++it) {
        if (tid == 0) L.sel = L.sx = L.sy = 0;
        __syncthreads();
        unsigned long long b = 0;   // the next component: area descending, then first run ascending
        for (int k = tid; k < nr; k += kMaskT) {
            if (P.par[k] != k || P.area[k] < g.a.brown_min_area) continue;
            const unsigned long long key = ((unsigned long long)(unsigned)P.area[k] << 32) | (0xffffffffu - (unsigned)k);
            if (key < prev) b = max(b, key);
        }
        for (int off = 32; off; off >>= 1) b = max(b, __shfl_xor(b, off));
        if ((tid & 63) == 0 && b) atomicMax(&L.sel, b);
        __syncthreads();
        const unsigned long long sel = L.sel;
        if (!sel) break;
        prev = sel;
        const int comp = (int)(0xffffffffu - (unsigned)sel), carea = (int)(sel >> 32);
        const int k = max(1, min(carea / 40, quota - placed));
        paint_runs(P, P.C, true, [&](int root) { return root == comp; });
        const int got = good_features_block<kMaskT>(L.gf, sg, h, w, 5, 1000, 3, k, kb, gp,
                                                    [&](int p) { return bit(P.C, p); });
        __syncthreads();
        if (got > 0) {
            const int take = min(got, max(1, g.dq - placed));
            for (int i = tid; i < take; i += kMaskT) {
                dp[3 * (placed + i)] = 2;
                dp[3 * (placed + i) + 1] = gp[2 * i];
                dp[3 * (placed + i) + 2] = gp[2 * i + 1];
            }
            placed += take;
        } else {   // the centroid
            unsigned long long sx = 0, sy = 0;
            for (int r = tid; r < nr; r += kMaskT) {
                if (P.par[r] != comp) continue;
                const Run rr = P.rn[r];
                const unsigned long long len = (unsigned)rr.x1 - rr.x0 + 1;
                sx += ((unsigned long long)rr.x0 + rr.x1) * len / 2;
                sy += (unsigned long long)rr.y * len;
            }
            if (sx | sy) {
                atomicAdd(&L.sx, sx);
                atomicAdd(&L.sy, sy);
            }
            __syncthreads();
            if (tid == 0) {
                dp[3 * placed] = 2;
                dp[3 * placed + 1] = (int)(L.sx / (unsigned)carea);
                dp[3 * placed + 2] = (int)(L.sy / (unsigned)carea);
            }
            placed += 1;
        }
        __syncthreads();
    }
    const int nd = placed;

    // 5: the picture, unless a bound was hit
    __syncthreads();
    const int status = S.status;
    if (tid == 0) {
        flags[n] = kRoiFound | status;
        pcounts[3 * n] = status ? 0 : nb;
        pcounts[3 * n + 1] = status ? 0 : nv;
        pcounts[3 * n + 2] = status ? 0 : nd;
    }
    if (status) return;
    lm_discs(o, h, w, pts, nb, 2, kLmRed);
    for (int i = 0; i < m; ++i) {
        const int j = i + 1 < m ? i + 1 : 0;
        draw_aa(o, h, w, cp[2 * i], cp[2 * i + 1], cp[2 * j], cp[2 * j + 1], kLmGreen, tid, kMaskT);
        __syncthreads();
    }
    lm_discs(o, h, w, pts + 3 * nb, nv, 2, kLmBlue);
    lm_discs(o, h, w, dp, nd, 4, kLmBrown);
}

int lm_quota(int landmarks_count, int* bq, int* vq, int* dq) {
    const int total = std::max(1, landmarks_count);
    *bq = *vq = std::max(1, total / 3);
    *dq = std::max(1, total - *bq - *vq);
    return *bq + *vq + 5 * *dq;
}

struct LandmarksWs {
    uint8_t *gray, *q, *bil, *e1, *e2, *luts, *canny;
    int32_t *sq, *sg, *mag2;
    uint32_t* dxdy;
    float* gmag;
    unsigned* mm;
    unsigned long long* keys;
    int *cbuf, *gfbuf;
    size_t canny_bytes, lut_bytes;
    int ccap, gfcap;
    LabelBufs lb;
    size_t bytes;
    LandmarksWs(void* base, int n, int h, int w, int landmarks_count) {
        Carver c{base};
        const size_t px = (size_t)n * h * w;
        int bq, vq, dq;
        lm_quota(landmarks_count, &bq, &vq, &dq);
        ccap = 8 * (h + w);
        gfcap = std::max(vq, 5 * dq);
        gray = c.take<uint8_t>(px);
        q = c.take<uint8_t>(px);     // CLAHE(gray)
        bil = c.take<uint8_t>(px);   // bilateral(q)
        e1 = c.take<uint8_t>(px);    // Canny(q) -> the union of the three edge maps
        e2 = c.take<uint8_t>(px);    // Canny(bil)
        sq = c.take<int32_t>(4 * px);
        sg = c.take<int32_t>(4 * px);
        gmag = c.take<float>(4 * px);
        mm = c.take<unsigned>((size_t)n * 6 * sizeof(unsigned));
        const CannyWs cw(nullptr, n, h, w);
        canny_bytes = cw.bytes;
        canny = c.take<uint8_t>(canny_bytes);   // Canny's magnitude / (dx, dy), also what sal_sobel_kernel leaves there
        const CannyWs cv(canny, n, h, w);
        mag2 = cv.mag;
        dxdy = cv.dxdy;
        lut_bytes = clahe_lut_bytes(n);
        luts = c.take<uint8_t>(lut_bytes);
        keys = c.take<unsigned long long>(good_features_key_bytes(n, h, w));
        cbuf = c.take<int>((size_t)n * ccap * 2 * 4);
        gfbuf = c.take<int>((size_t)n * gfcap * 2 * 4);
        lb.carve(c, n, h, w);
        bytes = c.off;
    }
};

}  // namespace

extern "C" {

int lf_landmarks_points_cap(int landmarks_count) {
    int bq, vq, dq;
    return lm_quota(landmarks_count, &bq, &vq, &dq);
}

size_t lf_landmarks_workspace(int n, int h, int w, int landmarks_count) {
    if (n <= 0 || h < 8 || w < 8) return 0;
    return LandmarksWs(nullptr, n, h, w, landmarks_count).bytes;
}

int lf_landmarks_u8(const uint8_t* rgb, const uint8_t* mask, const int32_t* contour, const int32_t* counts, int cap,
                    const lf_brown_params* prm, int landmarks_count, const int32_t* wc, const int32_t* ws_tab,
                    uint8_t* out, int32_t* points, int32_t* pcounts, int32_t* flags, int n, int h, int w,
                    void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(rgb && mask && contour && counts && prm && wc && ws_tab && out && points && pcounts && flags && workspace,
               "lf_landmarks: null buffer");
    LF_PLANE_CHECKS("lf_landmarks", n, h, w);
    LF_REQUIRE(cap > 0, "lf_landmarks: bad contour capacity %d", cap);
    LF_REQUIRE(h <= 65535 && w <= 65535, "lf_landmarks: image too large (%d x %d)", h, w);
    LF_REQUIRE(landmarks_count <= (1 << 16), "lf_landmarks: landmarks_count %d is over 65536", landmarks_count);
    const size_t lds = post_lds_bytes(4, h, (w + 31) / 32);
    LF_REQUIRE(lds <= kMaskLdsCap,
               "lf_landmarks: a %d x %d image needs %zu bytes of LDS for its four bit planes (limit %zu, one "
               "workgroup per image)", h, w, lds, kMaskLdsCap);
    LF_REQUIRE(prm->morph_kernel >= 1 && prm->morph_kernel <= 31,
               "lf_landmarks: brown_morph_kernel %d outside [1, 31]", prm->morph_kernel);
    LF_REQUIRE(ws_bytes >= lf_landmarks_workspace(n, h, w, landmarks_count),
               "lf_landmarks: workspace too small (%zu < %zu)", ws_bytes,
               lf_landmarks_workspace(n, h, w, landmarks_count));
    LF_REQUIRE((reinterpret_cast<size_t>(workspace) & 255) == 0, "lf_landmarks: workspace must be 256-byte aligned");
    const size_t bytes = (size_t)n * h * w * 3;
    LF_REQUIRE(rgb + bytes <= out || out + bytes <= rgb, "lf_landmarks: rgb and out overlap");
    LF_REQUIRE(lds <= dynamic_lds_cap<landmarks_kernel>(kMaskLdsCap, 48 * 1024),
               "lf_landmarks: could not raise the LDS limit of the landmarks kernel");

    hipStream_t s = lf::as_stream(stream);
    const int hw = h * w;
    const size_t px = (size_t)n * hw;
    const LandmarksWs ws(workspace, n, h, w, landmarks_count);
    LmArgs g{};
    g.a.use_lab = prm->use_lab_brown;
    g.a.hue_lo = prm->hue_lo;
    g.a.hue_hi = prm->hue_hi;
    g.a.s_min = prm->s_min;
    g.a.v_max = prm->v_max;
    g.a.a_min = prm->lab_a_min;
    g.a.b_min = prm->lab_b_min;
    g.a.brown_min_area = prm->min_area_px;
    g.a.se_brown = ellipse_rows(prm->morph_kernel);
    g.pcap = lm_quota(landmarks_count, &g.bq, &g.vq, &g.dq);
    g.ccap = ws.ccap;
    g.gfcap = ws.gfcap;

    if (hipMemcpyAsync(out, rgb, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemsetAsync(points, 0, (size_t)n * g.pcap * 3 * sizeof(int32_t), s) != hipSuccess) {
        lf::set_error("lf_landmarks: the copy of the input failed");
        return LF_ERR_LAUNCH;
    }
    int rc = upload_lab_tables(ws.lb.tabs, s, "lf_landmarks");
    if (rc != LF_OK) return rc;
    rc = lf_rgb2gray_u8(rgb, ws.gray, px, stream);
    if (rc != LF_OK) return rc;
    rc = lf_clahe_u8(ws.gray, ws.q, n, h, w, ws.luts, ws.lut_bytes, stream);
    if (rc != LF_OK) return rc;
    const dim3 grid_px((hw + kBlock - 1) / kBlock, n);
    const dim3 grid_fat((hw + kBlock * kPxPerThread - 1) / (kBlock * kPxPerThread), n);
    minmax_init_kernel<<<(n * 6 + 255) / 256, 256, 0, s>>>(ws.mm, n);
    sal_sobel_kernel<<<grid_fat, kBlock, 0, s>>>(ws.q, ws.mag2, ws.dxdy, ws.gmag, ws.mm, h, w);
    rc = lf_canny_u8(ws.q, ws.e1, n, h, w, 30.0, 90.0, 1, ws.canny, ws.canny_bytes, stream);
    if (rc != LF_OK) return rc;
    rc = lf_bilateral_u8(ws.q, wc, ws_tab, ws.bil, n, h, w, stream);
    if (rc != LF_OK) return rc;
    rc = lf_canny_u8(ws.bil, ws.e2, n, h, w, 50.0, 130.0, 1, ws.canny, ws.canny_bytes, stream);
    if (rc != LF_OK) return rc;
    lm_edges_kernel<<<grid_px, kBlock, 0, s>>>(ws.e1, ws.e2, ws.gmag, ws.mm, ws.bil, hw);
    rc = lf_corner_score_u8(ws.q, ws.sq, n, h, w, stream);
    if (rc != LF_OK) return rc;
    rc = lf_corner_score_u8(ws.gray, ws.sg, n, h, w, stream);
    if (rc != LF_OK) return rc;
    landmarks_kernel<<<n, kMaskT, lds, s>>>(rgb, mask, contour, counts, cap, ws.bil, ws.sq, ws.sg, ws.lb.tabs, ws.lb.rn,
                                            ws.lb.parent, ws.lb.area, (int)mask_runs_per_image(h, w), h, w,
                                            (w + 31) / 32, g, ws.keys, ws.cbuf, ws.gfbuf, out, points, pcounts, flags);
    return lf::check_launch("lf_landmarks");
}

}  // extern "C"
