// The thick-segment rule of include/leafhip.h ("Drawing rules"), stated once for the kernels that draw with it:
// lf_analyze_overlay_u8 (lf_filters.hip) walks a segment's pixels, lf_hist_figure_u8 (lf_hist_fig.hip) asks for one
// pixel which segments cover it.  tests/draw_ref.py is the same reading in numpy.
#pragma once
#include "lf_common.h"

#if defined(__HIPCC__)
namespace lf {

__device__ __forceinline__ long long floor_div(long long a, long long b) {
    const long long q = a / b;
    return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

// Calls px(x, y, u, c, L2) for every pixel of the h x w image that can lie within distance 1 of the segment
// A -> B, major steps t0, t0 + stride, ...: u = (p - A) . d, c = (p - A) x d, L2 = |d|^2.  The walk goes along the
// major axis over [min - 1, max + 1] and at each step offers the five pixels centre - 2 .. centre + 2 across it,
// centre = floor of the line there (see lf_analyze_overlay_u8).
template <class F>
__device__ __forceinline__ void seg_walk(int ax, int ay, int bx, int by, int h, int w, int t0, int stride, F&& px) {
    const long long dx = bx - ax, dy = by - ay, L2 = dx * dx + dy * dy;
    const bool xm = (dx < 0 ? -dx : dx) >= (dy < 0 ? -dy : dy);
    const int a0 = xm ? ax : ay, b0 = xm ? bx : by, a1 = xm ? ay : ax;
    const long long d0 = xm ? dx : dy, d1 = xm ? dy : dx;
    const int n0 = xm ? w : h, n1 = xm ? h : w;
    const int lo = max(min(a0, b0) - 1, 0), hi = min(max(a0, b0) + 1, n0 - 1);
    for (int s = lo + t0; s <= hi; s += stride) {
        const int mid = a1 + (d0 ? (int)floor_div((s - a0) * d1, d0) : 0);
        for (int q = max(mid - 2, 0); q <= min(mid + 2, n1 - 1); ++q) {
            const int x = xm ? s : q, y = xm ? q : s;
            const long long rx = x - ax, ry = y - ay;
            px(x, y, rx * dx + ry * dy, rx * dy - ry * dx, L2);
        }
    }
}

__device__ __forceinline__ void put_px(uint8_t* img, int w, int x, int y, unsigned k) {
    uint8_t* o = img + ((size_t)y * w + x) * 3;
    o[0] = (uint8_t)k;
    o[1] = (uint8_t)(k >> 8);
    o[2] = (uint8_t)(k >> 16);
}

// thickness 2: whether pixel (x, y) lies within distance 1 of the segment A -> B, from the pixel's terms u, c, L2
__device__ __forceinline__ bool thick_covers(int x, int y, int ax, int ay, int bx, int by, long long u, long long c,
                                             long long L2) {
    const long long ex = u <= 0 ? x - ax : x - bx, ey = u <= 0 ? y - ay : y - by;
    return (u <= 0 || u >= L2) ? ex * ex + ey * ey <= 1 : c * c <= L2;
}

// thickness 2: every pixel within distance 1 of the segment
__device__ __forceinline__ void draw_thick(uint8_t* img, int h, int w, int ax, int ay, int bx, int by, unsigned k,
                                           int t0, int stride) {
    seg_walk(ax, ay, bx, by, h, w, t0, stride, [&](int x, int y, long long u, long long c, long long L2) {
        if (thick_covers(x, y, ax, ay, bx, by, u, c, L2)) put_px(img, w, x, y, k);
    });
}

}  // namespace lf
#endif
