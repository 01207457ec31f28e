// lf_hist_figure_u8: the geometry of Transformation's Hist figure, [N][640][960][3] uint8 from lf_hsv_region_stats'
// 14 counts and 3 x 256 histogram entries per image.  The rules are stated in include/leafhip.h ("Charts");
// tests/chart_ref.py restates them in numpy.
//
// A pixel's colour is a function of its image's 782 numbers and its own coordinates, so the kernel is a store stream
// (1.8 MB per image) behind a small preamble.  A workgroup of 256 threads takes kRows rows of one image.  Preamble:
// the 8 bar lengths and 5 bar heights (a lane each), and, for the rows of the upper panels only, the 192 curve
// points: wave c sums channel c's histogram into its 64 bins, a lane per bin, and takes the channel's largest bin
// with a butterfly of wave shuffles; all of it lands in a few hundred bytes of LDS.  Then a lane finishes runs of
// four pixels of one row (12 bytes, three aligned dword stores: the figure's width is a multiple of four and a
// torch allocation is dword-aligned; the launcher checks), evaluating for each pixel the elements of its panel in
// paint order; for a curve, the one or two segments whose columns reach the pixel.  No atomics, no ordering between
// threads, integer arithmetic only; the products that can pass 2^32 are int64.
#include "lf_common.h"
#include "lf_draw.h"

namespace {

constexpr int kBlock = 256;
constexpr int kH = LF_HIST_FIG_H, kW = LF_HIST_FIG_W, kPanelW = LF_CHART_PANEL_W, kPanelH = LF_CHART_PANEL_H;
constexpr int kRows = 8;                       // rows of one image to a workgroup
constexpr int kRowBlocks = kH / kRows;
constexpr int kRunsPerRow = kW / 4, kRuns = kRows * kRunsPerRow;
constexpr int kBins = 64, kPitch = LF_CHART_HSV_PITCH;
constexpr unsigned kWhite = 0xffffffu, kBlack = 0u, kGrid = LF_CHART_GRID, kMarker = LF_CHART_MARKER;

struct Rect {
    int x0, y0, pw, ph;
};
constexpr Rect kRegions = LF_CHART_REGIONS_RECT, kHsv = LF_CHART_HSV_RECT, kHues = LF_CHART_HUES_RECT;
__constant__ unsigned d_region_colours[8] = LF_CHART_REGION_COLOURS;
__constant__ unsigned d_hue_colours[5] = LF_CHART_HUE_COLOURS;
__constant__ unsigned d_curve_colours[3] = LF_CHART_CURVE_COLOURS;

static_assert(kH % kRows == 0 && kPanelH % kRows == 0, "a workgroup's rows lie in one row of panels");
static_assert(kW % 4 == 0 && kPanelW % 4 == 0, "runs of four pixels");
static_assert(kW == 2 * kPanelW && kH == 2 * kPanelH, "four panels");
static_assert(8 * LF_CHART_REGION_SLOT == kRegions.ph && 5 * LF_CHART_HUE_SLOT == kHues.pw, "the bars fill their rectangles");
static_assert(kBins * kPitch == kHsv.pw && kHsv.ph > 3, "the curve points fill their rectangle");
static_assert(kRegions.pw % 4 == 0 && kRegions.ph % 4 == 0 && kHsv.pw % 4 == 0 && kHsv.ph % 4 == 0 &&
                  kHues.pw % 4 == 0 && kHues.ph % 4 == 0, "the grid's quarter positions are whole pixels");
static_assert(kBlock == 256, "waves 0..2 take the three channels, wave 3 the bars");

// what a workgroup keeps of its image
struct Figure {
    int len[8];          // region bars, 0 .. PW
    int hgt[5];          // hue bars, 0 .. PH
    int py[3][kBins];    // curve points: ly of bin j, 1 .. PH - 2
    int has[3];          // the channel has a curve
    long long top[3];    // the channel's largest bin
};

__device__ __forceinline__ long long clamp0(int v) { return v > 0 ? v : 0; }

// The static parts of a chart panel at (lx, ly) of its PW x PH plot rectangle: k = white outside, black on the frame
// around it, the grid's colour or white inside; whether the pixel lies inside the rectangle.
template <int PW, int PH>
__device__ __forceinline__ bool panel_static(int lx, int ly, unsigned& k) {
    k = kWhite;
    if (lx < -1 || lx > PW || ly < -1 || ly > PH) return false;
    if (lx == -1 || lx == PW || ly == -1 || ly == PH) {
        k = kBlack;
        return false;
    }
    if ((lx > 0 && lx % (PW / 4) == 0) || (ly > 0 && ly % (PH / 4) == 0)) k = kGrid;
    return true;
}

__device__ __forceinline__ unsigned figure_pixel(const Figure& f, int x, int y, bool upper) {
    const bool right = x >= kPanelW;
    unsigned k;
    if (!upper) {
        if (!right) return kWhite;   // the summary panel: text only
        const int lx = x - kHues.x0, ly = y - kHues.y0;   // hue ranges: vertical bars
        if (!panel_static<kHues.pw, kHues.ph>(lx, ly, k)) return k;
        const int slot = lx / LF_CHART_HUE_SLOT, in = lx - slot * LF_CHART_HUE_SLOT;
        if (in >= LF_CHART_HUE_BAR_LO && in < LF_CHART_HUE_BAR_HI && ly >= kHues.ph - f.hgt[slot])
            k = d_hue_colours[slot];
        return k;
    }
    if (!right) {   // colour regions: horizontal bars
        const int lx = x - kRegions.x0, ly = y - kRegions.y0;
        if (!panel_static<kRegions.pw, kRegions.ph>(lx, ly, k)) return k;
        const int slot = ly / LF_CHART_REGION_SLOT, in = ly - slot * LF_CHART_REGION_SLOT;
        if (in >= LF_CHART_REGION_BAR_LO && in < LF_CHART_REGION_BAR_HI && lx < f.len[slot])
            k = d_region_colours[slot];
        return k;
    }
    const int lx = x - kHsv.x0, ly = y - kHsv.y0;
    if (!panel_static<kHsv.pw, kHsv.ph>(lx, ly, k)) return k;
    // HSV histograms: markers, then the curves H, S, V
    if ((lx == (kPitch * 15 + 3) / 4 || lx == (kPitch * 35 + 3) / 4 || lx == (kPitch * 85 + 3) / 4) && (ly & 7) < 4)
        k = kMarker;
    // segment j joins the points at lx = 6j + 3 and 6j + 9 and reaches the columns 6j + 2 .. 6j + 10
    if (lx < kPitch / 2 - 1) return k;
    const int j_lo = max(lx - (kPitch + kPitch / 2 + 1) + kPitch - 1, 0) / kPitch;   // ceil((lx - 10) / 6), at least 0
    const int j_hi = min((lx - (kPitch / 2 - 1)) / kPitch, kBins - 2);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (!f.has[c]) continue;
        for (int j = j_lo; j <= j_hi; ++j) {
            const int ax = kPitch * j + kPitch / 2, ay = f.py[c][j], bx = ax + kPitch, by = f.py[c][j + 1];
            const long long dx = bx - ax, dy = by - ay, rx = lx - ax, ry = ly - ay;
            if (lf::thick_covers(lx, ly, ax, ay, bx, by, rx * dx + ry * dy, rx * dy - ry * dx, dx * dx + dy * dy))
                k = d_curve_colours[c];
        }
    }
    return k;
}

__global__ __launch_bounds__(kBlock) void hist_figure_kernel(const int32_t* __restrict__ counts,
                                                             const int32_t* __restrict__ hist,
                                                             uint8_t* __restrict__ out) {
    __shared__ Figure f;
    const int tid = (int)threadIdx.x;
    const size_t n = blockIdx.x / kRowBlocks;
    const int y_first = (int)(blockIdx.x - n * kRowBlocks) * kRows;
    const bool upper = y_first < kPanelH;   // the same for all of a workgroup's rows
    const int32_t* cn = counts + n * LF_HSV_NCOUNTS;

    const int wave = tid >> 6, lane = tid & 63;
    long long bin = 0;
    if (upper) {
        if (wave < 3) {   // a wave per channel, a lane per bin
            const int32_t* p = hist + (n * 3 + wave) * 256 + 4 * lane;
            bin = clamp0(p[0]) + clamp0(p[1]) + clamp0(p[2]) + clamp0(p[3]);
            long long top = bin;
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const long long o = __shfl_xor(top, s, 64);
                top = o > top ? o : top;
            }
            if (lane == 0) f.top[wave] = top;
        } else if (lane < 8) {
            const long long total = cn[0], c = clamp0(cn[1 + lane]);
            f.len[lane] = total > 0 ? (int)(((c < total ? c : total) * kRegions.pw + total / 2) / total) : 0;
        }
    } else if (tid < 5) {
        long long m = 1;
        for (int i = 0; i < 5; ++i) m = clamp0(cn[9 + i]) > m ? clamp0(cn[9 + i]) : m;
        f.hgt[tid] = (int)((clamp0(cn[9 + tid]) * kHues.ph + m / 2) / m);
    }
    __syncthreads();
    if (upper && wave < 3) {
        long long ymax = 1;
        for (int c = 0; c < 3; ++c) ymax = f.top[c] > ymax ? f.top[c] : ymax;
        const long long b = bin < ymax ? bin : ymax;
        f.py[wave][lane] = kHsv.ph - 2 - (int)((b * (kHsv.ph - 3) + ymax / 2) / ymax);
        if (lane == 0) f.has[wave] = f.top[wave] > 0;
    }
    __syncthreads();

    uint8_t* img = out + n * ((size_t)kH * kW * 3);
    for (int r = tid; r < kRuns; r += kBlock) {
        const int row = r / kRunsPerRow, x = (r - row * kRunsPerRow) * 4, y = y_first + row;
        unsigned px[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) px[e] = figure_pixel(f, x + e, y, upper);
        unsigned* wp = reinterpret_cast<unsigned*>(img + ((size_t)y * kW + x) * 3);
        wp[0] = px[0] | (px[1] << 24);
        wp[1] = (px[1] >> 8) | (px[2] << 16);
        wp[2] = (px[2] >> 16) | (px[3] << 8);
    }
}

}  // namespace

extern "C" {

int lf_hist_figure_u8(const int32_t* counts, const int32_t* hsv_hist, uint8_t* out, int n, lf_stream_t stream) {
    LF_REQUIRE(counts && hsv_hist && out, "lf_hist_figure: null buffer");
    LF_REQUIRE(n > 0, "lf_hist_figure: bad dims n=%d", n);
    LF_REQUIRE(reinterpret_cast<uintptr_t>(out) % 4 == 0, "lf_hist_figure: out is not 4-byte aligned");
    LF_REQUIRE((long long)n * kRowBlocks < ((long long)1 << 31), "lf_hist_figure: batch of %d figures is too large", n);
    hist_figure_kernel<<<(unsigned)(n * kRowBlocks), kBlock, 0, lf::as_stream(stream)>>>(counts, hsv_hist, out);
    return lf::check_launch("lf_hist_figure");
}

}  // extern "C"
