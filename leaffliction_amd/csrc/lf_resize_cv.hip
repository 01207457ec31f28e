// cv2.resize(img, (OW, OH), interpolation=cv2.INTER_LANCZOS4) for 8-bit RGB, with the training provider's light
// augmentation fused into the store (lf_resize_lanczos4_u8).  The resize of srcs/cli/Transformation.py:799-801 and
// :941-946; a different algorithm from Pillow's LANCZOS (lf_geom.hip): eight fixed taps whatever the scale, 11-bit
// coefficients, a 32-bit intermediate.
//
// The reading of OpenCV's 8-bit resize implemented here (cv2 is not available to check against: parity is unpinned).
// The tables are built on the host (ops.lanczos4_axis_table); the kernel does integer work only.
//   Per axis, scale = 1.0 / (dst / (double)src).  Per output index d: f = (float)((d + 0.5) * scale - 0.5),
//   s = floor(f), f -= s in float.  Eight float taps (interpolateLanczos4): f < FLT_EPSILON gives {0,0,0,1,0,0,0,0};
//   else with y0 = -(f+3)*pi*0.25 (f+3 a float sum, the product double), s0 = sin y0, c0 = cos y0 and
//   cs = {{1,0},{-r,-r},{0,1},{r,-r},{-1,0},{r,r},{0,-1},{-r,r}}, r = sqrt(1/2):
//   c[i] = (float)((cs[i][0]*s0 + cs[i][1]*c0) / (y*y)), y = -(f+3-i)*pi*0.25; their float sum `sum` in tap order;
//   c[i] *= 1.f / sum.  Fixed point: saturate_cast<short>(cvRound(c[i] * 2048)), no correction of the sum.
//   Tap i of output d reads source index clamp(s - 3 + i, 0, n - 1) (border replication; s itself is not clamped).
//   Horizontal pass: int32 = sum u8 * coef.  Vertical pass: sum int32 * coef in int32 (wrapping, as compiled OpenCV
//   does), then (v + (1 << 21)) >> 22 saturated to 8 bits.  Equal sizes are a copy: every f is 0, both passes are
//   the identity tap 2048, and (p * 2048 * 2048 + (1 << 21)) >> 22 = p.
// Epilogue (_apply_light_augmentation, Transformation.py:984-1005), per image from aug[n] = {use_b, b, use_c, c}:
//   use_b: p = (uint8)clip(p * b, 0, 255); then use_c: p = (uint8)clip((p - 127.5) * c + 127.5, 0, 255); float64,
//   multiply and add rounded separately as numpy does (the casts truncate).
//
// Layout: one workgroup of 256 threads per output tile of up to 32 x 32 pixels.  The tile's source window (the rows
// and columns its taps reach after clamping) is staged in LDS as bytes, the horizontal pass of every window row is
// kept in LDS as int32, the vertical pass reads it and stores four bytes per thread.  The window is at most
// kWin x kWin source pixels; the host shrinks the tile (down to one output, whose eight taps span eight inputs) until
// every tile's window fits, so any scale is taken.  LDS: 9.2 KiB window + 21 KiB intermediate + 4 KiB tables.
#include "lf_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kT = 32;     // largest output tile side
constexpr int kWin = 56;   // source window side: 32 outputs at scales up to 1.5, fewer outputs beyond
constexpr int kTaps = 8;
constexpr int kWinPitch = kWin * 3;   // bytes per staged window row
constexpr int kTmpPitch = kT * 3;     // int32 per intermediate row

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned augment(unsigned p, bool use_b, double b, bool use_c, double c) {
    if (use_b) {
        const double v = __dmul_rn((double)p, b);
        p = (unsigned)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
    }
    if (use_c) {
        const double v = __dadd_rn(__dmul_rn(__dadd_rn((double)p, -127.5), c), 127.5);
        p = (unsigned)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
    }
    return p;
}

// tables: xofs[ow], xcoef[ow][8], yofs[oh], ycoef[oh][8] (int32)
__global__ __launch_bounds__(kBlock) void resize_lanczos4_kernel(const uint8_t* __restrict__ in,
                                                                 uint8_t* __restrict__ out, int h, int w, int oh,
                                                                 int ow, int tile_h, int tile_w,
                                                                 const int32_t* __restrict__ tables,
                                                                 const double* __restrict__ aug, int n_images) {
    __shared__ uint8_t win[kWin * kWinPitch];
    __shared__ int tmp[kWin * kTmpPitch];
    __shared__ int kxs[kTaps][kT], kys[kTaps][kT], xrel[kTaps][kT], yrel[kTaps][kT];
    const lf::TileId tile = lf::xcd_tile((ow + tile_w - 1) / tile_w, (oh + tile_h - 1) / tile_h, n_images);
    if (!tile.ok) return;
    const int tid = threadIdx.x;
    const int ox0 = tile.tx * tile_w, oy0 = tile.ty * tile_h;
    const int cols = min(tile_w, ow - ox0), rows = min(tile_h, oh - oy0);
    const int32_t* xofs = tables;
    const int32_t* xcoef = tables + ow;
    const int32_t* yofs = tables + (size_t)ow * (1 + kTaps);
    const int32_t* ycoef = yofs + oh;
    // the window: from the first output's first tap to the last output's last tap (the offsets do not decrease)
    const int xlo = clampi(xofs[ox0] - 3, 0, w - 1), xhi = clampi(xofs[ox0 + cols - 1] + 4, 0, w - 1);
    const int ylo = clampi(yofs[oy0] - 3, 0, h - 1), yhi = clampi(yofs[oy0 + rows - 1] + 4, 0, h - 1);
    const int wx = min(xhi - xlo + 1, kWin), wy = min(yhi - ylo + 1, kWin);   // (the host chose a tile that fits)

    // tables of the tile: coefficients and window-relative tap positions, tap-major
    for (int it = tid; it < 2 * kTaps * kT; it += kBlock) {
        const int axis = it / (kTaps * kT), r = it - axis * (kTaps * kT), i = r / kT, c = r - i * kT;
        if (axis == 0) {
            const bool on = c < cols;
            const int s = on ? xofs[ox0 + c] : 0;
            kxs[i][c] = on ? xcoef[(size_t)(ox0 + c) * kTaps + i] : 0;
            xrel[i][c] = clampi(clampi(s - 3 + i, 0, w - 1) - xlo, 0, wx - 1) * 3;
        } else {
            const bool on = c < rows;
            const int s = on ? yofs[oy0 + c] : 0;
            kys[i][c] = on ? ycoef[(size_t)(oy0 + c) * kTaps + i] : 0;
            yrel[i][c] = clampi(clampi(s - 3 + i, 0, h - 1) - ylo, 0, wy - 1) * kTmpPitch;
        }
    }
    // stage the window: consecutive threads take consecutive bytes of a row
    const uint8_t* src = in + ((size_t)tile.n * h + ylo) * w * 3 + (size_t)xlo * 3;
    const int rowb = wx * 3;
    for (int it = tid; it < wy * rowb; it += kBlock) {
        const int r = it / rowb, b = it - r * rowb;
        win[r * kWinPitch + b] = src[(size_t)r * w * 3 + b];
    }
    __syncthreads();

    // horizontal pass: every window row, the tile's columns
    for (int it = tid; it < wy * kT; it += kBlock) {
        const int r = it / kT, c = it - r * kT;
        if (c >= cols) continue;
        const uint8_t* q = win + r * kWinPitch;
        unsigned s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int i = 0; i < kTaps; ++i) {
            const unsigned k = (unsigned)kxs[i][c];
            const uint8_t* p = q + xrel[i][c];
            s0 += p[0] * k;
            s1 += p[1] * k;
            s2 += p[2] * k;
        }
        int* o = tmp + r * kTmpPitch + c * 3;
        o[0] = (int)s0;
        o[1] = (int)s1;
        o[2] = (int)s2;
    }
    __syncthreads();

    // vertical pass and store: a thread makes four consecutive bytes of one output row of the tile
    const double* a = aug ? aug + (size_t)tile.n * 4 : nullptr;
    const bool use_b = a && a[0] != 0.0, use_c = a && a[2] != 0.0;
    const double fb = use_b ? a[1] : 1.0, fc = use_c ? a[3] : 1.0;
    const int rowo = cols * 3;
    uint8_t* dst = out + (((size_t)tile.n * oh + oy0) * ow + ox0) * 3;
    for (int it = tid; it < rows * (kTmpPitch / 4); it += kBlock) {
        const int r = it / (kTmpPitch / 4), b0 = (it - r * (kTmpPitch / 4)) * 4;
        if (b0 >= rowo) continue;
        unsigned v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < kTaps; ++i) {
            const unsigned k = (unsigned)kys[i][r];
            const int* p = tmp + yrel[i][r] + b0;   // (bytes past the tile's columns are computed and dropped)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += (unsigned)p[j] * k;
        }
        unsigned px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = (int)(v[j] + (1u << 21)) >> 22;
            px[j] = augment((unsigned)clampi(q, 0, 255), use_b, fb, use_c, fc);
        }
        uint8_t* o = dst + (size_t)r * ow * 3 + b0;
        if (b0 + 4 <= rowo && (reinterpret_cast<size_t>(o) & 3) == 0) {
            *reinterpret_cast<uint32_t*>(o) = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
        } else {
            for (int j = 0; j < 4 && b0 + j < rowo; ++j) o[j] = (uint8_t)px[j];
        }
    }
}

// The largest tile side <= kT (HOST) whose every tile reads a window of at most kWin inputs of an axis of n inputs
// and `outputs` outputs with the offsets ofs; 0 if the offsets decrease.  One output always fits: eight taps.
int fit_tile(const int32_t* ofs, int outputs, int n) {
    for (int i = 1; i < outputs; ++i)
        if (ofs[i] < ofs[i - 1]) return 0;
    auto clampl = [n](long long v) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); };
    for (int t = kT; t > 1; --t) {
        bool ok = true;
        for (int o0 = 0; o0 < outputs && ok; o0 += t) {
            const int o1 = std::min(o0 + t, outputs) - 1;
            ok = clampl((long long)ofs[o1] + 4) - clampl((long long)ofs[o0] - 3) + 1 <= kWin;
        }
        if (ok) return t;
    }
    return 1;
}

}  // namespace

extern "C" {

int lf_resize_lanczos4_u8(const uint8_t* in, uint8_t* out, int n, int h, int w, int oh, int ow,
                          const int32_t* tables, const int32_t* host_tables, const double* aug,
                          lf_stream_t stream) {
    LF_REQUIRE(in && out && tables && host_tables, "lf_resize_lanczos4: null buffer");
    LF_REQUIRE(n > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "lf_resize_lanczos4: bad dims n=%d h=%d w=%d oh=%d ow=%d",
               n, h, w, oh, ow);
    LF_REQUIRE((size_t)h * w * 3 < ((size_t)1 << 31) && (size_t)oh * ow * 3 < ((size_t)1 << 31),
               "lf_resize_lanczos4: image too large");
    LF_REQUIRE(in != out, "lf_resize_lanczos4: in-place resize is not supported");
    const int32_t* yofs = host_tables + (size_t)ow * (1 + kTaps);
    const int tile_w = fit_tile(host_tables, ow, w), tile_h = fit_tile(yofs, oh, h);
    LF_REQUIRE(tile_w > 0 && tile_h > 0, "lf_resize_lanczos4: source offsets must not decrease");
    const size_t tiles = (size_t)((ow + tile_w - 1) / tile_w) * ((oh + tile_h - 1) / tile_h) * n;
    LF_REQUIRE(tiles < ((size_t)1 << 31) - 8, "lf_resize_lanczos4: too many tiles");
    resize_lanczos4_kernel<<<lf::xcd_grid(tiles), kBlock, 0, lf::as_stream(stream)>>>(in, out, h, w, oh, ow, tile_h,
                                                                                      tile_w, tables, aug, n);
    return lf::check_launch("lf_resize_lanczos4");
}

}  // extern "C"
