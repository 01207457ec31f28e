// lf_canvas_tiles_u8: one [N][OH][OW][3] uint8 canvas composed from T source batches in one launch — each source
// resampled bilinearly into its tile by host-made integer tables, the rest of the canvas filled, then rectangles
// shaded.  The rules are stated in include/leafhip.h ("Canvas"); tests/canvas_ref.py restates them in numpy.
//
// The plan (tile descriptors with their source pointers, shade rectangles, axis tables) is one int32 block uploaded
// once per launch.  A workgroup copies the descriptors and rectangles to LDS (a few hundred bytes); a lane then
// finishes PX consecutive pixels of one canvas row: PX = 4 (12 bytes, three aligned dword stores) when every tile
// offset and width and the canvas width are multiples of four pixels, so that a run lies in one tile or in none,
// PX = 1 otherwise.  A tile of its source's own size whose rows are runs of whole dwords is copied with three
// aligned dword loads per run (the tables would give the same bytes: weight 2048 on the pixel itself).  Integer
// arithmetic only, no atomics, no scratch (the byte arrays are indexed by unrolled constants).
#include "lf_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTileInts = 12;   // dst_x, dst_y, dst_w, dst_h, src_h, src_w, channels, xtab, ytab, ptr lo, ptr hi, flags
constexpr int kShadeInts = 6;   // x, y, w, h, num, den
constexpr int kMaxTiles = 64, kMaxShades = 64;
constexpr int kFlagCopy = 1;    // the tile is a dword-aligned copy of its source
constexpr int kWeightBits = 11, kWeightOne = 1 << kWeightBits;   // table weights are k / 2048

// one axis entry: first tap i, weight of the second tap k (the first tap has 2048 - k); the second tap is
// min(i + 1, S - 1)
struct Tap {
    int i0, i1, k0, k1;
};
__device__ __forceinline__ Tap tap_at(const int32_t* __restrict__ tab, int d, int S) {
    Tap t;
    t.i0 = tab[2 * d];
    t.k1 = tab[2 * d + 1];
    t.k0 = kWeightOne - t.k1;
    t.i1 = min(t.i0 + 1, S - 1);
    return t;
}

template <int PX>
__global__ __launch_bounds__(kBlock) void canvas_tiles_kernel(uint8_t* __restrict__ out, int N, int OH, int OW,
                                                              const int32_t* __restrict__ plan, int n_tiles,
                                                              int n_shades, unsigned fill, unsigned groups_per_image) {
    __shared__ int s_tiles[kMaxTiles * kTileInts];
    __shared__ int s_shades[kMaxShades * kShadeInts];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < n_tiles * kTileInts; i += kBlock) s_tiles[i] = plan[i];
    for (int i = tid; i < n_shades * kShadeInts; i += kBlock) s_shades[i] = plan[n_tiles * kTileInts + i];
    __syncthreads();

    const size_t g = (size_t)blockIdx.x * kBlock + tid;
    const size_t n = g / groups_per_image;
    const unsigned r = (unsigned)(g - n * groups_per_image);
    const unsigned groups_per_row = (unsigned)OW / PX;
    const int y = (int)(r / groups_per_row), x = (int)(r - (unsigned)y * groups_per_row) * PX;
    if (n >= (size_t)N) return;   // the last workgroup's tail

    unsigned bytes[3 * PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) {
        bytes[3 * e + 0] = fill & 0xffu;
        bytes[3 * e + 1] = (fill >> 8) & 0xffu;
        bytes[3 * e + 2] = (fill >> 16) & 0xffu;
    }

    // the tile of this run: tiles do not overlap, and with PX = 4 a run never straddles a tile's edge
    int t = -1;
    for (int i = 0; i < n_tiles; ++i) {
        const int* d = s_tiles + i * kTileInts;
        if (x >= d[0] && x < d[0] + d[2] && y >= d[1] && y < d[1] + d[3]) t = i;
    }
    if (t >= 0) {
        const int* d = s_tiles + t * kTileInts;
        const int sh = d[4], sw = d[5], ch = d[6];
        const uint8_t* src = reinterpret_cast<const uint8_t*>(((unsigned long long)(unsigned)d[10] << 32) |
                                                              (unsigned long long)(unsigned)d[9]) +
                             n * (size_t)sh * sw * ch;
        const int dx = x - d[0], dy = y - d[1];
        if (PX == 4 && (d[11] & kFlagCopy)) {
            const unsigned* ip = reinterpret_cast<const unsigned*>(src + ((size_t)dy * sw + dx) * 3);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const unsigned word = ip[q];
#pragma unroll
                for (int e = 0; e < 4; ++e) bytes[q * 4 + e] = (word >> (8 * e)) & 0xffu;
            }
        } else {
            const Tap ty = tap_at(plan + d[8], dy, sh);
            const uint8_t* row0 = src + (size_t)ty.i0 * sw * ch;
            const uint8_t* row1 = src + (size_t)ty.i1 * sw * ch;
#pragma unroll
            for (int e = 0; e < PX; ++e) {
                const Tap tx = tap_at(plan + d[7], dx + e, sw);
                if (ch == 3) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int a = row0[tx.i0 * 3 + c], b = row0[tx.i1 * 3 + c];
                        const int cc = row1[tx.i0 * 3 + c], dd = row1[tx.i1 * 3 + c];
                        bytes[3 * e + c] = (unsigned)((ty.k0 * (tx.k0 * a + tx.k1 * b) +
                                                       ty.k1 * (tx.k0 * cc + tx.k1 * dd) + (1 << 21)) >> 22);
                    }
                } else {   // gray: one plane, replicated
                    const int a = row0[tx.i0], b = row0[tx.i1], cc = row1[tx.i0], dd = row1[tx.i1];
                    const unsigned v = (unsigned)((ty.k0 * (tx.k0 * a + tx.k1 * b) +
                                                   ty.k1 * (tx.k0 * cc + tx.k1 * dd) + (1 << 21)) >> 22);
                    bytes[3 * e + 0] = bytes[3 * e + 1] = bytes[3 * e + 2] = v;
                }
            }
        }
    }

    for (int i = 0; i < n_shades; ++i) {   // in table order, after the tiles
        const int* s = s_shades + i * kShadeInts;
        if (y < s[1] || y >= s[1] + s[3]) continue;
        const unsigned num = (unsigned)s[4], den = (unsigned)s[5];
#pragma unroll
        for (int e = 0; e < PX; ++e) {
            if (x + e < s[0] || x + e >= s[0] + s[2]) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) bytes[3 * e + c] = (bytes[3 * e + c] * num + den / 2) / den;
        }
    }

    uint8_t* op = out + ((n * OH + y) * (size_t)OW + x) * 3;
    if (PX == 4) {
        unsigned* wp = reinterpret_cast<unsigned*>(op);
#pragma unroll
        for (int q = 0; q < 3; ++q)
            wp[q] = bytes[q * 4] | (bytes[q * 4 + 1] << 8) | (bytes[q * 4 + 2] << 16) | (bytes[q * 4 + 3] << 24);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) op[c] = (uint8_t)bytes[c];
    }
}

inline bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

}  // namespace

extern "C" {

int lf_canvas_tiles_u8(uint8_t* out, int n, int oh, int ow, const int32_t* plan, const int32_t* plan_host,
                       size_t plan_ints, int n_tiles, int n_shades, int fill, lf_stream_t stream) {
    LF_REQUIRE(out && plan && plan_host, "lf_canvas_tiles: null buffer");
    LF_REQUIRE(n > 0 && oh > 0 && ow > 0, "lf_canvas_tiles: bad dims n=%d oh=%d ow=%d", n, oh, ow);
    LF_REQUIRE(n_tiles >= 0 && n_tiles <= kMaxTiles && n_shades >= 0 && n_shades <= kMaxShades,
               "lf_canvas_tiles: %d tiles, %d shades (at most %d and %d)", n_tiles, n_shades, kMaxTiles, kMaxShades);
    LF_REQUIRE((fill & ~0xffffff) == 0, "lf_canvas_tiles: fill is not 0xBBGGRR");
    const size_t head = (size_t)n_tiles * kTileInts + (size_t)n_shades * kShadeInts;
    LF_REQUIRE(plan_ints >= head && plan_ints < ((size_t)1 << 31), "lf_canvas_tiles: plan of %zu ints", plan_ints);
    bool vec = ow % 4 == 0 && aligned4(out);
    for (int t = 0; t < n_tiles; ++t) {
        const int32_t* d = plan_host + (size_t)t * kTileInts;
        const int dx = d[0], dy = d[1], dw = d[2], dh = d[3], sh = d[4], sw = d[5], ch = d[6];
        LF_REQUIRE(dw > 0 && dh > 0 && dx >= 0 && dy >= 0 && (long long)dx + dw <= ow && (long long)dy + dh <= oh,
                   "lf_canvas_tiles: tile %d (%d, %d, %d x %d) does not lie in the %d x %d canvas", t, dx, dy, dw, dh,
                   ow, oh);
        LF_REQUIRE(sh > 0 && sw > 0 && sh <= 32768 && sw <= 32768 && (ch == 1 || ch == 3),
                   "lf_canvas_tiles: source %d of %d x %d x %d", t, sh, sw, ch);
        LF_REQUIRE(d[9] != 0 || d[10] != 0, "lf_canvas_tiles: source %d is a null pointer", t);
        for (int u = 0; u < t; ++u) {
            const int32_t* o = plan_host + (size_t)u * kTileInts;
            LF_REQUIRE(dx >= o[0] + o[2] || o[0] >= dx + dw || dy >= o[1] + o[3] || o[1] >= dy + dh,
                       "lf_canvas_tiles: tiles %d and %d overlap", u, t);
        }
        // each axis table lies behind the head of the plan, and its taps lie in the source
        const int tab[2] = {d[7], d[8]}, len[2] = {dw, dh}, lim[2] = {sw, sh};
        for (int a = 0; a < 2; ++a) {
            LF_REQUIRE(tab[a] >= 0 && (size_t)tab[a] >= head && (size_t)tab[a] + 2 * (size_t)len[a] <= plan_ints,
                       "lf_canvas_tiles: a table of tile %d does not lie in the plan", t);
            for (int i = 0; i < len[a]; ++i) {
                const int i0 = plan_host[tab[a] + 2 * i], k1 = plan_host[tab[a] + 2 * i + 1];
                LF_REQUIRE(i0 >= 0 && i0 < lim[a] && k1 >= 0 && k1 <= kWeightOne,
                           "lf_canvas_tiles: entry %d of a table of tile %d (tap %d of %d, weight %d)", i, t, i0,
                           lim[a], k1);
            }
        }
        const bool copy = (d[11] & kFlagCopy) != 0;
        LF_REQUIRE((d[11] & ~kFlagCopy) == 0, "lf_canvas_tiles: flags of tile %d", t);
        LF_REQUIRE(!copy || (sh == dh && sw == dw && ch == 3 && sw % 4 == 0 && d[9] % 4 == 0),
                   "lf_canvas_tiles: tile %d is flagged a copy but is not its source's size in whole dwords", t);
        vec = vec && dx % 4 == 0 && dw % 4 == 0;
    }
    for (int s = 0; s < n_shades; ++s) {
        const int32_t* d = plan_host + (size_t)n_tiles * kTileInts + (size_t)s * kShadeInts;
        LF_REQUIRE(d[2] >= 0 && d[3] >= 0 && d[0] > -(1 << 24) && d[0] < (1 << 24) && d[1] > -(1 << 24) &&
                       d[1] < (1 << 24) && d[2] < (1 << 24) && d[3] < (1 << 24),
                   "lf_canvas_tiles: shade %d (%d, %d, %d x %d)", s, d[0], d[1], d[2], d[3]);
        LF_REQUIRE(d[5] > 0 && d[4] >= 0 && d[4] <= d[5] && d[5] <= (1 << 16),
                   "lf_canvas_tiles: shade %d is %d / %d (0 <= num <= den <= 65536)", s, d[4], d[5]);
    }
    const size_t groups_per_image = (size_t)oh * ow / (vec ? 4 : 1);
    const size_t groups = groups_per_image * n;
    LF_REQUIRE(groups_per_image < ((size_t)1 << 31) && (groups + kBlock - 1) / kBlock < ((size_t)1 << 31),
               "lf_canvas_tiles: batch of %d canvases of %d x %d is too large", n, oh, ow);
    const unsigned blocks = (unsigned)((groups + kBlock - 1) / kBlock);
    auto kernel = vec ? canvas_tiles_kernel<4> : canvas_tiles_kernel<1>;
    kernel<<<blocks, kBlock, 0, lf::as_stream(stream)>>>(out, n, oh, ow, plan, n_tiles, n_shades, (unsigned)fill,
                                                         (unsigned)groups_per_image);
    return lf::check_launch("lf_canvas_tiles");
}

}  // extern "C"
