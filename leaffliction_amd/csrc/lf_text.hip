// lf_draw_text_u8: strings of the project's 5x7 bitmap font (lf_font5x7.h) drawn into [N][H][W][3] uint8 pictures,
// all strings of all images in one launch, and lf_font5x7, the host's view of the same table.  The pixel rule is
// stated in include/leafhip.h ("Text"); tests/text_ref.py restates it in numpy.
//
// A workgroup of 256 threads takes 256 consecutive pixels (row-major) of one string's UNCLIPPED box of
// 6*scale*length x 7*scale pixels; the item table carries each string's first workgroup (a running sum the
// launcher checks), and a workgroup finds its string by bisection.  A lane whose pixel the string paints looks
// through the LATER strings of the same image (the table is ordered by image, so they follow it directly) and
// stores only if none of them paints that pixel too: every pixel has exactly one writer, the last string of the
// table that paints it, whatever order the hardware runs the workgroups in.  No atomics, no LDS, integer arithmetic.
#include "lf_common.h"
#include "lf_font5x7.h"

namespace {

constexpr int kBlock = 256;
constexpr int kItemInts = 8;   // lf_text_item: image, x, y, first char, length, colour, scale, first workgroup
constexpr int kMaxScale = 8;
constexpr int kMaxLength = 4096;

__constant__ uint8_t d_font[LF_FONT5X7_BYTES] = LF_FONT5X7_ROWS;
const uint8_t h_font[LF_FONT5X7_BYTES] = LF_FONT5X7_ROWS;

struct TextItem {
    int image, x, y, first, length, colour, scale, block;
};

__device__ __forceinline__ TextItem load_item(const int32_t* __restrict__ items, int i) {
    const int32_t* p = items + (size_t)i * kItemInts;
    TextItem t;
    t.image = p[0];
    t.x = p[1];
    t.y = p[2];
    t.first = p[3];
    t.length = p[4];
    t.colour = p[5];
    t.scale = p[6];
    t.block = p[7];
    return t;
}

// whether string t paints pixel (px, py): the rule of include/leafhip.h, word for word
__device__ __forceinline__ bool paints(const TextItem& t, const uint8_t* __restrict__ chars, int px, int py) {
    const int k = t.scale, cell = 6 * k;
    const int u = px - t.x, v = py - t.y;
    if (v < 0 || v >= 7 * k || u < 0 || u >= cell * t.length) return false;
    const int ci = u / cell, col = (u - ci * cell) / k;
    if (col >= 5) return false;
    int c = chars[t.first + ci];
    if (c < LF_FONT5X7_FIRST || c >= LF_FONT5X7_FIRST + LF_FONT5X7_GLYPHS) c = '?';
    return (d_font[(c - LF_FONT5X7_FIRST) * 7 + v / k] >> (4 - col)) & 1;
}

__global__ __launch_bounds__(kBlock) void draw_text_kernel(uint8_t* __restrict__ img, int H, int W,
                                                           const int32_t* __restrict__ items, int n_items,
                                                           const uint8_t* __restrict__ chars) {
    const int b = (int)blockIdx.x;
    const int i = lf::last_item_not_past(n_items, b, [&](int m) { return items[(size_t)m * kItemInts + 7]; });
    const TextItem t = load_item(items, i);
    const int bw = 6 * t.scale * t.length;             // the box; an empty string owns no workgroup
    const int idx = (b - t.block) * kBlock + (int)threadIdx.x;
    if (bw <= 0 || idx >= bw * 7 * t.scale) return;
    const int v = idx / bw, u = idx - v * bw;
    const int px = t.x + u, py = t.y + v;
    if (px < 0 || px >= W || py < 0 || py >= H) return;   // pixels outside the image are dropped
    if (!paints(t, chars, px, py)) return;
    for (int j = i + 1; j < n_items; ++j) {               // the later strings of this image
        const TextItem o = load_item(items, j);
        if (o.image != t.image) break;
        if (paints(o, chars, px, py)) return;             // that string's own lane writes the pixel
    }
    uint8_t* p = img + (((size_t)t.image * H + py) * W + px) * 3;
    p[0] = (uint8_t)(t.colour & 0xff);
    p[1] = (uint8_t)((t.colour >> 8) & 0xff);
    p[2] = (uint8_t)((t.colour >> 16) & 0xff);
}

}  // namespace

extern "C" {

int lf_font5x7(uint8_t* out) {
    LF_REQUIRE(out, "lf_font5x7: null buffer");
    for (int i = 0; i < LF_FONT5X7_BYTES; ++i) out[i] = h_font[i];
    return LF_OK;
}

int lf_draw_text_u8(uint8_t* img, int n, int h, int w, const int32_t* items, const int32_t* items_host, int n_items,
                    const uint8_t* chars, size_t chars_bytes, lf_stream_t stream) {
    LF_REQUIRE(img && items && items_host && chars, "lf_draw_text: null buffer");
    LF_REQUIRE(n > 0 && h > 0 && w > 0 && n_items > 0, "lf_draw_text: bad dims n=%d h=%d w=%d items=%d", n, h, w,
               n_items);
    LF_REQUIRE((long long)n * h * w < ((long long)1 << 40), "lf_draw_text: batch of %d images of %d x %d is too large",
               n, h, w);
    long long blocks = 0;
    int last_image = 0;
    for (int i = 0; i < n_items; ++i) {
        const int32_t* p = items_host + (size_t)i * kItemInts;
        const int image = p[0], x = p[1], y = p[2], first = p[3], length = p[4], colour = p[5], scale = p[6];
        LF_REQUIRE(image >= 0 && image < n, "lf_draw_text: image %d of string %d (0..%d)", image, i, n - 1);
        LF_REQUIRE(image >= last_image, "lf_draw_text: string %d breaks the table's order by image", i);
        LF_REQUIRE(scale >= 1 && scale <= kMaxScale, "lf_draw_text: scale %d of string %d (1..%d)", scale, i,
                   kMaxScale);
        LF_REQUIRE(length >= 0 && length <= kMaxLength, "lf_draw_text: length %d of string %d (0..%d)", length, i,
                   kMaxLength);
        LF_REQUIRE(first >= 0 && (size_t)first + (size_t)length <= chars_bytes,
                   "lf_draw_text: the characters of string %d do not lie in the buffer", i);
        LF_REQUIRE(x > -(1 << 24) && x < (1 << 24) && y > -(1 << 24) && y < (1 << 24),
                   "lf_draw_text: origin (%d, %d) of string %d", x, y, i);
        LF_REQUIRE((colour & ~0xffffff) == 0, "lf_draw_text: colour of string %d is not 0xBBGGRR", i);
        LF_REQUIRE(p[7] == blocks, "lf_draw_text: first workgroup of string %d is not the running sum", i);
        const long long box = (long long)6 * scale * length * 7 * scale;
        blocks += (box + kBlock - 1) / kBlock;
        last_image = image;
    }
    LF_REQUIRE(blocks < ((long long)1 << 31), "lf_draw_text: too many pixels");
    if (blocks == 0) return LF_OK;   // empty strings only: nothing to draw
    draw_text_kernel<<<(unsigned)blocks, kBlock, 0, lf::as_stream(stream)>>>(img, h, w, items, n_items, chars);
    return lf::check_launch("lf_draw_text");
}

}  // extern "C"
