// Internal helpers shared by the libleafhip translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "leafhip.h"

namespace lf {

void set_error(const char* fmt, ...);
void clear_error();

inline hipStream_t as_stream(lf_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// After a kernel launch: translate a HIP launch error into the ABI's error code.
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return LF_ERR_LAUNCH;
    }
    return LF_OK;
}

#define LF_REQUIRE(cond, ...)        \
    do {                             \
        if (!(cond)) {               \
            lf::set_error(__VA_ARGS__); \
            return LF_ERR_INVALID;   \
        }                            \
    } while (0)

// Grid for a grid-stride streaming kernel: enough workgroups to fill 256 CUs a few
// times over, capped (guide §6 G11).
inline unsigned stream_grid(size_t work_items, unsigned block, unsigned cap = 256u * 8u) {
    size_t g = (work_items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// Byte-moving kernels run one short pass per thread on the largest grid that fits
// (measured on MI355X, 4096 x 224x224x3: a 2048-workgroup grid-stride copy moves
// 5.1 TB/s, one 16-byte item per thread 6.1 TB/s, the same with nontemporal accesses
// 6.6 TB/s; scripts/microbench/copy_bw.hip).
constexpr unsigned kFullGrid = 1u << 30;

// Nontemporal accesses pay once the launch is larger than what the Infinity Cache would
// have kept for the next kernel anyway (256 MiB); below that plain accesses win
// (ping-pong copy of 512 images: 7.0 TB/s plain, 6.3 TB/s nontemporal).
inline bool streaming(size_t bytes_touched) { return bytes_touched >= ((size_t)256 << 20); }

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Q8.8 Gaussian taps as a kernel argument (they live in scalar registers), and the i8-MFMA blur
// (lf_blur_mfma.hip) that lf_gauss_blur_u8 tries first.
struct BlurTaps {
    uint16_t k[32];
};
bool blur_mfma_launch(const uint8_t* in, uint8_t* out, int n, int h, int w, int channels,
                      const BlurTaps& taps, int ksize, hipStream_t s);
typedef float f32x4 __attribute__((ext_vector_type(4)));

// One bf16 convolution, as both of its kernels take it: the streaming one (lf_conv_bf16s.hip: Cin, Cout <= 64,
// filter bank resident in LDS, one statistics partial per workgroup) and the K-chunked one (lf_conv_bf16.hip:
// everything else, one partial per tile).  conv_bf16_launch (lf_conv_bf16.hip) fills it and picks the kernel.
struct ConvBf16Args {
    const void* x;            // fp32 or bf16 NCHW (template XBF)
    const uint16_t* wprep;    // bf16 [ceil(cin/16)][taps][cout][16]
    void* y;                  // bf16 NCHW; the K-chunked kernel also stores fp32 (template YBF)
    int n, cin, h, w, cout;
    const float* in_scale;    // optional prologue relu?(x*scale+shift)
    const float* in_shift;
    int in_relu;
    // optional epilogue on the fp32 accumulators before rounding: v*out_scale[co]+out_shift[co], then ReLU if
    // out_relu — inference: the layer's folded BatchNorm(+ReLU), so that what is stored is the activation itself
    const float* out_scale;
    const float* out_shift;
    int out_relu;
    // ---- training epilogue (the output is bf16 and what is summed is the ROUNDED value, i.e. exactly what later
    // kernels read back):
    int accumulate;            // y = bf16(conv + y_old) (input-gradient of a block with two consumers)
    // per (output channel, partial) sums -> stat_part[(co * stat_tiles + partial) * 2 + {0,1}], a partial being a
    // workgroup tile (K-chunked kernel) or a workgroup (streaming kernel); the terms are stat_accumulate()'s:
    //   stat_mask_y == null: BatchNorm FORWARD statistics {sum d, sum d*d}, d = y - stat_pivot[co];
    //   else BatchNorm-BACKWARD sums of the BN this gradient feeds: d = y * [mask_y*mask_scale[co] +
    //   mask_shift[co] > 0 or !mask_relu] -> {sum d, sum d*mask_y}
    float* stat_part;          // or null
    const float* stat_pivot;   // may be null (pivot 0)
    long long stat_tiles;      // partials per channel: n * tiles per image, or the streaming grid
    const uint16_t* stat_mask_y;
    const float* mask_scale;
    const float* mask_shift;
    int mask_relu;
    // inference, optional, streaming kernel only: per (image, segment) channel sums of the STORED values (what a
    // global-average pool of the stored activation adds up): unit_sums[(n * segments_per_image + segment) * cout + co]
    float* unit_sums;
    // filled by launch_conv_bf16 (K-chunked kernel)
    int chunks, chunks16;     // staged chunks (32 channels); 16-channel slices of wprep
    // filled by conv_bf16s_launch (streaming kernel)
    int tiles_x, tiles_y;
    int seg_tiles, segs;      // a column strip is walked in `segs` segments of `seg_tiles` tiles (see conv_bf16s_kernel)
    int interleave;           // 1: an image's strips on one XCD (see conv_bf16s_kernel)
};
// arguments of the bf16 weight-gradient kernel (lf_wgrad_bf16.hip)
struct WgradBf16Args {
    const uint16_t* x;   // [N][Cin][H][W] bf16 (STEM: const float*, fp32 [N][Cin][H][W])
    const uint16_t* g;   // [N][Cout][H][W] bf16: dY itself, or the upstream gradient when bn_y is set
    float* part;         // [splits][Cin][TAPS][Cout]
    const float* in_scale;  // optional prologue on A: relu?(x*scale[ci]+shift[ci])
    const float* in_shift;
    int in_relu;
    int n, cin, cout, h, w;
    int tiles_x, tiles_y;
    int seg_tiles, segs;   // a column strip is walked in `segs` segments of `seg_tiles` tiles (wgrad_bf16_kernel)
    int interleave;        // 1: an image's strips on one XCD
    // optional: dY = BatchNorm backward of g (BN input bn_y), formed while staging:
    //   dz = (g*alpha[n][co] + add[n][co]) * [bn_y*coef0[co] + coef1[co] > 0 or !bn_relu]
    //   dY = bf16(coef2[co]*dz + coef3[co]*bn_y + coef4[co])
    // and written to dy_out (may be null) by the ci-block-0 workgroups, each element once
    const uint16_t* bn_y;
    const float* bn_alpha;
    const float* bn_add;
    const float* bn_coef;  // [5][Cout]
    uint16_t* dy_out;
    int bn_relu;
};

// The streaming kernel's plan for a shape: the instantiation <CI, NCO, TW, TH> (xbf: bf16 input, c16: one
// 16-channel output block instead of nco 32-channel ones) and how the grid of `wgs` workgroups walks the column
// strips.  ok = false: the shape is not covered.
struct ConvBf16sPlan {
    bool ok;
    int xbf, c16;
    int ci, nco, tw, th, tiles_x, tiles_y, seg_tiles, segs, wgs, interleave;
};
ConvBf16sPlan conv_bf16s_plan(int n, int cin, int h, int w, int cout, int ksize, int x_bf16);
int conv_bf16s_launch(ConvBf16Args a, const ConvBf16sPlan& pl, int ksize, hipStream_t s);
// the streaming kernel reads y back (read-modify-write epilogue) when it accumulates or gathers mask sums
inline bool conv_bf16s_rmw(int accumulate, bool mask) { return accumulate || mask; }

// Weight-gradient slabs part[splits][count] -> dst = beta*dst + their sum, in a fixed order (deterministic, no float
// atomics): more than kSlabGroup slabs are first summed in groups of kSlabGroup into the `slab_groups` slabs that
// follow them in the workspace.  slab_reduce_kernel lives in lf_wgrad.hip.
constexpr int kSlabGroup = 32;
inline int slab_groups(int splits) { return (splits + kSlabGroup - 1) / kSlabGroup; }
inline int slab_stages(int splits) { return splits > kSlabGroup ? 2 : 1; }
void reduce_slabs(float* part, float* dst, size_t count, int splits, float beta, hipStream_t s);

// How conv_bf16s_kernel and wgrad_bf16_kernel deal out units of work (segments of column strips, `units_per_image`
// to each of n images) to `wgs` workgroups: round-robin over the grid, or with `interleave` image i on XCD i % 8
// (workgroups k, k + 8, ... run on XCD k and take that XCD's units in order).  Workgroup wg walks units
// first, first + step, ... < total of its sequence (the grid's, or its XCD's); lf::StripWalk decodes them.
struct StripShare {
    int total, first, step, units;
};
__host__ __device__ inline StripShare strip_share(int n, int units_per_image, int wgs, int interleave, int wg) {
    const int xk = wg & 7;
    StripShare s;
    s.total = interleave ? (n > xk ? (n - xk + 7) / 8 : 0) * units_per_image : n * units_per_image;
    s.first = interleave ? wg >> 3 : wg;
    s.step = interleave ? wgs >> 3 : wgs;
    s.units = (s.step > 0 && s.total > s.first) ? (s.total - s.first + s.step - 1) / s.step : 0;
    return s;
}
// The most units one workgroup walks: workgroup 0 walks the most.
inline int max_units_per_workgroup(int n, int units_per_image, int wgs, int interleave) {
    return strip_share(n, units_per_image, wgs, interleave, 0).units;
}

// Column strips are cut into segments (which re-stage the two rows above them) only when `strips` of them are fewer
// than the `want` units that fill the chip, and never into segments of fewer than four tiles.
inline void strip_segments(int strips, int want, int tiles_y, int* seg_tiles, int* segs) {
    int s = (want + strips - 1) / strips;
    const int max_segs = (tiles_y + 3) / 4;        // at least four tiles to a segment
    if (s > max_segs) s = max_segs;
    if (s < 1) s = 1;
    *seg_tiles = (tiles_y + s - 1) / s;
    *segs = (tiles_y + *seg_tiles - 1) / *seg_tiles;
}

// Tile kernels whose neighbouring tiles share input halos: workgroups are dealt to the eight XCDs
// round-robin in dispatch order and every XCD has its own L2, so a plain (tile_x, tile_y, image)
// grid puts horizontally adjacent tiles under different L2s and every halo line is fetched from
// HBM once per XCD that touches it.  These kernels launch a 1-D grid of 8*ceil(total/8) workgroups
// and give XCD k the k-th contiguous eighth of the tiles (x fastest, then y, then image).
inline unsigned xcd_grid(size_t total_tiles) { return (unsigned)(8 * ((total_tiles + 7) / 8)); }

#if defined(__HIPCC__)
struct TileId {
    int tx, ty, n;
    bool ok;
};
// the tile this workgroup of an xcd_grid(total) launch acts as; ids >= total have no tile
__device__ __forceinline__ unsigned xcd_tile_id(unsigned total) {
    const unsigned per_xcd = (total + 7) / 8, b = blockIdx.x;
    return (b & 7u) * per_xcd + (b >> 3);
}
__device__ __forceinline__ TileId xcd_tile(int tiles_x, int tiles_y, int n_images) {
    const unsigned per_image = (unsigned)(tiles_x * tiles_y), total = per_image * (unsigned)n_images;
    const unsigned id = xcd_tile_id(total);
    TileId t;
    t.ok = id < total;
    t.n = (int)(id / per_image);
    const unsigned rem = id - (unsigned)t.n * per_image;
    t.ty = (int)(rem / (unsigned)tiles_x);
    t.tx = (int)(rem - (unsigned)t.ty * (unsigned)tiles_x);
    return t;
}

// The same for kernels on a (blocks, images) grid whose neighbouring blocks read neighbouring
// source lines (gathers along rotated / sheared rows): the block a workgroup should act as.
struct Block2 {
    unsigned x, y;
};
// the core: workgroup b (flat, in dispatch order) of `total` acts as block xcd_flat(b, total), which gives XCD k
// the k-th contiguous share of the blocks whatever total % 8 is
__device__ __forceinline__ unsigned xcd_flat(unsigned b, unsigned total) {
    const unsigned k = b & 7u, fl = total >> 3, rm = total & 7u;
    return k * fl + (k < rm ? k : rm) + (b >> 3);
}
__device__ __forceinline__ Block2 xcd_block2() {
    const unsigned gx = gridDim.x;
    const unsigned id = xcd_flat(blockIdx.x + gx * blockIdx.y, gx * gridDim.y);
    Block2 r;
    r.y = id / gx;
    r.x = id - r.y * gx;
    return r;
}
// and on a 3-D grid (the tile kernels of the convolutions: tile, channel group, image)
struct Block3 {
    int x, y, z;
};
__device__ __forceinline__ Block3 xcd_block3() {
    const unsigned gx = gridDim.x, gxy = gx * gridDim.y;
    const unsigned id = xcd_flat(blockIdx.x + gx * (blockIdx.y + gridDim.y * blockIdx.z), gxy * gridDim.z);
    Block3 r;
    r.z = (int)(id / gxy);
    r.y = (int)((id - (unsigned)r.z * gxy) / gx);
    r.x = (int)(id - (unsigned)r.z * gxy - (unsigned)r.y * gx);
    return r;
}
// and on a (splits, gy, gz) grid of split-K kernels (the fp32 weight gradients), whose gy * gz channel blocks
// of one split stage the same items: x is the split, and the channel block is the fastest part of the logical
// id, so the blocks of a split are neighbours in one XCD's dispatch sequence and run there side by side
__device__ __forceinline__ Block3 xcd_split_block3() {
    const unsigned gx = gridDim.x, gy = gridDim.y, per = gy * gridDim.z;
    Block3 r;
    if (per == 1) {  // one channel block: nothing to share, the splits keep their blockIdx order
        r.x = (int)blockIdx.x;
        r.y = r.z = 0;
        return r;
    }
    const unsigned id = xcd_flat(blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z), gx * per);
    r.x = (int)(id / per);
    const unsigned c = id - (unsigned)r.x * per;
    r.z = (int)(c / gy);
    r.y = (int)(c - (unsigned)r.z * gy);
    return r;
}

// One workgroup's walk over segments of column strips (a strip = a tile's width of columns of one image, a segment
// = seg_tiles consecutive tiles of it, top to bottom; `segs` segments to a strip), dealt out as strip_share() says.
struct StripUnit {
    int n, strip, t_first, t_count;  // image, strip of the image, first tile of the segment, its tiles
    int rem;                         // the segment's index inside its image: segment * tiles_x + strip
};
struct StripWalk {
    int units;  // what this workgroup walks: unit(0) .. unit(units - 1)
    __device__ __forceinline__ StripWalk(int n, int tiles_x, int tiles_y, int seg_tiles, int segs, int interleave)
        : tiles_x_(tiles_x), tiles_y_(tiles_y), seg_tiles_(seg_tiles), per_image_(tiles_x * segs),
          interleave_(interleave != 0) {
        const StripShare s = strip_share(n, per_image_, (int)gridDim.x, interleave_, (int)blockIdx.x);
        units = s.units;
        first_ = s.first;
        step_ = s.step;
    }
    __device__ __forceinline__ StripUnit unit(int ui) const {
        const int q = first_ + ui * step_;
        const int im = q / per_image_, seg = (q - im * per_image_) / tiles_x_;
        StripUnit u;
        u.rem = q - im * per_image_;
        u.n = interleave_ ? im * 8 + (int)(blockIdx.x & 7) : im;
        u.strip = u.rem - seg * tiles_x_;
        u.t_first = seg * seg_tiles_;
        u.t_count = min(seg_tiles_, tiles_y_ - u.t_first);
        return u;
    }

private:
    int tiles_x_, tiles_y_, seg_tiles_, per_image_, first_, step_;
    bool interleave_;
};

// Kernels that take images of different sizes in one launch number their units of work through all images: the
// last of n items whose first unit, start_of(item), is not past g (the starts ascend from start_of(0) <= g).
template <typename Start>
__device__ __forceinline__ int last_item_not_past(int n, long long g, Start start_of) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if ((long long)start_of(m) <= g)
            lo = m;
        else
            hi = m - 1;
    }
    return lo;
}

// bf16 held as uint16_t: widen exactly, and round to nearest even
__device__ __forceinline__ float bf16_up(unsigned bits16) { return __uint_as_float(bits16 << 16); }
__device__ __forceinline__ uint16_t bf16_down(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// two floats -> one dword of bf16 (lo in the low half), round to nearest even
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 v;
    v.x = (__bf16)lo;
    v.y = (__bf16)hi;
    return __builtin_bit_cast(unsigned, v);
}

// DPP sums: over each 16-lane row (every lane of the row holds the row sum), and over the 32 lanes of each wave
// half (the total lands in lanes 16-31 / 48-63)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float v) {
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, true));
}
__device__ __forceinline__ float row_sum16(float v) {
    v += dpp_move<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
    v += dpp_move<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
    v += dpp_move<0x141, 0xf>(v);  // row_half_mirror
    v += dpp_move<0x140, 0xf>(v);  // row_mirror: every lane of a 16-lane row holds the row sum
    return v;
}
__device__ __forceinline__ float half_sum32(float v) {
    v = row_sum16(v);
    v += dpp_move<0x142, 0xa>(v);  // row_bcast15 into rows 1 and 3
    return v;
}

// One term of the statistics a convolution epilogue gathers for the BatchNorm next to it (what
// lf_bn_train_stats_tiles_f32 / lf_bn_bwd_sums_tiles_f32 read), v being the output value as stored:
//   forward (masked = false): d = v - pivot                                      -> a += d, b += d*d
//   backward (masked):        d = v * [!mask_relu or y_mask*msc + msh > 0]       -> a += d, b += d*y_mask
// A pixel outside the image (in_image = false) adds d = 0.
__device__ __forceinline__ void stat_accumulate(float v, bool in_image, bool masked, float pivot, float y_mask,
                                                float msc, float msh, int mask_relu, float& a, float& b) {
    const bool on = in_image && (!mask_relu || fmaf(y_mask, msc, msh) > 0.f);
    const float d = masked ? (on ? v : 0.f) : (in_image ? v - pivot : 0.f);
    a += d;
    b = fmaf(d, masked ? y_mask : d, b);
}

// ---- pieces of the bf16 convolution kernels (lf_conv_bf16.hip, lf_conv_bf16s.hip, lf_wgrad_bf16.hip).  None holds a
// barrier or a wait of its own, and all take the kernel's own pointers and arrays: where the waves meet stays in
// the kernels.

// element e of a vector of dwords that each hold two bf16 (the lower-indexed one in the low half), widened
template <typename W>
__device__ __forceinline__ float bf16_at(const W& w, int e) {
    return bf16_up((e & 1) ? w[e / 2] >> 16 : w[e / 2] & 0xffffu);
}
// and all G of them (v: float[G] or a float vector)
template <int G, typename W, typename V>
__device__ __forceinline__ void unpack_bf16(const W& w, V& v) {
#pragma unroll
    for (int e = 0; e < G; e += 2) {
        v[e] = bf16_up(w[e / 2] & 0xffffu);
        v[e + 1] = bf16_up(w[e / 2] >> 16);
    }
}

// the fused prologue of a convolution input: the producer's BatchNorm (+ReLU) on one value
__device__ __forceinline__ float pro_apply(float v, float sc, float sh, int relu) {
    v = fmaf(v, sc, sh);
    return relu ? fmaxf(v, 0.f) : v;
}

// BatchNorm backward on one element (lf_nn.hip's kernels, and the weight gradients that form dY while staging):
//   dz = (g*al + ad) * [y*sc + sh > 0 or !relu]
// the ReLU mask is recomputed from y with the forward's own fmaf, so the activation tensor is never materialised:
// fmaf(y, sc, sh) > 0 here and fmaf(y, c0, c1) > 0 below are that fmaf, (c0, c1) being the BN's (scale, shift).
__device__ __forceinline__ float bn_dz1(float g, float y, float al, float ad, float sc, float sh, int relu) {
    float dz = fmaf(g, al, ad);
    if (relu && !(fmaf(y, sc, sh) > 0.f)) dz = 0.f;
    return dz;
}
//   dY = c2*dz + c3*y + c4, c0..c4 being the channel's column of the [5][C] coefficient block
__device__ __forceinline__ float bn_dy1(float g, float y, float al, float ad, float c0, float c1, float c2, float c3,
                                        float c4, int relu) {
    return fmaf(c2, bn_dz1(g, y, al, ad, c0, c1, relu), fmaf(c3, y, c4));
}

// Staging four channels x G pixels as [pixel][channel] bf16: raw[i] = channel i's G pixels as loaded; ok = false:
// outside the image, which stays exactly zero.  transform(i, v) works on channel i's G fp32 values; every second
// channel the pair (i - 1, i) leaves as store(e, pair, dword), one dword per pixel e — channel by channel, so that
// few values are live at a time.
template <int G, typename W, typename Transform, typename Store>
__device__ __forceinline__ void stage_quad(const W (&raw)[4], bool ok, Transform transform, Store store) {
    float prev[G];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v[G];
#pragma unroll
        for (int e = 0; e < G; ++e) v[e] = 0.f;
        if (ok) {
            unpack_bf16<G>(raw[i], v);
            transform(i, v);
        }
        if (i & 1) {
#pragma unroll
            for (int e = 0; e < G; ++e) store(e, i >> 1, pack_bf16(prev[e], v[e]));
        } else {
#pragma unroll
            for (int e = 0; e < G; ++e) prev[e] = v[e];
        }
    }
}
// Its twin for the halo columns: four channels of ONE pixel -> the pixel's two dwords.  widen(i) = channel i's value,
// transform(i, v) as above with v a float[1].
template <typename Widen, typename Transform>
__device__ __forceinline__ u32x2 stage_halo_quad(bool ok, Widen widen, Transform transform) {
    float v[4][1] = {{0.f}, {0.f}, {0.f}, {0.f}};
    if (ok) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i][0] = widen(i);
#pragma unroll
        for (int i = 0; i < 4; ++i) transform(i, v[i]);
    }
    u32x2 o;
    o.x = pack_bf16(v[0][0], v[1][0]);
    o.y = pack_bf16(v[2][0], v[3][0]);
    return o;
}

// The epilogue of a thread that finishes EIGHT consecutive pixels of one output channel (16 bytes of bf16), the
// accumulators having gone through a transpose buffer in LDS.
// row8_request: the read-modify-write operand rows of the thread's channels co0 + 32 * cb + 8 * j + ec (j < NJ:
// four rows of 8 channels to a 32-channel block, two to a 16-channel one), eight pixels at offset po of each
// channel plane of `image` — asked for before the MFMAs, used after them.
template <int NCB, int NJ>
__device__ __forceinline__ void row8_request(u32x4 (&r)[NCB][NJ], const uint16_t* image, int co0, int ec, size_t hw,
                                             size_t po) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            r[cb][j] = *reinterpret_cast<const u32x4*>(image + (size_t)(co0 + cb * 32 + 8 * j + ec) * hw + po);
}
// row8_finish: acc8 = the eight fp32 accumulators (16-byte aligned LDS) -> (+ old) -> (* *osc + *osh, read only
// when scaled) -> ReLU -> bf16
__device__ __forceinline__ u32x4 row8_finish(const float* acc8, bool accumulate, const u32x4& old, bool scaled,
                                             const float* osc, const float* osh, int relu) {
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(acc8);
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(acc8 + 4);
    float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    if (accumulate)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bf16_at(old, e);
    if (scaled) {
        const float sc = *osc, sh = *osh;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaf(v[e], sc, sh);
    }
    if (relu)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 8; e += 2) o[e / 2] = pack_bf16(v[e], v[e + 1]);
    return o;
}
// row8_sums: the eight stat_accumulate terms of the ROUNDED values o, all inside the image: forward terms about
// *pivot (null: 0), or (masked) backward terms under the mask rows `mask_words` with mask scale *msc and shift *msh.
// Only the kind's own constants are read.  (One loop per kind of sum: the kind is uniform, the loops are unrolled.)
__device__ __forceinline__ void row8_sums(const u32x4& o, bool masked, const float* pivot, const float* msc,
                                          const float* msh, const u32x4& mask_words, int mask_relu, float& a,
                                          float& b) {
    if (!masked) {
        const float pv = pivot != nullptr ? *pivot : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) stat_accumulate(bf16_at(o, e), true, false, pv, 0.f, 0.f, 0.f, 0, a, b);
    } else {
        const float sc = *msc, sh = *msh;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            stat_accumulate(bf16_at(o, e), true, true, 0.f, bf16_at(mask_words, e), sc, sh, mask_relu, a, b);
    }
}

// Statistics partials of a workgroup: red[WAVES][CT][2] (one partial per wave and channel of the workgroup's CT
// channels from co0 on) -> stat_part[(co * stat_tiles + partial) * 2 + {0,1}], the waves added in order from the
// left (deterministic).  The caller's barrier stands between the writes of `red` and this.
template <int WAVES, int CT>
__device__ __forceinline__ void write_stat_part(float* stat_part, long long stat_tiles, int cout, long long partial,
                                                int co0, const float* red, int tid, int threads) {
    for (int c = tid; c < CT; c += threads) {
        if (co0 + c >= cout) continue;
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int wp = 0; wp < WAVES; ++wp) {
            a += red[(wp * CT + c) * 2];
            b += red[(wp * CT + c) * 2 + 1];
        }
        float* dst = stat_part + ((size_t)(co0 + c) * (size_t)stat_tiles + (size_t)partial) * 2;
        dst[0] = a;
        dst[1] = b;
    }
}

template <bool NT, typename T>
__device__ __forceinline__ T ldg(const T* p) {
    return NT ? __builtin_nontemporal_load(p) : *p;
}
template <bool NT, typename T>
__device__ __forceinline__ void stg(T* p, T v) {
    if (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}
#endif

}  // namespace lf
