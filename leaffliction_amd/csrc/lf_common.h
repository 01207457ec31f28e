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

// The streaming kernel's plan for a shape: the instantiation <CI, NCO, TW, TH> and how the grid of `wgs` workgroups
// walks the column strips.  ok = false: the shape is not covered.
struct ConvBf16sPlan {
    bool ok;
    int ci, nco, tw, th, tiles_x, tiles_y, seg_tiles, segs, wgs, interleave;
};
ConvBf16sPlan conv_bf16s_plan(int n, int cin, int h, int w, int cout, int ksize, int x_bf16);
int conv_bf16s_launch(ConvBf16Args a, const ConvBf16sPlan& pl, int ksize, hipStream_t s);
// the streaming kernel reads y back (read-modify-write epilogue) when it accumulates or gathers mask sums
inline bool conv_bf16s_rmw(int accumulate, bool mask) { return accumulate || mask; }

// Weight-gradient slabs part[splits][count] -> dst = beta*dst + their sum, in a fixed order (deterministic, no float
// atomics): more than kSlabGroup slabs are first summed in groups of kSlabGroup into the `slab_groups` slabs that
// follow them in the workspace.  slab_reduce_kernel lives in lf_conv.hip.
constexpr int kSlabGroup = 32;
inline int slab_groups(int splits) { return (splits + kSlabGroup - 1) / kSlabGroup; }
inline int slab_stages(int splits) { return splits > kSlabGroup ? 2 : 1; }
void reduce_slabs(float* part, float* dst, size_t count, int splits, float beta, hipStream_t s);

// The most units (segments of column strips) one workgroup walks when `wgs` workgroups deal out n images of
// `units_per_image` units each as conv_bf16s_kernel and wgrad_bf16_kernel do: round-robin over the grid, or with
// `interleave` image i on XCD i % 8 (workgroups k, k + 8, ...).  Workgroup 0 walks the most.
inline int max_units_per_workgroup(int n, int units_per_image, int wgs, int interleave) {
    const long long total = interleave ? (long long)((n + 7) / 8) * units_per_image : (long long)n * units_per_image;
    const long long step = interleave ? wgs / 8 : wgs;
    return step > 0 ? (int)((total + step - 1) / step) : 0;
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
__device__ __forceinline__ Block2 xcd_block2() {
    const unsigned gx = gridDim.x, total = gx * gridDim.y;
    const unsigned b = blockIdx.x + gx * blockIdx.y;
    const unsigned k = b & 7u, fl = total >> 3, rm = total & 7u;
    const unsigned id = k * fl + (k < rm ? k : rm) + (b >> 3);
    Block2 r;
    r.y = id / gx;
    r.x = id - r.y * gx;
    return r;
}

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
