// libleafhip — conv2d forward / dgrad / wgrad as implicit GEMM on the fp32 MFMA
// (v_mfma_f32_32x32x2_f32: exact f32, bitwise an fmaf chain; 64 FLOP/clk/SIMD).
//
// Layouts: activations NCHW f32; conv weights "IKO" = [Cin][kh*kw][Cout] (the GEMM's
// K-major order, Cout contiguous).  Stride 1, "same" zero padding, no bias
// (keras Conv2D(filters, 3|1, padding="same", use_bias=False), srcs/model/cnn.py:27-29,44).
//
// Forward / dgrad, direct kernel (conv_mfma_kernel: the stem, 1x1):  D[co][pixel] = sum_k W[co][k] X[k][pixel],
//   k = (ci, tap).  A operand = weights (lane -> co), B operand = pixels (lane -> pixel),
//   so one accumulator register holds 32 consecutive pixels of one output channel and the
//   NCHW store is 128-byte contiguous per half-wave.
//   A workgroup (4 waves) owns a TWxTH pixel tile (flat-indexed 32-pixel blocks, so tile
//   shapes like 28x8 work) x CT output channels; the input patch (+halo) and the weight
//   slice for KC input channels are staged in LDS per K-chunk.  Staging uses 16-byte
//   loads (row interiors and weight rows) with every load of a chunk in flight at once, and
//   the NEXT chunk's loads are issued into registers before the current chunk's MFMAs
//   (a bounded register prefetch: <= 13 float4 per thread); 2-4 workgroups are resident per
//   CU so one workgroup's LDS write phase overlaps another's MFMAs.
//   An optional prologue applies y = relu(x*scale[c]+shift[c]) to the input while staging
//   (BatchNorm+ReLU of the producer fused into the consumer; zero padding stays zero).
// Forward / dgrad, Winograd kernel (conv_wino_kernel: every other 3x3): F(2x2,3x3) on the same
//   staged patch (v_mfma_f32_16x16x4_f32, 16 products per 2x2 outputs instead of 36; see the kernel).
//
// wgrad kernel (wgrad_mfma_kernel): dW[ci][tap][co] = sum_pixels X[ci][p+tap] dY[co][p],
//   K = pixels, split across workgroups and across the waves of a workgroup (reduced through
//   LDS); every workgroup writes one partial slab and a two-stage reduce sums the slabs in a
//   fixed order (deterministic, no float atomics).  The 3x3 layers but the stem's use wgrad3_kernel,
//   which accumulates in the Winograd F(2x2,3x3) domain instead.  wgrad_smallcin_kernel packs (ci, tap)
//   into the MFMA's M dimension for the stem (Cin*9 <= 32): one MFMA per pixel pair.
//
// proj_bwd_kernel: the backward of a projection shortcut (1x1 conv + BatchNorm) in one pass — BatchNorm backward,
//   the 1x1 weight gradient and the 1x1 input gradient share the staged dY, which never leaves the chip.
#include <type_traits>

#include "lf_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;

// Raw buffer loads: SGPR resource (base, byte size) + a 32-bit byte offset per lane; an offset
// at or beyond the size returns 0, which is how zero padding is fetched (no branches, no
// 64-bit address arithmetic per lane).
typedef float lf_f4 __attribute__((ext_vector_type(4)));
constexpr unsigned kBufOob = 0xffffffffu;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const float* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned off) {
    const lf_f4 v = __builtin_bit_cast(lf_f4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float buf_load1(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}

struct ConvArgs {
    const float* x;
    const float* w;       // [Cin][TAPS][Cout] (the direct kernel)
    const float* wino_u;  // [Cin][Cout][16], U = G g G^T of every filter (the Winograd kernel)
    float* y;
    const float* in_scale;  // optional prologue (nullptr = none)
    const float* in_shift;
    int n, cin, cout, h, wd;
    int tiles_x, tiles_y;
    int in_relu;
    int accumulate;  // y += conv(...) instead of y = conv(...)
    int vec_ok;      // W % 4 == 0, Cout % 4 == 0, 16-byte aligned bases
    // images per workgroup column (1, or 2 for the STK instantiation): with H = 28 and 8-row
    // tiles two images are walked as one 56-row strip, so no tile is half empty; the tile that
    // straddles the seam carries each image's own halo rows
    int stack;
    // optional BatchNorm statistics of the output, gathered in the epilogue: per (channel, tile)
    // sum and sum of squares of (y - pivot[co]) -> stat_part[(co * stat_tiles + tile) * 2 + {0,1}]
    float* stat_part;
    const float* stat_pivot;  // may be null (pivot 0)
    long long stat_tiles;     // n * tiles_x * tiles_y
    // with stat_mask_y (same shape as y) the epilogue gathers BatchNorm-BACKWARD sums instead:
    // d = y_out * [stat_mask_y*mask_scale[co]+mask_shift[co] > 0 or !mask_relu];
    // stat_part gets {sum d, sum d*stat_mask_y}
    const float* stat_mask_y;
    const float* mask_scale;
    const float* mask_shift;
    int mask_relu;
};

using lf::half_sum32;
using lf::pro_apply;
using lf::row_sum16;

// Winograd F(2x2,3x3) transforms (Lavin & Gray 2016): Y = A^T [(G g G^T) . (B^T d B)] A with
//   G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1], B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1],
//   A^T = [1 1 1 0; 0 1 -1 -1].
// Every coefficient is 0, +-1 or +-1/2, so small-integer data stays exact.  Index = row * 4 + col.
__device__ __forceinline__ void wino_filter(const float (&g)[9], float (&u)[16]) {
    float t[4][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float s = g[c] + g[6 + c];
        t[0][c] = g[c];
        t[1][c] = (s + g[3 + c]) * 0.5f;
        t[2][c] = (s - g[3 + c]) * 0.5f;
        t[3][c] = g[6 + c];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float s = t[r][0] + t[r][2];
        u[r * 4 + 0] = t[r][0];
        u[r * 4 + 1] = (s + t[r][1]) * 0.5f;
        u[r * 4 + 2] = (s - t[r][1]) * 0.5f;
        u[r * 4 + 3] = t[r][2];
    }
}
__device__ __forceinline__ void wino_input(const float (&d)[16], float (&v)[16]) {
    float t[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        t[0 + c] = d[0 + c] - d[8 + c];
        t[4 + c] = d[4 + c] + d[8 + c];
        t[8 + c] = d[8 + c] - d[4 + c];
        t[12 + c] = d[4 + c] - d[12 + c];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        v[r * 4 + 0] = t[r * 4 + 0] - t[r * 4 + 2];
        v[r * 4 + 1] = t[r * 4 + 1] + t[r * 4 + 2];
        v[r * 4 + 2] = t[r * 4 + 2] - t[r * 4 + 1];
        v[r * 4 + 3] = t[r * 4 + 1] - t[r * 4 + 3];
    }
}
__device__ __forceinline__ void wino_output(const float (&m)[16], float (&y)[4]) {
    float b[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        b[0][c] = m[0 + c] + m[4 + c] + m[8 + c];
        b[1][c] = m[4 + c] - m[8 + c] - m[12 + c];
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        y[r * 2 + 0] = b[r][0] + b[r][1] + b[r][2];
        y[r * 2 + 1] = b[r][1] - b[r][2] - b[r][3];
    }
}

// ---------------------------------------------------------------------------
// forward / dgrad: the pieces both kernels share, the direct kernel, the Winograd kernel
// ---------------------------------------------------------------------------
constexpr int kMaxProC = 512;  // prologue scale/shift staged in LDS for this many channels at a time

// The producer's BatchNorm scale/shift of the kMaxProC input channels from cbase on (a multiple of kMaxProC) ->
// lsc[2][kMaxProC].  The channels that fill up a ragged last K-chunk (of at most 8) get 0, 0: they stage as zeros.
__device__ __forceinline__ void stage_pro_consts(const ConvArgs& p, float* lsc, int cbase, int tid) {
    const int nc = min(((p.cin + 7) & ~7) - cbase, kMaxProC);
    for (int c = tid; c < nc; c += kThreads) {
        const bool in = cbase + c < p.cin;
        lsc[c] = in ? p.in_scale[cbase + c] : 0.f;
        lsc[kMaxProC + c] = in ? p.in_shift[cbase + c] : 0.f;
    }
}
// A launch with more input channels than that moves the window when the K-loop reaches its end: called (by every
// thread) at the top of chunk c0, in front of the chunk's first barrier.  The last readers of the old window, the
// store phase of the chunk before, finished before that chunk's second barrier; the first barrier of this one
// stands between these writes and the chunk's own store phase.
__device__ __forceinline__ void advance_pro_consts(const ConvArgs& p, float* lsc, int c0, int tid) {
    if (p.in_scale != nullptr && c0 > 0 && (c0 & (kMaxProC - 1)) == 0) stage_pro_consts(p, lsc, c0, tid);
}

// The per-channel constants a workgroup reads, staged in LDS: the prologue's first window and the epilogue's
// statistics constants of the workgroup's CT couts from co0 on (lep[3][CT]: pivot, 0 where there is none; mask
// scale; mask shift).  A kernel calls this right after it has issued chunk 0's patch loads, so the wait for these
// few L2-resident floats lies under the patch's own.  The barriers of the K-loop stand between the writes and
// every reader.
template <int CT>
__device__ __forceinline__ void stage_channel_consts(const ConvArgs& p, float* lsc, float* lep, int co0, int tid) {
    static_assert(CT <= kThreads, "at most one cout per thread");
    if (p.in_scale != nullptr) stage_pro_consts(p, lsc, 0, tid);
    if (p.stat_part != nullptr && tid < CT) {
        const int co = co0 + tid, coc = min(co, p.cout - 1);
        const bool masked = p.stat_mask_y != nullptr;
        lep[tid] = (!masked && p.stat_pivot != nullptr && co < p.cout) ? p.stat_pivot[co] : 0.f;
        lep[CT + tid] = masked ? p.mask_scale[coc] : 0.f;
        lep[2 * CT + tid] = masked ? p.mask_shift[coc] : 0.f;
    }
}

// XCD-aware order: workgroups are dealt to the eight XCDs round-robin in dispatch order (x, then y,
// then z), each XCD with its own L2.  XCD k takes the k-th contiguous share of the (tile, channel
// group, strip) space, so the tiles that share halo rows meet in one L2.  Strip rows ty0 .. ty0+TH-1:
// the first `ra` belong to image n + imgA (rows gyA0 ..), the rest (only when the tile straddles a
// seam, or hangs over the bottom) to the next image.
template <int TW, int TH, int HALO, bool STK>
struct ConvTile {
    int bz, by, tile;  // strip, cout group, tile of the strip
    int tx0, ty0, n;   // n: first image of the strip
    int imgA, gyA0, ra;
    bool imgA_ok, imgB_ok;

    __device__ __forceinline__ explicit ConvTile(const ConvArgs& p) {
        const lf::Block3 b = lf::xcd_block3();
        bz = b.z;
        by = b.y;
        tile = b.x;
        tx0 = (tile % p.tiles_x) * TW;
        ty0 = (tile / p.tiles_x) * TH;
        n = bz * p.stack;
        imgA = ty0 / p.h;
        gyA0 = ty0 - imgA * p.h;
        ra = min(TH, p.h - gyA0);
        imgA_ok = imgA < p.stack && n + imgA < p.n;
        imgB_ok = STK && imgA + 1 < p.stack && n + imgA + 1 < p.n;
    }

    // patch row -> (image, row): [0, ra+2H) image A from gyA0-H; then image B from -H
    __device__ __forceinline__ bool patch_row(int py, int h, int& img, int& gy) const {
        if (py < ra + 2 * HALO) {
            img = imgA;
            gy = gyA0 - HALO + py;
            return imgA_ok && gy >= 0 && gy < h;
        }
        img = imgA + 1;
        gy = py - (ra + 2 * HALO) - HALO;
        return imgB_ok && ra < TH && gy >= 0 && gy < h && gy < TH - ra + HALO;
    }
};

// The input patch (+halo) of one K-chunk of kKC channels in LDS ([kKC][PH][PW]), prologue applied.
// Vector staging: per patch row TW/4 float4 interior items + 2*HALO halo scalars, kept in two
// homogeneous item arrays (mixing both kinds in one array makes the compiler wait for every load
// right where it is issued).  Per-thread invariants (the workgroup has one tile; a chunk only moves
// the channel base): byte offsets from the chunk's first channel plane with kBufOob for everything
// that must read as zero (rows and columns outside the image, slots beyond the item count);
// LDS index | kc << 16.  Channels beyond Cin fall outside the chunk's buffer size -> zeros.
template <int TW, int TH, int HALO, bool STK, int kKC>
struct PatchStage {
    static constexpr int PW = TW + 2 * HALO, PH = TH + 2 * HALO + (STK ? 2 * HALO : 0), PP = PW * PH;
    static constexpr int TW4 = TW / 4;
    static constexpr int NVI = kKC * PH * TW4, IPT = (NVI + kThreads - 1) / kThreads;
    static constexpr int NHI = kKC * PH * 2 * HALO, HPT = (NHI + kThreads - 1) / kThreads;
    static_assert(TW % 4 == 0, "float4 patch rows");

    size_t hw;  // H*W
    float4 pv[IPT];
    float ph[HPT > 0 ? HPT : 1];
    unsigned pg[IPT], pl[IPT];
    unsigned hg[HPT > 0 ? HPT : 1], hl[HPT > 0 ? HPT : 1];
    unsigned okmask = 0;  // bit i: interior item i in-image; bit 16+i: halo item i in-image

    __device__ __forceinline__ PatchStage(const ConvArgs& p, const ConvTile<TW, TH, HALO, STK>& t, int tid) {
        hw = (size_t)p.h * p.wd;
        const unsigned uhw = (unsigned)hw;
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const int e = tid + i * kThreads;
            const int kc = e / (PH * TW4), rem = e - kc * (PH * TW4);
            const int py = rem / TW4, slot = rem - py * TW4;
            int img, gy;
            const bool ok = t.patch_row(py, p.h, img, gy) && e < NVI;
            pg[i] = ok ? 4u * ((unsigned)(img * p.cin + kc) * uhw + (unsigned)gy * (unsigned)p.wd + (unsigned)(t.tx0 + 4 * slot)) : kBufOob;
            pl[i] = (unsigned)(kc * PP + py * PW + HALO + 4 * slot) | ((unsigned)kc << 16);
            okmask |= (ok ? 1u : 0u) << i;
        }
#pragma unroll
        for (int i = 0; i < HPT; ++i) {
            const int e = tid + i * kThreads;
            const int kc = e / (PH * 2), rem = e - kc * (PH * 2);
            const int py = rem >> 1, side = rem & 1;
            const int gx = side ? t.tx0 + TW : t.tx0 - 1;
            int img, gy;
            const bool ok = t.patch_row(py, p.h, img, gy) && e < NHI && gx >= 0 && gx < p.wd;
            hg[i] = ok ? 4u * ((unsigned)(img * p.cin + kc) * uhw + (unsigned)gy * (unsigned)p.wd + (unsigned)gx) : kBufOob;
            hl[i] = (unsigned)(kc * PP + py * PW + (side ? PW - 1 : 0)) | ((unsigned)kc << 16);
            okmask |= (ok ? 1u : 0u) << (16 + i);
        }
    }

    // chunk c0's loads into registers (with a strip of two images the second image's chunk lies Cin
    // planes further on; the host only stacks when Cin is a whole number of chunks).  A chunk past the last one
    // would have an empty buffer: its loads fetch nothing and return zeros.
    __device__ __forceinline__ void load(const ConvArgs& p, const float* xin, int c0) {
        const int nc = min(kKC, p.cin - c0);
        const __amdgpu_buffer_rsrc_t rx = buf_rsrc(
            xin + (size_t)c0 * hw,
            nc > 0 ? 4u * (unsigned)((STK ? (p.stack - 1) * p.cin : 0) + nc) * (unsigned)hw : 0u);
#pragma unroll
        for (int i = 0; i < IPT; ++i) pv[i] = buf_load4(rx, pg[i]);
#pragma unroll
        for (int i = 0; i < HPT; ++i) ph[i] = buf_load1(rx, hg[i]);
    }

    // The registers loaded for chunk c0 -> LDS.  PRO: the launch has a prologue (the K-loop exists once for either
    // case, so the store phase has no branch on it); lsc then holds the window that contains the chunk
    // (advance_pro_consts).
    template <bool PRO, bool AHEAD = true>
    __device__ __forceinline__ void store(const ConvArgs& p, float* lp, const float* lsc, int c0, int tid) const {
        // Every item's scale and shift are read from the LDS window first: they do not depend on the patch loads,
        // so their latency lies under the counted waits for those.  An item outside the image takes 0, 0 and stays
        // zero without a branch of its own; slots beyond the item count read a clamped channel and store nothing.
        // (!AHEAD: each item's constants are read where the item is stored, for a kernel that has no registers
        // to hold them all.)
        float isc[IPT], ish[IPT], hsc[HPT > 0 ? HPT : 1], hsh[HPT > 0 ? HPT : 1];
        const int cw = c0 & (kMaxProC - 1);
        auto consts = [&](unsigned l, bool ok, float& sc, float& sh) {
            const int c = min(cw + (int)(l >> 16), kMaxProC - 1);
            const float s = lsc[c], t = lsc[kMaxProC + c];
            sc = ok ? s : 0.f;
            sh = ok ? t : 0.f;
        };
        if (PRO && AHEAD) {
#pragma unroll
            for (int i = 0; i < IPT; ++i) consts(pl[i], okmask >> i & 1u, isc[i], ish[i]);
#pragma unroll
            for (int i = 0; i < HPT; ++i) consts(hl[i], okmask >> (16 + i) & 1u, hsc[i], hsh[i]);
            // an opaque use, so that no read is moved down into the branch of a partial item, behind a wait
#pragma unroll
            for (int i = 0; i < IPT; ++i) asm volatile("" : "+v"(isc[i]), "+v"(ish[i]));
#pragma unroll
            for (int i = 0; i < HPT; ++i) asm volatile("" : "+v"(hsc[i]), "+v"(hsh[i]));
        }
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            if ((i + 1) * kThreads <= NVI || tid + i * kThreads < NVI) {  // only the last item can be partial
                float4 v = pv[i];
                if (PRO) {
                    if (!AHEAD) consts(pl[i], okmask >> i & 1u, isc[i], ish[i]);
                    v.x = pro_apply(v.x, isc[i], ish[i], p.in_relu);
                    v.y = pro_apply(v.y, isc[i], ish[i], p.in_relu);
                    v.z = pro_apply(v.z, isc[i], ish[i], p.in_relu);
                    v.w = pro_apply(v.w, isc[i], ish[i], p.in_relu);
                }
                float* dst = lp + (pl[i] & 0xffffu);
                dst[0] = v.x;
                dst[1] = v.y;
                dst[2] = v.z;
                dst[3] = v.w;
            }
        }
#pragma unroll
        for (int i = 0; i < HPT; ++i) {
            if ((i + 1) * kThreads <= NHI || tid + i * kThreads < NHI) {
                float v = ph[i];
                if (PRO && !AHEAD) consts(hl[i], okmask >> (16 + i) & 1u, hsc[i], hsh[i]);
                if (PRO) v = pro_apply(v, hsc[i], hsh[i], p.in_relu);
                lp[hl[i] & 0xffffu] = v;
            }
        }
    }

    // Scalar staging (ragged shapes / partial tiles), loads straight to LDS: a thread owns one patch
    // position (two when the patch has more than 256) and walks the chunk's channels: every load is
    // base + c*H*W
    static __device__ __forceinline__ void stage_scalar(const ConvArgs& p, float* lp, const float* xin,
                                                        int tx0, int ty0, int c0, int tid) {
        constexpr int SLOTS = PP <= 64 ? 64 : (PP <= 128 ? 128 : 256);
        constexpr int G = kThreads / SLOTS;
        constexpr int ROUNDS = (PP + SLOTS - 1) / SLOTS;
        const int slot = tid % SLOTS, grp = tid / SLOTS;
        const size_t hw = (size_t)p.h * p.wd;
        const unsigned uhw = (unsigned)hw;
        const bool pro = p.in_scale != nullptr;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int pos = slot + r * SLOTS;
            if (pos < PP) {
                const int py = pos / PW, px = pos - py * PW;
                const int gy = ty0 + py - HALO, gx = tx0 + px - HALO;
                const bool inb = gy >= 0 && gy < p.h && gx >= 0 && gx < p.wd;
                const unsigned goff = inb ? (unsigned)gy * (unsigned)p.wd + (unsigned)gx : 0u;
#pragma unroll 4
                for (int kc = grp; kc < kKC; kc += G) {
                    const int c = c0 + kc;
                    float v = 0.f;
                    if (inb && c < p.cin) {
                        v = xin[(unsigned)c * uhw + goff];
                        if (pro) v = pro_apply(v, p.in_scale[c], p.in_shift[c], p.in_relu);
                    }
                    lp[kc * PP + pos] = v;
                }
            }
        }
    }
};

// BatchNorm statistics: red[WPX][CT][2] (per pixel-wave partials) -> stat_part, in a fixed order
template <int WPX, int CT>
__device__ __forceinline__ void write_stat_part(const ConvArgs& p, const float* red, int bz, int tile, int co0,
                                                int tid) {
    __syncthreads();
    lf::write_stat_part<WPX, CT>(p.stat_part, p.stat_tiles, p.cout, (long long)bz * (p.tiles_x * p.tiles_y) + tile,
                                 co0, red, tid, kThreads);
}

// Direct GEMM (the stem and the 1x1 convolutions).  TAPS: 9 (3x3) or 1 (1x1).  Tile TW x TH pixels = NPB blocks of 32 (flat index); waves WCO x WPX = 4,
// each wave computes MB cout-blocks x NB pixel-blocks of 32 with v_mfma_f32_32x32x2_f32.
// min waves/SIMD asked of the register allocator: accumulators + VGPRs share one 512-entry
// file per SIMD lane; with the prefetch registers <=32 accumulators fit 3 waves, more fit 2.
template <int TAPS, int TW, int TH, int WCO, int MB, int WPX, int NB, int kKC, bool STK = false>
__global__ __launch_bounds__(kThreads, (MB * NB * 16 <= 32 ? 3 : 2))
void conv_mfma_kernel(ConvArgs p) {
    constexpr int NPB = TW * TH / 32;
    static_assert(TW * TH % 32 == 0, "tile must be whole 32-pixel blocks");
    static_assert(WCO * WPX == 4 && WPX * NB == NPB, "wave decomposition");
    constexpr int CT = 32 * WCO * MB;
    constexpr int HALO = TAPS == 9 ? 1 : 0;
    using Patch = PatchStage<TW, TH, HALO, STK, kKC>;
    constexpr int PW = Patch::PW, PP = Patch::PP;
    constexpr int PATCH = kKC * PP;
    constexpr int WSZ = kKC * TAPS * CT;
    static_assert(PATCH % 4 == 0, "16-byte aligned weight region");
    constexpr int CT4 = CT / 4, NWI = kKC * TAPS * CT4, WPT = (NWI + kThreads - 1) / kThreads;

    __shared__ __attribute__((aligned(16))) float lds[PATCH + WSZ];
    __shared__ float lsc[2 * kMaxProC];
    __shared__ float lep[3 * CT];
    float* lp = lds;
    float* lw = lds + PATCH;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wave_co = wid % WCO, wave_px = wid / WCO;
    const ConvTile<TW, TH, HALO, STK> t(p);
    const int co0 = t.by * CT;
    const size_t hw = (size_t)p.h * p.wd;
    const unsigned uhw = (unsigned)hw;
    const float* xin = p.x + (size_t)t.n * p.cin * hw;

    // per-lane LDS read bases
    const int khalf = lane >> 5, j = lane & 31;
    int bbase[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int f = (wave_px * NB + nb) * 32 + j;
        const int r = f / TW, prow = (STK && r >= t.ra) ? r + 2 * HALO : r;
        bbase[nb] = khalf * PP + prow * PW + (f % TW);
    }
    const int abase = khalf * TAPS * CT + wave_co * MB * 32 + j;

    f32x16 acc[MB][NB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][nb][r] = 0.f;

    // cp loop only partially unrolled: the scheduler otherwise hoists dozens of LDS reads and
    // the accumulators + prefetch registers no longer fit
    auto compute_chunk = [&]() {
#pragma unroll 2
        for (int cp = 0; cp < kKC / 2; ++cp) {
            const float* lwc = lw + abase + 2 * cp * TAPS * CT;
            const float* lpc = lp + 2 * cp * PP;
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const int dy = TAPS == 9 ? tap / 3 : 0, dx = TAPS == 9 ? tap % 3 : 0;
                float a[MB], b[NB];
#pragma unroll
                for (int m = 0; m < MB; ++m) a[m] = lwc[tap * CT + m * 32];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) b[nb] = lpc[bbase[nb] + dy * PW + dx];
#pragma unroll
                for (int m = 0; m < MB; ++m)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        acc[m][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[nb], acc[m][nb], 0, 0, 0);
            }
        }
    };

    const int nchunks = (p.cin + kKC - 1) / kKC;
    const bool vec = p.vec_ok && (t.tx0 + TW <= p.wd);  // uniform per workgroup

    if (vec) {
        // ---------------- vector staging with register prefetch ----------------
        float4 wv[WPT];
        // with > 64 accumulators there are no registers left to hold the weight prefetch: those
        // variants prefetch the patch only and fetch the (L2-resident) weights in the store phase
        constexpr bool kPrefetchW = MB * NB * 16 <= 64;
        Patch patch(p, t, tid);
        // weight rows: byte offsets from the chunk's first row, kBufOob for cout columns beyond the
        // tensor; rows beyond Cin fall outside the chunk's buffer size -> zeros
        unsigned wg[WPT];
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int e = tid + i * kThreads;
            const int row = e / CT4, col = (e - row * CT4) * 4;
            wg[i] = (e < NWI && co0 + col < p.cout) ? 4u * ((unsigned)row * (unsigned)p.cout + (unsigned)(co0 + col)) : kBufOob;
        }
        auto load_weights = [&](int c0) {
            const __amdgpu_buffer_rsrc_t rw =
                buf_rsrc(p.w + (size_t)c0 * TAPS * p.cout,
                         4u * (unsigned)(min(kKC, p.cin - c0) * TAPS) * (unsigned)p.cout);
#pragma unroll
            for (int i = 0; i < WPT; ++i) wv[i] = buf_load4(rw, wg[i]);
        };
        auto store_chunk = [&](int c0) {
            if (!kPrefetchW) load_weights(c0);
            // the constants of more than three items at once would cost <1,56,8,2,1,2,7> its third wave per SIMD
            constexpr bool kAhead = Patch::IPT + Patch::HPT <= 3;
            if (p.in_scale != nullptr)  // workgroup-uniform, around the whole patch store
                patch.template store<true, kAhead>(p, lp, lsc, c0, tid);
            else
                patch.template store<false>(p, lp, lsc, c0, tid);
#pragma unroll
            for (int i = 0; i < WPT; ++i) {
                const int e = tid + i * kThreads;
                if (e < NWI) reinterpret_cast<float4*>(lw)[e] = wv[i];  // lw[row*CT + col]
            }
        };
        patch.load(p, xin, 0);
        if (kPrefetchW) load_weights(0);
        stage_channel_consts<CT>(p, lsc, lep, co0, tid);
        for (int ch = 0; ch < nchunks; ++ch) {
            advance_pro_consts(p, lsc, ch * kKC, tid);
            __syncthreads();  // previous chunk's LDS reads are done
            store_chunk(ch * kKC);
            __syncthreads();
            if (ch + 1 < nchunks) {  // in flight during the MFMAs
                patch.load(p, xin, (ch + 1) * kKC);
                if (kPrefetchW) load_weights((ch + 1) * kKC);
            }
            compute_chunk();
        }
    } else {
        // ---------------- scalar staging (ragged shapes / partial tiles) ----------------
        constexpr int WROWS = kKC * TAPS, RPP = kThreads / CT;
        const int wcol = tid % CT, wrow0 = tid / CT;
        const bool wcol_ok = co0 + wcol < p.cout;
        stage_channel_consts<CT>(p, lsc, lep, co0, tid);
        for (int ch = 0; ch < nchunks; ++ch) {
            const int c0 = ch * kKC;
            __syncthreads();
            Patch::stage_scalar(p, lp, xin, t.tx0, t.ty0, c0, tid);
            const int wvalid = (p.cin - c0) * TAPS;
#pragma unroll 4
            for (int row = wrow0; row < WROWS; row += RPP) {
                float v = 0.f;
                if (wcol_ok && row < wvalid)
                    v = p.w[((unsigned)c0 * TAPS + row) * (unsigned)p.cout + (unsigned)(co0 + wcol)];
                lw[row * CT + wcol] = v;
            }
            __syncthreads();
            compute_chunk();
        }
    }

    float* yout = p.y + (size_t)t.n * p.cout * hw;
    const bool stats = p.stat_part != nullptr, masked = p.stat_mask_y != nullptr;
    float* red = lds;  // [WPX][CT][2] statistics scratch
    static_assert(WPX * CT * 2 <= PATCH + WSZ, "stat scratch must fit the staging LDS");
    if (stats) __syncthreads();  // every wave is done with the staging LDS
    const float* my = masked ? p.stat_mask_y + (size_t)t.n * p.cout * hw : nullptr;
    // epilogue: D[row = co][col = pixel]; row = (r&3) + 8*(r>>2) + 4*(lane>>5).
    // Processed in groups of RG accumulator rows: the group's read-modify-write operands
    // (accumulate) and BatchNorm-backward mask values are loaded unconditionally from clamped
    // addresses first, so RG*NB loads are in flight together, then stored / reduced.
    constexpr int RG = TAPS == 1 ? (NB <= 2 ? 4 : 1) : (NB <= 2 ? 16 : 4);
    bool pix_ok[NB];
    unsigned pixc[NB];  // pixel offset, 0 when outside the image
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int f = (wave_px * NB + nb) * 32 + j;
        const int r = f / TW, ox = t.tx0 + f % TW;
        const bool in_a = r < t.ra;
        const int oy = in_a ? t.gyA0 + r : r - t.ra;
        pix_ok[nb] = (in_a ? t.imgA_ok : t.imgB_ok) && oy < p.h && ox < p.wd;
        pixc[nb] = pix_ok[nb] ? (unsigned)((in_a ? t.imgA : t.imgA + 1) * p.cout) * uhw +
                                    (unsigned)oy * (unsigned)p.wd + (unsigned)ox
                              : 0u;
    }
#pragma unroll
    for (int m = 0; m < MB; ++m) {
#pragma unroll
        for (int rg = 0; rg < 16; rg += RG) {
            // keeps the later groups' LDS reads of the statistics constants from being hoisted to the top of the
            // epilogue, where they cost the 112- and 128-accumulator variants their third wave per SIMD
            asm volatile("" ::: "memory");
            float oldv[RG][NB], yv[RG][NB];
            if (p.accumulate) {
#pragma unroll
                for (int rr = 0; rr < RG; ++rr) {
                    const int r = rg + rr;
                    const int co = co0 + (wave_co * MB + m) * 32 + 4 * khalf + (r & 3) + 8 * (r >> 2);
                    const float* src = yout + (size_t)min(co, p.cout - 1) * hw;
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) oldv[rr][nb] = src[pixc[nb]];
                }
            }
            if (masked) {
#pragma unroll
                for (int rr = 0; rr < RG; ++rr) {
                    const int r = rg + rr;
                    const int co = co0 + (wave_co * MB + m) * 32 + 4 * khalf + (r & 3) + 8 * (r >> 2);
                    const float* src = my + (size_t)min(co, p.cout - 1) * hw;
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) yv[rr][nb] = src[pixc[nb]];
                }
            }
#pragma unroll
            for (int rr = 0; rr < RG; ++rr) {
                const int r = rg + rr;
                const int cl = (wave_co * MB + m) * 32 + 4 * khalf + (r & 3) + 8 * (r >> 2);
                const int co = co0 + cl;
                const bool co_ok = co < p.cout;
                float* dst = yout + (size_t)co * hw;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    if (p.accumulate) acc[m][nb][r] += oldv[rr][nb];  // the statistics see the sum
                    if (co_ok && pix_ok[nb])
                        dst[pixc[nb]] = acc[m][nb][r];
                }
                if (!stats) continue;
                float s1 = 0.f, s2 = 0.f;
                if (!masked) {  // forward statistics about the pivot
                    const float pv = lep[cl];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        lf::stat_accumulate(acc[m][nb][r], pix_ok[nb], false, pv, 0.f, 0.f, 0.f, 0, s1, s2);
                } else {  // backward sums of the BatchNorm this gradient feeds
                    const float msc = lep[CT + cl], msh = lep[2 * CT + cl];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        lf::stat_accumulate(acc[m][nb][r], co_ok && pix_ok[nb], true, 0.f, yv[rr][nb], msc, msh,
                                            p.mask_relu, s1, s2);
                }
                s1 = half_sum32(s1);
                s2 = half_sum32(s2);
                if (j == 31) {
                    red[(wave_px * CT + cl) * 2] = s1;
                    red[(wave_px * CT + cl) * 2 + 1] = s2;
                }
            }
        }
    }
    if (stats) write_stat_part<WPX, CT>(p, red, t.bz, t.tile, co0, tid);
}

// Winograd F(2x2,3x3) (every 3x3 convolution but the stem).  The tile TW x TH is NT = (TW/2)*(TH/2) Winograd tiles (flat index, 2x2 output pixels each) and the
// workgroup's CT = 16*MB output channels; 4 waves, K-chunks of 8 input channels.  Per 4-channel K-step,
// each of the 16 transform positions is a GEMM U[pos] (cout x cin) . V[pos] (cin x tiles) on
// v_mfma_f32_16x16x4_f32; a wave owns MB cout-blocks x NB tile-blocks of 16, all 16 positions, so M[pos]
// for one (cout, tile) sits in one lane and register and the inverse transform is register-local.
// U = G g G^T comes prepared from wino_filters_kernel (once per layer, role and step) and a chunk's slice
// of it is copied to LDS (pitch 20 floats per filter: conflict-free ds_read_b128 of a lane's 16 positions);
// V = B^T d B is formed per lane from the LDS patch.  The patch staging (prologue, zeros, two-image
// strip) is the direct kernel's.  64 accumulators per (cout-block, tile-block): 2 waves per SIMD.
template <int TW, int TH, int MB, int NB, bool STK>
__global__ __launch_bounds__(kThreads, 2)
void conv_wino_kernel(ConvArgs p) {
    constexpr int kKC = 8, WPX = 4;  // K-chunk; every wave takes all of the workgroup's couts
    constexpr int TXN = TW / 2, NT = TXN * (TH / 2);  // Winograd tiles per row / per workgroup
    static_assert(TH % 2 == 0, "F(2x2,3x3): even tile");
    static_assert(WPX * NB * 16 >= NT, "wave decomposition");
    constexpr int CT = 16 * MB;
    constexpr int kUP = 20;  // LDS pitch of one (channel, cout) U: 16 positions + 4 (conflict-free b128 reads)
    using Patch = PatchStage<TW, TH, 1, STK, kKC>;
    constexpr int PW = Patch::PW, PP = Patch::PP;
    constexpr int PATCH = kKC * PP;
    constexpr int WSZ = kKC * CT * kUP;
    static_assert(PATCH % 4 == 0, "16-byte aligned U region");

    __shared__ __attribute__((aligned(16))) float lds[PATCH + WSZ];
    __shared__ float lsc[2 * kMaxProC];
    __shared__ float lep[3 * CT];
    float* lp = lds;
    float* lw = lds + PATCH;

    const int tid = threadIdx.x, lane = tid & 63, wave_px = tid >> 6;
    const ConvTile<TW, TH, 1, STK> t(p);
    const int co0 = t.by * CT;
    const size_t hw = (size_t)p.h * p.wd;
    const unsigned uhw = (unsigned)hw;
    const float* xin = p.x + (size_t)t.n * p.cin * hw;

    // lane l reads the 4x4 patch window of tile (l & 15) of each of its tile-blocks for channel
    // (l >> 4) of the K-step (tiles past NT read the last tile's window; they are never stored), and
    // U[cout = l & 15][channel = l >> 4] of each of its cout-blocks
    const int wq = lane >> 4, wl = lane & 15;
    int vbase[NB];
    const int ubase = (wq * CT + wl) * kUP;
    f32x4 wacc[MB][NB][16];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int tt = min((wave_px * NB + nb) * 16 + wl, NT - 1);
        const int r0 = 2 * (tt / TXN), prow = (STK && r0 >= t.ra) ? r0 + 2 : r0;
        vbase[nb] = wq * PP + prow * PW + 2 * (tt % TXN);
    }
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int q = 0; q < 16; ++q) wacc[m][nb][q] = f32x4{0.f, 0.f, 0.f, 0.f};

    // late(0), late(1) (unless late is nullptr): called before the last quarter and the last eighth of the chunk's
    // MFMAs; the scheduler moves nothing across them
    auto compute_chunk = [&](auto late) {
#pragma unroll
        for (int s = 0; s < kKC / 4; ++s) {
            // the cout-blocks' U first, then one tile-block's V at a time
            float u[MB][16];
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                const float4* us = reinterpret_cast<const float4*>(lw + ubase + (4 * s * CT + m * 16) * kUP);
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const float4 v4 = us[q4];
                    u[m][4 * q4 + 0] = v4.x;
                    u[m][4 * q4 + 1] = v4.y;
                    u[m][4 * q4 + 2] = v4.z;
                    u[m][4 * q4 + 3] = v4.w;
                }
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float* src = lp + vbase[nb] + 4 * s * PP;
                float d[16], v[16];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float2 lo = *reinterpret_cast<const float2*>(src + r * PW);
                    const float2 hi = *reinterpret_cast<const float2*>(src + r * PW + 2);
                    d[r * 4 + 0] = lo.x;
                    d[r * 4 + 1] = lo.y;
                    d[r * 4 + 2] = hi.x;
                    d[r * 4 + 3] = hi.y;
                }
                wino_input(d, v);
#pragma unroll
                for (int m = 0; m < MB; ++m)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        if constexpr (!std::is_same_v<decltype(late), std::nullptr_t>) {
                            const int at = (nb * MB + m) * 16 + q;
                            if (s == kKC / 4 - 1 && (at == NB * MB * 8 || at == NB * MB * 12)) {
                                __builtin_amdgcn_sched_barrier(0);
                                late(at == NB * MB * 8 ? 0 : 1);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                        wacc[m][nb][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[m][q], v[q], wacc[m][nb][q], 0, 0, 0);
                    }
            }
        }
    };

    // filters: the chunk's slice of the prepared U (wino_filters_kernel: [Cin][Cout][16]) is kKC runs
    // of CT * 64 contiguous bytes, copied to LDS as they are.  Thread tid takes quarter tid & 3 of the
    // filter (channel tid / (4 CT) + i * KSTEP, cout (tid / 4) % CT), i < UPT: a wave's 16-byte loads
    // cover whole 1 KB runs, and item i lies a fixed stride after item 0 in global memory and in LDS.
    // Couts beyond Cout start at 2^31, channels beyond Cin fall outside the chunk's buffer size -> zeros.
    constexpr int KSTEP = kThreads / (4 * CT), UPT = kKC / KSTEP;
    static_assert(kThreads % (4 * CT) == 0 && kKC % KSTEP == 0, "whole channels per pass");
    const int ukc = tid / (4 * CT), uco = (tid >> 2) % CT, uq4 = tid & 3;
    const unsigned ustep = 64u * KSTEP * (unsigned)p.cout;
    const unsigned ugo = co0 + uco < p.cout ? 4u * (((unsigned)ukc * (unsigned)p.cout + (unsigned)(co0 + uco)) * 16u + 4u * (unsigned)uq4) : 0x80000000u;
    float* const ulds = lw + (ukc * CT + uco) * kUP + 4 * uq4;
    float4 uv[UPT];
    static_assert(UPT % 2 == 0, "U is asked for in two halves");
    auto load_u_half = [&](int c0, int half) {
        // (the size as in PatchStage::load; written as a select, which stays in scalar registers where
        // max(min(), 0) becomes a vector instruction and the loads a loop over lanes)
        const int nc = min(kKC, p.cin - c0);
        const __amdgpu_buffer_rsrc_t ru =
            buf_rsrc(p.wino_u + (size_t)c0 * p.cout * 16, nc > 0 ? 64u * (unsigned)nc * (unsigned)p.cout : 0u);
#pragma unroll
        for (int i = 0; i < UPT / 2; ++i) {
            const int e = half * (UPT / 2) + i;
            uv[e] = buf_load4(ru, ugo + (unsigned)e * ustep);
        }
    };
    auto load_u = [&](int c0) {
        load_u_half(c0, 0);
        load_u_half(c0, 1);
    };
    auto store_u = [&]() {
#pragma unroll
        for (int i = 0; i < UPT; ++i) *reinterpret_cast<float4*>(ulds + i * KSTEP * CT * kUP) = uv[i];
    };

    const int nchunks = (p.cin + kKC - 1) / kKC;
    const bool vec = p.vec_ok && (t.tx0 + TW <= p.wd);  // uniform per workgroup

    if (vec) {
        // ---------------- vector staging with register prefetch ----------------
        // The patch is prefetched into registers during the previous chunk's MFMAs.  The next chunk's U is asked
        // for inside the last quarter of those MFMAs, one half at its start and one in its middle, where the
        // operand registers of the MFMAs already issued are free (held across all of a chunk's MFMAs its 4 * UPT
        // registers measured 0.8 ms per step slower); so the store phase waits for no load issued after the
        // chunk's first barrier.  With two tile-blocks per wave (21 patch registers) there is no room for that
        // without scratch: that instantiation fetches U in the store phase, in flight while the patch goes to LDS.
        // Chunk 0's U and the per-channel constants are asked for right behind chunk 0's patch, so the
        // workgroup's first wait covers all three.
        constexpr bool kUAhead = NB == 1;
        Patch patch(p, t, tid);
        patch.load(p, xin, 0);
        if (kUAhead) load_u(0);
        stage_channel_consts<CT>(p, lsc, lep, co0, tid);
        // The loop exists once with and once without a prologue (workgroup-uniform), and the last chunk, which
        // asks for nothing more, stands behind it: no body has a branch around a load, so every wait of a store
        // phase counts exactly the loads issued after the one it needs.
        auto k_loop = [&](auto pro_c) {
            constexpr bool PRO = decltype(pro_c)::value;
            auto chunk = [&](int ch, auto last_c) {
                constexpr bool LAST = decltype(last_c)::value;
                // kept in a scalar register, so that the buffer descriptors built from it are
                const int c0 = __builtin_amdgcn_readfirstlane(ch * kKC);
                if (PRO) advance_pro_consts(p, lsc, c0, tid);
                __syncthreads();  // previous chunk's LDS reads are done
                if (!kUAhead) load_u(c0);
                patch.template store<PRO>(p, lp, lsc, c0, tid);
                store_u();
                __syncthreads();
                if (!LAST) patch.load(p, xin, c0 + kKC);  // in flight during the MFMAs
                if constexpr (kUAhead && !LAST)
                    compute_chunk([&](int half) { load_u_half(c0 + kKC, half); });
                else
                    compute_chunk(nullptr);
            };
            for (int ch = 0; ch + 1 < nchunks; ++ch) chunk(ch, std::false_type{});
            chunk(nchunks - 1, std::true_type{});
        };
        if (p.in_scale != nullptr)
            k_loop(std::true_type{});
        else
            k_loop(std::false_type{});
    } else {
        // ---------------- scalar staging (ragged shapes / partial tiles) ----------------
        stage_channel_consts<CT>(p, lsc, lep, co0, tid);
        for (int ch = 0; ch < nchunks; ++ch) {
            const int c0 = ch * kKC;
            __syncthreads();
            Patch::stage_scalar(p, lp, xin, t.tx0, t.ty0, c0, tid);
            load_u(c0);
            store_u();
            __syncthreads();
            compute_chunk(nullptr);
        }
    }

    float* yout = p.y + (size_t)t.n * p.cout * hw;
    const bool stats = p.stat_part != nullptr, masked = p.stat_mask_y != nullptr;
    float* red = lds;  // [WPX][CT][2] statistics scratch
    static_assert(WPX * CT * 2 <= PATCH + WSZ, "stat scratch must fit the staging LDS");
    if (stats) __syncthreads();  // every wave is done with the staging LDS
    const float* my = masked ? p.stat_mask_y + (size_t)t.n * p.cout * hw : nullptr;
    // epilogue: register i of wacc[m][nb][pos] is M[pos] of cout (l >> 4) * 4 + i of cout-block m
    // and tile l & 15 of tile-block nb; the inverse transform gives its 2x2 pixels (both rows in one
    // image: the strip seam row ra is even).  Pixel pairs are loaded and stored as float2 where y (and
    // the mask tensor) allow it: W even makes every offset here even and both pixels of a pair in-image
    // together.
    // The 4 * MB (cout-block, register) steps go in groups of G.  A group first issues every read it
    // needs (the old outputs when accumulating, the mask tensor for the BatchNorm-backward sums),
    // unconditionally and from clamped offsets, so one memory latency is exposed per group instead of
    // one per step; only then does it transform, add and store, step by step in the old order.  A wave
    // whose tiles and couts all lie inside the tensor (FULL) stores without a branch.
    // Statistics: per lane over its tiles' pixels, then over the 16 lanes of a row (DPP), then over
    // the WPX waves in LDS.
    const bool y2 = (p.wd & 1) == 0 && (reinterpret_cast<size_t>(p.y) & 7) == 0 &&
                    (reinterpret_cast<size_t>(p.stat_mask_y) & 7) == 0;
    bool pok[NB][4];
    unsigned pofs[NB][4];  // pixel offsets, 0 when outside the image
    bool lane_full = true;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int tt = (wave_px * NB + nb) * 16 + wl;
        const int r0 = 2 * (tt / TXN), ox = t.tx0 + 2 * (tt % TXN);
        const bool in_a = r0 < t.ra;
        const int oy = in_a ? t.gyA0 + r0 : r0 - t.ra;
        const bool img_ok = tt < NT && (in_a ? t.imgA_ok : t.imgB_ok);
        const unsigned base = (unsigned)((in_a ? t.imgA : t.imgA + 1) * p.cout) * uhw;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int py = oy + (q >> 1), px = ox + (q & 1);
            pok[nb][q] = img_ok && py < p.h && px < p.wd;
            pofs[nb][q] = pok[nb][q] ? base + (unsigned)py * (unsigned)p.wd + (unsigned)px : 0u;
            lane_full = lane_full && (pok[nb][q] || tt >= NT);
        }
    }
    constexpr int STEPS = 4 * MB, G = (STEPS * NB <= 8 ? STEPS : 8 / NB);  // 32 pixels per lane and tensor in flight
    static_assert(STEPS % G == 0, "whole groups");
    auto epilogue = [&](auto full_c) {
        // FULL: every tile slot below NT has all four pixels in the image, y2 holds and no cout is absent
        constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
        for (int g0 = 0; g0 < STEPS; g0 += G) {
            float oldv[G][NB][4], yv[G][NB][4];
            // one tensor after the other, each behind a single uniform branch: with a branch per step between
            // the loads the compiler falls back to full waits
            auto batch = [&](const float* src, float (&dst)[G][NB][4]) {
#pragma unroll
                for (int gs = 0; gs < G; ++gs) {
                    const int m = (g0 + gs) / 4, i = (g0 + gs) % 4;
                    const float* sp = src + (size_t)min(co0 + m * 16 + 4 * wq + i, p.cout - 1) * hw;
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        if (FULL || y2) {
#pragma unroll
                            for (int r = 0; r < 2; ++r) {
                                const float2 v2 = *reinterpret_cast<const float2*>(sp + pofs[nb][2 * r]);
                                dst[gs][nb][2 * r] = v2.x;
                                dst[gs][nb][2 * r + 1] = v2.y;
                            }
                        } else {
#pragma unroll
                            for (int q = 0; q < 4; ++q) dst[gs][nb][q] = sp[pofs[nb][q]];
                        }
                    }
                }
            };
            if (p.accumulate) batch(yout, oldv);
            if (masked) batch(my, yv);
#pragma unroll
            for (int gs = 0; gs < G; ++gs) {
                const int m = (g0 + gs) / 4, i = (g0 + gs) % 4;
                const int cl = m * 16 + 4 * wq + i;
                const int co = co0 + cl;
                const bool co_ok = FULL || co < p.cout;
                const size_t cofs = (size_t)min(co, p.cout - 1) * hw;
                float out[NB][4];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    float mm[16];
#pragma unroll
                    for (int q = 0; q < 16; ++q) mm[q] = wacc[m][nb][q][i];
                    wino_output(mm, out[nb]);
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    if (p.accumulate) {  // the statistics see the sum
#pragma unroll
                        for (int q = 0; q < 4; ++q) out[nb][q] += oldv[gs][nb][q];
                    }
                    if (FULL) {
                        // slots beyond NT (only where the tiles do not fill the waves) are the one thing left to mask
                        if (NT == WPX * NB * 16 || pok[nb][0]) {
#pragma unroll
                            for (int r = 0; r < 2; ++r)
                                *reinterpret_cast<float2*>(yout + cofs + pofs[nb][2 * r]) =
                                    make_float2(out[nb][2 * r], out[nb][2 * r + 1]);
                        }
                    } else if (co_ok) {
#pragma unroll
                        for (int r = 0; r < 2; ++r) {
                            float* dst = yout + cofs + pofs[nb][2 * r];
                            if (y2 && pok[nb][2 * r] && pok[nb][2 * r + 1]) {
                                *reinterpret_cast<float2*>(dst) = make_float2(out[nb][2 * r], out[nb][2 * r + 1]);
                            } else {
                                if (pok[nb][2 * r]) dst[0] = out[nb][2 * r];
                                if (pok[nb][2 * r + 1]) yout[cofs + pofs[nb][2 * r + 1]] = out[nb][2 * r + 1];
                            }
                        }
                    }
                }
                if (!stats) continue;
                float s1 = 0.f, s2 = 0.f;
                if (!masked) {  // forward statistics about the pivot
                    const float pv = lep[cl];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            lf::stat_accumulate(out[nb][q], pok[nb][q], false, pv, 0.f, 0.f, 0.f, 0, s1, s2);
                } else {  // backward sums of the BatchNorm this gradient feeds
                    const float msc = lep[CT + cl], msh = lep[2 * CT + cl];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            lf::stat_accumulate(out[nb][q], co_ok && pok[nb][q], true, 0.f, yv[gs][nb][q], msc, msh,
                                                p.mask_relu, s1, s2);
                }
                s1 = row_sum16(s1);
                s2 = row_sum16(s2);
                if (wl == 0) {
                    red[(wave_px * CT + cl) * 2] = s1;
                    red[(wave_px * CT + cl) * 2 + 1] = s2;
                }
            }
        }
    };
    // wave-uniform: voted over the lanes' own store predicates, so the branch-free path cannot store where the
    // general one would not
    if (__all(y2 && lane_full && co0 + CT <= p.cout))
        epilogue(std::true_type{});
    else
        epilogue(std::false_type{});
    if (stats) write_stat_part<WPX, CT>(p, red, t.bz, t.tile, co0, tid);
}

// ---------------------------------------------------------------------------
// wgrad
// ---------------------------------------------------------------------------
// 1x1 (wgrad_mfma_kernel): D[ci][co] += sum over pixel pairs.  A operand = X (lane -> ci, k = pixel),
// B operand = dY (lane -> co).  A workgroup owns a (32*WCI ci) x (32*WCO co) weight block and
// a range of (image, tile) work items; its 4 waves are WCI x WCO x KSPL with the KSPL waves
// splitting the rows of each tile.
struct WgradArgs {
    const float* x;   // [N][Cin][H][W]
    const float* dy;  // [N][Cout][H][W]
    float* part;      // [splits][Cin][TAPS][Cout] partial slabs
    const float* in_scale;
    const float* in_shift;
    int n, cin, cout, h, wd;
    int tiles_x, tiles_y, items, items_per_split;
    int in_relu;
    int vec_ok;
    // optional: dY is the BatchNorm backward of `dy` (= upstream g), formed while staging
    //   dz = (g*alpha[n][co] + add[n][co]) * [bn_y*coef0[co] + coef1[co] > 0 or !bn_relu]
    //   dY = coef2[co]*dz + coef3[co]*bn_y + coef4[co]
    // and written to dy_out by the ci-block-0 workgroups (each element exactly once)
    const float* bn_y;     // null = plain dY
    const float* bn_alpha;
    const float* bn_add;
    const float* bn_coef;  // [5][Cout]
    float* dy_out;
    int bn_relu;
};

__device__ __forceinline__ float bn_dy1(float g, float y, float al, float ad, float c0, float c1,
                                        float c2, float c3, float c4, int relu) {
    float dz = fmaf(g, al, ad);
    if (relu && !(fmaf(y, c0, c1) > 0.f)) dz = 0.f;
    return fmaf(c2, dz, fmaf(c3, y, c4));
}

// Three waves per SIMD for the instantiations that spilled to scratch at four (128 registers): plan_wgrad sizes
// the grid for three resident workgroups per CU anyway.  <16,8,1,2,2> needs more than either and runs at two.
template <int TW, int TH, int WCI, int WCO, int KSPL>
__global__ __launch_bounds__(kThreads, KSPL == 2 ? 4 : 3) void wgrad_mfma_kernel(WgradArgs p) {
    static_assert(WCI * WCO * KSPL == 4, "wave decomposition");
    static_assert(TH % KSPL == 0 && TW % 4 == 0, "rows split across waves, float4 rows");
    constexpr int PP = (TW * TH) | 1;  // odd plane pitch (X and dY): 32 lanes on 32 channels hit 32 banks
    constexpr int CI_T = 32 * WCI, CO_T = 32 * WCO;
    constexpr int XSZ = CI_T * PP, DSZ = CO_T * PP;
    constexpr int RED = KSPL > 1 ? 1024 : 0;  // one wave's accumulators
    constexpr int LDSF = XSZ + DSZ > RED ? XSZ + DSZ : RED;
    constexpr int TW4 = TW / 4;
    constexpr int NXI = CI_T * TH * TW4, XPT = (NXI + kThreads - 1) / kThreads;
    constexpr int NDI = CO_T * TH * TW4, DPT = (NDI + kThreads - 1) / kThreads;
    __shared__ float lds[LDSF];
    float* lx = lds;
    float* ld = lds + XSZ;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int w_ci = wid % WCI, w_co = (wid / WCI) % WCO, w_k = wid / (WCI * WCO);
    // split and channel blocks from the dispatch index: the blocks of a split share an XCD (lf::xcd_split_block3)
    const lf::Block3 blk = lf::xcd_split_block3();
    const int ci0 = blk.y * CI_T, co0 = blk.z * CO_T;
    const int khalf = lane >> 5, j = lane & 31;
    const size_t hw = (size_t)p.h * p.wd;
    const unsigned uhw = (unsigned)hw;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    const int abase = (w_ci * 32 + j) * PP + khalf;  // + row*TW + x
    const int bbase = (w_co * 32 + j) * PP + khalf;
    const bool pro = p.in_scale != nullptr;

    auto compute_item = [&]() {
        constexpr int ROWS = TH / KSPL;
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            const int row = w_k * ROWS + rr;
#pragma unroll 2
            for (int xx = 0; xx < TW; xx += 2) {
                const float b = ld[bbase + row * TW + xx];
                const float a = lx[abase + row * TW + xx];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
        }
    };

    const int first = blk.x * p.items_per_split;
    const int last = min(first + p.items_per_split, p.items);
    const int tiles = p.tiles_x * p.tiles_y;

    if (p.vec_ok) {  // every tile is full in x (host guarantees W % TW == 0 for this path)
        float4 xv[XPT], dv[DPT];
        unsigned xok = 0;
        // producer BatchNorm scale/shift of this workgroup's CI_T channels, staged once in LDS
        __shared__ float lsc[kMaxProC / 2];
        if (pro) {
            for (int c = tid; c < CI_T; c += kThreads) {
                const int gc = ci0 + c;
                lsc[c] = gc < p.cin ? p.in_scale[gc] : 1.f;
                lsc[kMaxProC / 4 + c] = gc < p.cin ? p.in_shift[gc] : 0.f;
            }
        }
        // optional: dY = BatchNorm backward of p.dy, formed while staging (see WgradArgs)
        const bool bn = p.bn_y != nullptr;
        float4 yv[DPT];
        float dal[DPT], dad[DPT];
        unsigned dok = 0;
        __shared__ float lbn[5 * CO_T];
        if (bn) {
            for (int e = tid; e < 5 * CO_T; e += kThreads) {
                const int kk = e / CO_T, gc = co0 + (e - kk * CO_T);
                lbn[e] = gc < p.cout ? p.bn_coef[(size_t)kk * p.cout + gc] : 0.f;
            }
        }
        // the next item's loads stay in registers over the MFMAs
        auto load_x = [&](int item) {
            const int n = item / tiles, t = item - n * tiles;
            const int tx0 = (t % p.tiles_x) * TW, ty0 = (t / p.tiles_x) * TH;
            const float* xin = p.x + (size_t)n * p.cin * hw;
            xok = 0;
#pragma unroll
            for (int i = 0; i < XPT; ++i) {
                const int e = tid + i * kThreads;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                const int c = e / (TH * TW4), rem = e - c * (TH * TW4);
                const int py = rem / TW4, slot = rem - py * TW4;
                const int gc = ci0 + c, gy = ty0 + py;
                if (e < NXI && gc < p.cin && gy < p.h) {
                    v = *reinterpret_cast<const float4*>(xin + (unsigned)gc * uhw +
                                                         (unsigned)gy * (unsigned)p.wd + tx0 + 4 * slot);
                    xok |= 1u << i;
                }
                xv[i] = v;
            }
        };
        auto load_d = [&](int item) {
            const int n = item / tiles, t = item - n * tiles;
            const int tx0 = (t % p.tiles_x) * TW, ty0 = (t / p.tiles_x) * TH;
            const float* din = p.dy + (size_t)n * p.cout * hw;
            dok = 0;
#pragma unroll
            for (int i = 0; i < DPT; ++i) {
                const int e = tid + i * kThreads;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                const int c = e / (TH * TW4), rem = e - c * (TH * TW4);
                const int py = rem / TW4, slot = rem - py * TW4;
                const int gc = co0 + c, gy = ty0 + py;
                if (e < NDI && gc < p.cout && gy < p.h) {
                    v = *reinterpret_cast<const float4*>(din + (unsigned)gc * uhw +
                                                         (unsigned)gy * (unsigned)p.wd + tx0 + 4 * slot);
                    dok |= 1u << i;
                }
                dv[i] = v;
            }
            if (bn) {
                const float* yin = p.bn_y + (size_t)n * p.cout * hw;
#pragma unroll
                for (int i = 0; i < DPT; ++i) {
                    const int e = tid + i * kThreads;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    const int c = e / (TH * TW4), rem = e - c * (TH * TW4);
                    const int py = rem / TW4, slot = rem - py * TW4;
                    if (dok >> i & 1u)
                        v = *reinterpret_cast<const float4*>(yin + (unsigned)(co0 + c) * uhw +
                                                             (unsigned)(ty0 + py) * (unsigned)p.wd + tx0 + 4 * slot);
                    yv[i] = v;
                }
#pragma unroll
                for (int i = 0; i < DPT; ++i) {
                    const int gc = min(co0 + (tid + i * kThreads) / (TH * TW4), p.cout - 1);
                    dal[i] = p.bn_alpha != nullptr ? p.bn_alpha[(size_t)n * p.cout + gc] : 1.f;
                    dad[i] = p.bn_add != nullptr ? p.bn_add[(size_t)n * p.cout + gc] : 0.f;
                }
            }
        };
        auto store_x = [&]() {
#pragma unroll
            for (int i = 0; i < XPT; ++i) {
                const int e = tid + i * kThreads;
                if (e < NXI) {
                    const int c = e / (TH * TW4), rem = e - c * (TH * TW4);
                    const int py = rem / TW4, slot = rem - py * TW4;
                    float4 v = xv[i];
                    if (pro && (xok >> i & 1u)) {
                        const float sc = lsc[c], sh = lsc[kMaxProC / 4 + c];
                        v.x = pro_apply(v.x, sc, sh, p.in_relu);
                        v.y = pro_apply(v.y, sc, sh, p.in_relu);
                        v.z = pro_apply(v.z, sc, sh, p.in_relu);
                        v.w = pro_apply(v.w, sc, sh, p.in_relu);
                    }
                    float* dst = lx + c * PP + py * TW + 4 * slot;
                    dst[0] = v.x;
                    dst[1] = v.y;
                    dst[2] = v.z;
                    dst[3] = v.w;
                }
            }
        };
        auto store_d = [&](int item) {
            const int sn = item / tiles, st = item - sn * tiles;
            const int stx0 = (st % p.tiles_x) * TW, sty0 = (st / p.tiles_x) * TH;
#pragma unroll
            for (int i = 0; i < DPT; ++i) {
                const int e = tid + i * kThreads;
                if (e < NDI) {
                    const int c = e / (TH * TW4), rem = e - c * (TH * TW4);
                    float4 v = dv[i];
                    if (bn && (dok >> i & 1u)) {
                        const float c0 = lbn[c], c1 = lbn[CO_T + c], c2 = lbn[2 * CO_T + c],
                                    c3 = lbn[3 * CO_T + c], c4 = lbn[4 * CO_T + c];
                        v.x = bn_dy1(v.x, yv[i].x, dal[i], dad[i], c0, c1, c2, c3, c4, p.bn_relu);
                        v.y = bn_dy1(v.y, yv[i].y, dal[i], dad[i], c0, c1, c2, c3, c4, p.bn_relu);
                        v.z = bn_dy1(v.z, yv[i].z, dal[i], dad[i], c0, c1, c2, c3, c4, p.bn_relu);
                        v.w = bn_dy1(v.w, yv[i].w, dal[i], dad[i], c0, c1, c2, c3, c4, p.bn_relu);
                        if (blk.y == 0 && p.dy_out != nullptr) {
                            const int py = rem / TW4, slot = rem - py * TW4;
                            *reinterpret_cast<float4*>(p.dy_out + ((size_t)sn * p.cout + co0 + c) * hw +
                                                       (size_t)(sty0 + py) * p.wd + stx0 + 4 * slot) = v;
                        }
                    }
                    float* dst = ld + c * PP + rem * 4;
                    dst[0] = v.x;
                    dst[1] = v.y;
                    dst[2] = v.z;
                    dst[3] = v.w;
                }
            }
        };
        if (first < last) {
            load_x(first);
            load_d(first);
        }
        for (int item = first; item < last; ++item) {
            __syncthreads();
            store_x();
            store_d(item);
            __syncthreads();
            if (item + 1 < last) {
                load_x(item + 1);
                load_d(item + 1);
            }
            compute_item();
        }
    } else {
        // scalar staging: thread -> one tile position, walking channels
        constexpr int POS = TW * TH;
        constexpr int SLOTS = POS <= 64 ? 64 : (POS <= 128 ? 128 : 256);
        constexpr int G = kThreads / SLOTS;
        static_assert(POS <= 256, "wgrad tiles are at most 256 positions");
        const int slot = tid % SLOTS, grp = tid / SLOTS;
        const int spy = slot / TW, spx = slot - spy * TW;
        for (int item = first; item < last; ++item) {
            const int n = item / tiles, t = item - n * tiles;
            const int tx0 = (t % p.tiles_x) * TW, ty0 = (t / p.tiles_x) * TH;
            const float* xin = p.x + (size_t)n * p.cin * hw;
            const float* din = p.dy + (size_t)n * p.cout * hw;
            __syncthreads();
            if (slot < POS) {
                const int gy = ty0 + spy, gx = tx0 + spx;
                const bool ok = gy < p.h && gx < p.wd;
                const unsigned off = ok ? (unsigned)gy * (unsigned)p.wd + (unsigned)gx : 0u;
#pragma unroll 4
                for (int c = grp; c < CI_T; c += G) {
                    const int gc = ci0 + c;
                    float v = 0.f;
                    if (ok && gc < p.cin) {
                        v = xin[(unsigned)gc * uhw + off];
                        if (pro) v = pro_apply(v, p.in_scale[gc], p.in_shift[gc], p.in_relu);
                    }
                    lx[c * PP + slot] = v;
                }
#pragma unroll 4
                for (int c = grp; c < CO_T; c += G) {
                    const int gc = co0 + c;
                    float v = 0.f;
                    if (ok && gc < p.cout) v = din[(unsigned)gc * uhw + off];
                    ld[c * PP + slot] = v;
                }
            }
            __syncthreads();
            compute_item();
        }
    }

    // K-split waves fold their accumulators into wave k = 0 through LDS, one (ci,co) block
    // at a time, in a fixed order
    if (KSPL > 1) {
        const int q = w_co * WCI + w_ci;
#pragma unroll 1
        for (int k = 1; k < KSPL; ++k) {
#pragma unroll 1
            for (int qq = 0; qq < WCI * WCO; ++qq) {
                __syncthreads();
                if (w_k == k && q == qq) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) lds[r * 64 + lane] = acc[r];
                }
                __syncthreads();
                if (w_k == 0 && q == qq) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] += lds[r * 64 + lane];
                }
            }
        }
    }
    if (w_k == 0) {
        float* out = p.part + (size_t)blk.x * p.cin * p.cout;
        const int co = co0 + w_co * 32 + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = ci0 + w_ci * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
            if (ci < p.cin && co < p.cout) out[(size_t)ci * p.cout + co] = acc[r];
        }
    }
}

// ---------------------------------------------------------------------------
// projection shortcut backward: BatchNorm backward + 1x1 weight gradient + 1x1 input gradient
// ---------------------------------------------------------------------------
// One pass over x, g and bn_y: dyp = BN'(g) (bn_dy1 with alpha 1, add 0: the bits wgrad_mfma_kernel writes to
// dy_out) lives only in LDS and feeds both products,
//   dW[ci][co] = sum_px x[ci][px] dyp[co][px]      (A = x, lane -> ci; B = dyp, lane -> co; K = pixels)
//   dx[ci][px] = sum_co w[ci][co] dyp[co][px]      (A = w, lane -> ci; B = dyp, lane -> pixel; K = co)
// A 1x1 has no halo: a plane is hw flat pixels and an item is kProjP consecutive pixels of one image.  A workgroup
// owns every channel of its items (Cin = 32 CIB, Cout = 64 CIB, one wave per 32 output channels), so each tensor is
// read once.  Wave w accumulates dW[all ci][co block w] over the workgroup's items and computes, per item, the dx
// block (ci block w % CIB, pixel half w / CIB); its rows of w stay in registers for the whole launch (lane half h
// holds co = h Cout/2 + s at k-step s, one contiguous run per lane), so the filter bank takes no LDS.  The next
// item's loads are issued into registers ahead of the MFMAs; the dx block is stored (128-byte runs per channel)
// before the weight-gradient MFMAs, which cover the stores' latency.  Grid = splits, one slab [Cin][Cout] each,
// summed by lf::reduce_slabs in a fixed order: no atomics.
struct ProjBwdArgs {
    const float* x;     // [N][Cin][HW]
    const float* g;     // [N][Cout][HW]
    const float* bn_y;  // [N][Cout][HW]
    const float* coef;  // [5][Cout]
    const float* w;     // [Cin][Cout]
    float* dx;          // [N][Cin][HW]
    float* part;        // [splits][Cin][Cout]
    int hw, items_per_image, items, items_per_split;
    int bn_relu;
};

constexpr int kProjP = 64;

__device__ __forceinline__ void buf_store1(__amdgpu_buffer_rsrc_t r, unsigned off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, off, 0, 0);
}

template <int CIB>
__global__ __launch_bounds__(128 * CIB, 2) void proj_bwd_kernel(ProjBwdArgs p) {
    constexpr int CIN = 32 * CIB, COUT = 64 * CIB, NT = 128 * CIB;
    constexpr int P = kProjP, PP = P | 1, P4 = P / 4;  // odd channel pitch: 32 lanes on 32 channels hit 32 banks
    constexpr int CSTEP = NT / P4;                     // channels between a thread's staging slots
    constexpr int XPT = CIN / CSTEP, DPT = COUT / CSTEP;
    constexpr int HC = COUT / 2;
    static_assert(CIN % CSTEP == 0 && COUT % CSTEP == 0 && HC % 4 == 0, "whole float4 slots per thread");
    __shared__ float lds[(CIN + COUT) * PP + 5 * COUT];
    float* lx = lds;
    float* ld = lds + CIN * PP;
    float* lbn = ld + COUT * PP;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int khalf = lane >> 5, j = lane & 31;
    const int cib = wid % CIB, pxb = wid / CIB;
    const unsigned uhw = (unsigned)p.hw;

    for (int e = tid; e < 5 * COUT; e += NT) lbn[e] = p.coef[e];
    // this wave's rows of w, for the whole launch
    float wr[HC];
    {
        const float4* wp = reinterpret_cast<const float4*>(p.w + (size_t)(cib * 32 + j) * COUT + khalf * HC);
#pragma unroll
        for (int q = 0; q < HC / 4; ++q) {
            const float4 v = wp[q];
            wr[4 * q] = v.x;
            wr[4 * q + 1] = v.y;
            wr[4 * q + 2] = v.z;
            wr[4 * q + 3] = v.w;
        }
    }
    f32x16 accw[CIB];
#pragma unroll
    for (int a = 0; a < CIB; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) accw[a][r] = 0.f;

    // Staging invariants, decoded once: slot i of a thread is channel c0 + i * CSTEP, pixels 4 * slot .. + 3 of the
    // item; an item only moves the buffer base.
    const int c0 = tid / P4, slot = tid % P4;
    const unsigned goff = 4u * ((unsigned)c0 * uhw + 4u * (unsigned)slot), gstep = 4u * CSTEP * uhw;
    const int loff = c0 * PP + 4 * slot;
    const unsigned xbytes = 4u * ((CIN - 1) * uhw + P), dbytes = 4u * ((COUT - 1) * uhw + P);
    const unsigned soff = 4u * ((unsigned)(cib * 32 + 4 * khalf) * uhw + (unsigned)(pxb * 32 + j));

    float4 xv[XPT], gv[DPT], yv[DPT];
    auto load_item = [&](int item) {
        const int n = item / p.items_per_image;
        const size_t px0 = (size_t)(item - n * p.items_per_image) * P;
        const __amdgpu_buffer_rsrc_t rx = buf_rsrc(p.x + (size_t)n * CIN * p.hw + px0, xbytes);
        const __amdgpu_buffer_rsrc_t rg = buf_rsrc(p.g + (size_t)n * COUT * p.hw + px0, dbytes);
        const __amdgpu_buffer_rsrc_t ry = buf_rsrc(p.bn_y + (size_t)n * COUT * p.hw + px0, dbytes);
#pragma unroll
        for (int i = 0; i < XPT; ++i) xv[i] = buf_load4(rx, goff + (unsigned)i * gstep);
#pragma unroll
        for (int i = 0; i < DPT; ++i) gv[i] = buf_load4(rg, goff + (unsigned)i * gstep);
#pragma unroll
        for (int i = 0; i < DPT; ++i) yv[i] = buf_load4(ry, goff + (unsigned)i * gstep);
    };
    auto store_item = [&]() {
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            float* dst = lx + loff + i * CSTEP * PP;
            dst[0] = xv[i].x;
            dst[1] = xv[i].y;
            dst[2] = xv[i].z;
            dst[3] = xv[i].w;
        }
#pragma unroll
        for (int i = 0; i < DPT; ++i) {
            const int c = c0 + i * CSTEP;
            const float k0 = lbn[c], k1 = lbn[COUT + c], k2 = lbn[2 * COUT + c], k3 = lbn[3 * COUT + c],
                        k4 = lbn[4 * COUT + c];
            float* dst = ld + loff + i * CSTEP * PP;
            dst[0] = bn_dy1(gv[i].x, yv[i].x, 1.f, 0.f, k0, k1, k2, k3, k4, p.bn_relu);
            dst[1] = bn_dy1(gv[i].y, yv[i].y, 1.f, 0.f, k0, k1, k2, k3, k4, p.bn_relu);
            dst[2] = bn_dy1(gv[i].z, yv[i].z, 1.f, 0.f, k0, k1, k2, k3, k4, p.bn_relu);
            dst[3] = bn_dy1(gv[i].w, yv[i].w, 1.f, 0.f, k0, k1, k2, k3, k4, p.bn_relu);
        }
    };
    auto compute_item = [&](int item) {
        // input gradient of the item: K = co, this lane half's run of HC channels
        f32x16 accx;
#pragma unroll
        for (int r = 0; r < 16; ++r) accx[r] = 0.f;
        const float* bx = ld + khalf * HC * PP + pxb * 32 + j;
#pragma unroll
        for (int s = 0; s < HC; ++s) accx = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[s], bx[s * PP], accx, 0, 0, 0);
        const int n = item / p.items_per_image;
        const size_t px0 = (size_t)(item - n * p.items_per_image) * P;
        const __amdgpu_buffer_rsrc_t rdx = buf_rsrc(p.dx + (size_t)n * CIN * p.hw + px0, xbytes);
#pragma unroll
        for (int r = 0; r < 16; ++r) buf_store1(rdx, soff + 4u * (unsigned)((r & 3) + 8 * (r >> 2)) * uhw, accx[r]);
        // weight gradient: K = the item's pixels
        const float* bw = ld + (wid * 32 + j) * PP + khalf;
        const float* aw = lx + j * PP + khalf;
#pragma unroll 8
        for (int s = 0; s < P; s += 2) {
            const float b = bw[s];
#pragma unroll
            for (int a = 0; a < CIB; ++a)
                accw[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(aw[a * 32 * PP + s], b, accw[a], 0, 0, 0);
        }
    };

    const int first = blockIdx.x * p.items_per_split;
    const int last = min(first + p.items_per_split, p.items);
    if (first < last) load_item(first);
    for (int item = first; item < last; ++item) {
        __syncthreads();  // lbn is staged / the previous item's MFMAs have read the tiles
        store_item();
        __syncthreads();
        if (item + 1 < last) load_item(item + 1);
        compute_item(item);
    }

    float* out = p.part + (size_t)blockIdx.x * CIN * COUT;
#pragma unroll
    for (int a = 0; a < CIB; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            out[(a * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf) * COUT + wid * 32 + j] = accw[a][r];
}


// 3x3 wgrad in the Winograd domain, F(2x2,3x3) transposed:
//   dW(3x3) = G^T [ sum_tiles (B^T d B) . (A dY A^T) ] G
// over the 2x2 output tiles of an item (d = the tile's 4x4 input patch, halo included).  For each of
// the 16 positions p, M_p[ci][co] = sum_tiles V_p[ci][tile] D_p[co][tile] is a GEMM with K = tiles,
// 16 MFMAs per tile pair instead of 36 per 8 pixels.  A workgroup of 2*WCI*WCO*KSPL waves owns a
// (32*WCI ci) x (32*WCO co) weight block; wave (q, g, k) accumulates the 8 positions of rows 2g and
// 2g+1 of the position grid (128 accumulators, two waves per SIMD) over its K-split share of each
// item's tiles, forming V and D per lane from the staged patch (4 patch rows x 4 columns, 2 dY
// rows x 2 columns) with adds only.
// The K-split partners fold in the Winograd domain; G^T M G is applied once per workgroup.  The
// next item's X patch and dY tile are prefetched into registers during the MFMAs: the dY tile whole
// where the registers allow, in two halves at two stage points per item where they do not (the
// schedule is described at the item loop).
// Grid (splits, ci-blocks, co-blocks).  A workgroup takes its split and channel blocks from its
// dispatch index (lf::xcd_split_block3), not from blockIdx: the channel blocks of a split stage the
// same X patches and dY tiles, so they run side by side on one XCD and find each other's lines in
// its L2.  The placement is for speed only; which items a split walks and the slab it writes
// (part[split]) do not depend on it.
// floats of (dynamic) LDS: two staging buffers (X patch + dY tile each), or the K-split scratch,
// or the epilogue's exchange of position rows 1 and 2
template <int TW, int TH, int WCI, int WCO, int KSPL>
constexpr int wgrad3_lds_floats() {
    const int pp = ((TW + 2) * (TH + 2)) | 1, dp = (TW * TH) | 1;
    const int buf = 32 * WCI * pp + 32 * WCO * dp;
    const int red = KSPL > 1 ? 16 * 1024 : 0;
    const int xch = WCI * WCO * 2 * 3 * 1024;
    const int m = 2 * buf > red ? 2 * buf : red;
    return m > xch ? m : xch;
}

template <int TW, int TH, int WCI, int WCO, int KSPL>
__global__ __launch_bounds__(64 * 2 * WCI * WCO * KSPL, 2) void wgrad3_kernel(WgradArgs p) {
    constexpr int NT = 64 * 2 * WCI * WCO * KSPL;
    constexpr int TWH = TW / 2, NTILE = TWH * (TH / 2), SH = NTILE / KSPL;  // 2x2 tiles: item, share
    static_assert(TH % 2 == 0 && TW % 4 == 0 && NTILE % KSPL == 0 && SH % 2 == 0,
                  "2x2 tiles split across waves in pairs, float4 rows");
    static_assert(SH % TWH == 0 || TWH % SH == 0, "a K-split share is whole tile rows or part of one");
    constexpr int PW = TW + 2, PH = TH + 2;
    constexpr int PP = (PW * PH) | 1;  // odd plane pitch: 32 lanes on 32 channels hit 32 banks
    constexpr int DP = (TW * TH) | 1;
    constexpr int CI_T = 32 * WCI, CO_T = 32 * WCO, NQ = WCI * WCO;
    constexpr int XSZ = CI_T * PP, DSZ = CO_T * DP;
    constexpr int BUF = XSZ + DSZ;  // one staging buffer; the kernel double-buffers
    static_assert(wgrad3_lds_floats<TW, TH, WCI, WCO, KSPL>() >= 2 * BUF, "LDS sizing");
    constexpr int TW4 = TW / 4;
    constexpr int NXI = CI_T * PH * TW4, XPT = (NXI + NT - 1) / NT;      // interior float4 items
    constexpr int NHI = CI_T * PH * 2 * 1, HPT = (NHI + NT - 1) / NT;  // halo scalars
    constexpr int NDI = CO_T * TH * TW4, DPT = (NDI + NT - 1) / NT;
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int pg = wid & 1, rest = wid >> 1;  // rows 2pg, 2pg+1 of the 4x4 position grid
    const int w_ci = rest % WCI, w_co = (rest / WCI) % WCO, w_k = rest / NQ;
    // split and channel blocks from the dispatch index: the blocks of a split share an XCD (lf::xcd_split_block3)
    const lf::Block3 blk = lf::xcd_split_block3();
    const int ci0 = blk.y * CI_T, co0 = blk.z * CO_T;
    const int khalf = lane >> 5, j = lane & 31;
    const size_t hw = (size_t)p.h * p.wd;
    const unsigned uhw = (unsigned)hw;

    f32x16 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // Row i of B^T d = d[ra] + sa * d[rb] (B^T rows: d0-d2, d1+d2, d2-d1, d1-d3); rows 2pg and 2pg+1
    // are positions 0-3 and 4-7 of the wave.  Rows of A dY (A rows: dY0, dY0+dY1, dY0-dY1, -dY1):
    // pg = 0 takes dY0 and dY1 + dY0, pg = 1 takes dY0 - dY1 and +dY1; row 3's sign, and that of
    // column 3 of A^T (taken as +u1), are undone in the epilogue.  Each lane walks tile 2kk + khalf
    // of its share.
    const int ra0 = 2 * pg, rb0 = 2 - pg, ra1 = 1, rb1 = 2 + pg;
    const float sa0 = -1.f, sa1 = pg ? -1.f : 1.f;
    const float ea = pg ? -1.f : 0.f, fb = pg ? 0.f : 1.f;
    const int t0 = w_k * SH;  // first tile of the wave's share
    const int abase = (w_ci * 32 + j) * PP + (t0 / TWH) * 2 * PW + (t0 % TWH) * 2 + 2 * khalf;
    const int bbase = (w_co * 32 + j) * DP + (t0 / TWH) * 2 * TW + (t0 % TWH) * 2 + 2 * khalf;
    const int xa0 = abase + ra0 * PW, xb0 = abase + rb0 * PW, xa1 = abase + ra1 * PW, xb1 = abase + rb1 * PW;
    const bool pro = p.in_scale != nullptr;

    // quarter q (0..3) of the wave's tile pairs from staging buffer `buf`
    constexpr int NK = SH / 2;
    auto compute_quarter = [&](auto qc, int buf) {
        constexpr int Q = decltype(qc)::value;
        constexpr int K0 = NK * Q / 4, K1 = NK * (Q + 1) / 4;
        const float* lx = lds + buf * BUF;
        const float* ld = lx + XSZ;
#pragma unroll
        for (int kk = K0; kk < K1; ++kk) {
            // tile pair 2kk, 2kk+1 of the share: same tile row (TWH is even)
            const int tr = (2 * kk) / TWH, tc = (2 * kk) % TWH;
            const int xoff = tr * 2 * PW + tc * 2, doff = tr * 2 * TW + tc * 2;
            float t[2][4], u[2][2];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                t[0][c] = fmaf(sa0, lx[xb0 + xoff + c], lx[xa0 + xoff + c]);
                t[1][c] = fmaf(sa1, lx[xb1 + xoff + c], lx[xa1 + xoff + c]);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float y0 = ld[bbase + doff + c], y1 = ld[bbase + TW + doff + c];
                u[0][c] = fmaf(ea, y1, y0);
                u[1][c] = fmaf(fb, y0, y1);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float v[4] = {t[h][0] - t[h][2], t[h][1] + t[h][2], t[h][2] - t[h][1], t[h][1] - t[h][3]};
                const float d[4] = {u[h][0], u[h][0] + u[h][1], u[h][0] - u[h][1], u[h][1]};
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc[h * 4 + c] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[c], d[c], acc[h * 4 + c], 0, 0, 0);
            }
        }
    };
    using Q0 = std::integral_constant<int, 0>;
    using Q1 = std::integral_constant<int, 1>;
    using Q2 = std::integral_constant<int, 2>;
    using Q3 = std::integral_constant<int, 3>;

    const int first = blk.x * p.items_per_split;
    const int last = min(first + p.items_per_split, p.items);
    const int tiles = p.tiles_x * p.tiles_y;

    if (p.vec_ok) {  // every tile is full in x (host guarantees W % TW == 0 for this path)
        // With four float4 of dY per thread (CO_T = 64 over a 128-pixel tile) a whole prefetched dY tile (dv, yv,
        // alpha / add: 40 registers) does not fit beside the 128 accumulators.  Those variants hold half of the
        // thread's slots at a time: slots [0, DH) are the tile's first CO_T / 2 channels, [DH, DPT) the others.
        constexpr bool kSplitD = DPT > 2;
        static_assert(!kSplitD || DPT == 4, "the dY tile is prefetched whole or in two halves");
        constexpr int DH = kSplitD ? DPT / 2 : DPT;  // dY slots a thread holds in registers
        float4 xv[XPT], dv[DH], yv[DH];
        float xh[HPT], dal[DH], dad[DH];
        unsigned xok = 0, dok = 0;
        const bool bn = p.bn_y != nullptr;
        // producer BatchNorm scale/shift of this workgroup's CI_T channels, staged once in LDS
        __shared__ float lsc[kMaxProC / 2];
        if (pro) {
            for (int c = tid; c < CI_T; c += NT) {
                const int gc = ci0 + c;
                lsc[c] = gc < p.cin ? p.in_scale[gc] : 1.f;
                lsc[kMaxProC / 4 + c] = gc < p.cin ? p.in_shift[gc] : 0.f;
            }
        }
        // BatchNorm-backward coefficients of this workgroup's CO_T channels
        __shared__ float lbn[5 * CO_T];
        if (bn) {
            for (int e = tid; e < 5 * CO_T; e += NT) {
                const int kk = e / CO_T, gc = co0 + (e - kk * CO_T);
                lbn[e] = gc < p.cout ? p.bn_coef[(size_t)kk * p.cout + gc] : 0.f;
            }
        }
        // Per-thread staging invariants, decoded once: an item only moves the tile origin.
        //   *_g: BYTE offset of the element from the patch origin (image n, channel block, row
        //        ty0-1, column tx0-1 for X; row ty0, column tx0 for dY), kBufOob when the
        //        thread's slot / channel does not exist;
        //   *_l: LDS float index | (patch row << 16)
        unsigned xg[XPT], hg[HPT], dg[DPT];
        unsigned xl[XPT], hl[HPT], dl[DPT];
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int e = tid + i * NT;
            const int c = e / (PH * TW4), rem = e - c * (PH * TW4);
            const int py = rem / TW4, slot = rem - py * TW4;
            const bool ok = e < NXI && ci0 + c < p.cin;
            xg[i] = ok ? 4u * ((unsigned)c * uhw + (unsigned)py * (unsigned)p.wd + 1u + 4u * (unsigned)slot) : kBufOob;
            xl[i] = (unsigned)(c * PP + py * PW + 1 + 4 * slot) | ((unsigned)py << 16);
        }
#pragma unroll
        for (int i = 0; i < HPT; ++i) {
            const int e = tid + i * NT;
            const int c = e / (PH * 2), rem = e - c * (PH * 2);
            const int py = rem >> 1, side = rem & 1;
            const bool ok = e < NHI && ci0 + c < p.cin;
            hg[i] = ok ? 4u * ((unsigned)c * uhw + (unsigned)py * (unsigned)p.wd + (side ? TW + 1u : 0u)) : kBufOob;
            hl[i] = (unsigned)(c * PP + py * PW + (side ? PW - 1 : 0)) | ((unsigned)py << 16) |
                    ((unsigned)side << 30);
        }
#pragma unroll
        for (int i = 0; i < DPT; ++i) {
            const int e = tid + i * NT;
            const int c = e / (TH * TW4), rem = e - c * (TH * TW4);
            const int py = rem / TW4, slot = rem - py * TW4;
            const bool ok = e < NDI && co0 + c < p.cout;
            dg[i] = ok ? 4u * ((unsigned)c * uhw + (unsigned)py * (unsigned)p.wd + 4u * (unsigned)slot) : kBufOob;
            dl[i] = (unsigned)(c * DP + rem * 4) | ((unsigned)py << 16);
        }
        const unsigned xbytes = 4u * ((unsigned)min(CI_T, p.cin - ci0) * uhw + (unsigned)p.wd + 1u);
        const unsigned dbytes = 4u * (unsigned)min(CO_T, p.cout - co0) * uhw;
        // Issue the loads of an item's X patch (with_x) and / or of half `dhalf` of its dY tile (-1: no dY; a
        // variant that holds the whole tile has only half 0).  Nothing here is conditional: where `live` is false
        // (there is no such item) every load takes the out-of-range offset, which fetches zeros and no memory.
        auto load_item = [&](int item, bool with_x, int dhalf, bool live) {
            const int n = item / tiles, t = item - n * tiles;
            const int tx0 = (t % p.tiles_x) * TW, ty0 = (t / p.tiles_x) * TH;
            const size_t torg = (size_t)ty0 * p.wd + tx0;
            const size_t nl = (size_t)n;
            // patch origin = one row up, one column left of the tile (never dereferenced there:
            // rows / columns outside the image get the out-of-range offset)
            const __amdgpu_buffer_rsrc_t rx =
                buf_rsrc(p.x + (nl * p.cin + ci0) * hw + torg - (size_t)p.wd - 1, xbytes);
            const __amdgpu_buffer_rsrc_t rd = buf_rsrc(p.dy + (nl * p.cout + co0) * hw + torg, dbytes);
            if (with_x) {
            xok = 0;
#pragma unroll
            for (int i = 0; i < XPT; ++i) {
                const unsigned gy = (unsigned)(ty0 + (int)((xl[i] >> 16) & 0xffu) - 1);
                const bool ok = live && xg[i] != kBufOob && gy < (unsigned)p.h;
                xv[i] = buf_load4(rx, ok ? xg[i] : kBufOob);
                xok |= (ok ? 1u : 0u) << i;
            }
#pragma unroll
            for (int i = 0; i < HPT; ++i) {
                const unsigned gy = (unsigned)(ty0 + (int)((hl[i] >> 16) & 0xffu) - 1);
                const bool side = (hl[i] >> 30) & 1u;
                const bool ok = live && hg[i] != kBufOob && gy < (unsigned)p.h && (side ? tx0 + TW < p.wd : tx0 > 0);
                xh[i] = buf_load1(rx, ok ? hg[i] : kBufOob);
                xok |= (ok ? 1u : 0u) << (16 + i);
            }
            }
            if (dhalf < 0) return;
            const int s0 = dhalf * DH;  // the half's first slot
            dok = 0;
#pragma unroll
            for (int i = 0; i < DH; ++i) {
                const unsigned gy = (unsigned)(ty0 + (int)((dl[s0 + i] >> 16) & 0xffu));
                const bool ok = live && dg[s0 + i] != kBufOob && gy < (unsigned)p.h;
                dv[i] = buf_load4(rd, ok ? dg[s0 + i] : kBufOob);
                dok |= (ok ? 1u : 0u) << i;
            }
            if (bn) {
                const __amdgpu_buffer_rsrc_t ry =
                    buf_rsrc(p.bn_y + ((size_t)n * p.cout + co0) * hw + torg, dbytes);
#pragma unroll
                for (int i = 0; i < DH; ++i) yv[i] = buf_load4(ry, (dok >> i & 1u) ? dg[s0 + i] : kBufOob);
                if (p.bn_alpha != nullptr) {
#pragma unroll
                    for (int i = 0; i < DH; ++i) {
                        const int e = tid + (s0 + i) * NT;
                        const int gc = min(co0 + e / (TH * TW4), p.cout - 1);
                        dal[i] = p.bn_alpha[(size_t)n * p.cout + gc];
                        dad[i] = p.bn_add != nullptr ? p.bn_add[(size_t)n * p.cout + gc] : 0.f;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < DH; ++i) {
                        dal[i] = 1.f;
                        dad[i] = 0.f;
                    }
                }
            }
        };
        // write what load_item(item, with_x, dhalf) fetched into staging buffer `buf`
        auto store_item = [&](int item, int buf, bool with_x, int dhalf) {
            float* lx = lds + buf * BUF;
            float* ld = lx + XSZ;
            if (with_x) {
#pragma unroll
            for (int i = 0; i < XPT; ++i) {
                if (tid + i * NT < NXI) {
                    const int c = (tid + i * NT) / (PH * TW4);
                    float4 v = xv[i];  // padding was fetched as zeros
                    if (pro && (xok >> i & 1u)) {
                        const float sc = lsc[c], sh = lsc[kMaxProC / 4 + c];
                        v.x = pro_apply(v.x, sc, sh, p.in_relu);
                        v.y = pro_apply(v.y, sc, sh, p.in_relu);
                        v.z = pro_apply(v.z, sc, sh, p.in_relu);
                        v.w = pro_apply(v.w, sc, sh, p.in_relu);
                    }
                    float* dst = lx + (xl[i] & 0xffffu);
                    {
                        dst[0] = v.x;
                        dst[1] = v.y;
                        dst[2] = v.z;
                        dst[3] = v.w;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < HPT; ++i) {
                if (tid + i * NT < NHI) {
                    const int c = (tid + i * NT) / (PH * 2);
                    float v = xh[i];
                    if (pro && (xok >> (16 + i) & 1u))
                        v = pro_apply(v, lsc[c], lsc[kMaxProC / 4 + c], p.in_relu);
                    lx[hl[i] & 0xffffu] = v;
                }
            }
            }
            if (dhalf < 0) return;
            const int s0 = dhalf * DH;
            const int sn = item / tiles, st = item - sn * tiles;
            const int stx0 = (st % p.tiles_x) * TW, sty0 = (st / p.tiles_x) * TH;
            float* dyo = bn ? p.dy_out + ((size_t)sn * p.cout + co0) * hw + (size_t)sty0 * p.wd + stx0 : nullptr;
#pragma unroll
            for (int i = 0; i < DH; ++i) {
                if (tid + (s0 + i) * NT < NDI) {
                    const int c = (tid + (s0 + i) * NT) / (TH * TW4);
                    float4 v = dv[i];
                    if (bn && (dok >> i & 1u)) {
                        const float c0 = lbn[c], c1 = lbn[CO_T + c], c2 = lbn[2 * CO_T + c],
                                    c3 = lbn[3 * CO_T + c], c4 = lbn[4 * CO_T + c];
                        v.x = bn_dy1(v.x, yv[i].x, dal[i], dad[i], c0, c1, c2, c3, c4, p.bn_relu);
                        v.y = bn_dy1(v.y, yv[i].y, dal[i], dad[i], c0, c1, c2, c3, c4, p.bn_relu);
                        v.z = bn_dy1(v.z, yv[i].z, dal[i], dad[i], c0, c1, c2, c3, c4, p.bn_relu);
                        v.w = bn_dy1(v.w, yv[i].w, dal[i], dad[i], c0, c1, c2, c3, c4, p.bn_relu);
                        if (blk.y == 0 && p.dy_out != nullptr)
                            *reinterpret_cast<float4*>(dyo + (dg[s0 + i] >> 2)) = v;
                    }
                    float* dst = ld + (dl[s0 + i] & 0xffffu);
                    {
                        dst[0] = v.x;
                        dst[1] = v.y;
                        dst[2] = v.z;
                        dst[3] = v.w;
                    }
                }
            }
        };
        // Double-buffered staging, one barrier per item: while an item's MFMAs run from one buffer the next
        // item is written into the other from registers loaded well before, and the loads after those are
        // issued.  No load is stored at the stage point that issued it.
        // The two waves sharing a SIMD (wid, wid+4) move through their MFMAs in lock step, so they stage at
        // different quarters: while one writes LDS the other keeps the MFMA pipe busy.
        //   whole dY tile in registers: one stage point per item (after quarter 0 or 2), which stores item
        //     idx+1 (X patch and dY tile, loaded a full item earlier) and loads item idx+2;
        //   dY tile in halves (kSplitD): two stage points per item, half an item apart (after quarters 0 and
        //     2, or 1 and 3).  The first stores X and dY half 0 of item idx+1 and loads dY half 1 of idx+1,
        //     then X of idx+2; the second stores that half 1 and loads dY half 0 of idx+2.  A half is in
        //     flight over two quarters of MFMAs, the X patch over a whole item.
        // The variants that hold the whole tile keep the branch around their loads (idx + 2 < count): with a
        // `live` flag in its place they compiled to slower loops (profiles/r07_a_wgrad_schedule.md).
        int cur = 0;
        const int count = last - first;
        // clamped where loads are issued for items that do not exist: a dead load's item is the split's last
        auto nth = [&](int idx) { return first + (kSplitD ? min(idx, count - 1) : idx); };
        if (count > 0) {
            load_item(nth(0), true, 0, true);
            __syncthreads();  // lsc / lbn are staged
            store_item(nth(0), 0, true, 0);
            if (kSplitD) {
                load_item(nth(0), false, 1, true);
                store_item(nth(0), 0, false, 1);
            }
            if (kSplitD)
                load_item(nth(1), true, 0, count > 1);
            else if (count > 1)
                load_item(nth(1), true, 0, true);
        }
        __syncthreads();
        const int stage_q = (wid >> 2) & 1;
        for (int idx = 0; idx < count; ++idx) {
            const bool more = idx + 1 < count;
            auto stage_a = [&]() {
                store_item(nth(idx + 1), cur ^ 1, true, 0);
                if (kSplitD) {
                    load_item(nth(idx + 1), false, 1, true);
                    load_item(nth(idx + 2), true, -1, idx + 2 < count);
                } else if (idx + 2 < count) {
                    load_item(nth(idx + 2), true, 0, true);
                }
            };
            auto stage_b = [&]() {
                store_item(nth(idx + 1), cur ^ 1, false, 1);
                load_item(nth(idx + 2), false, 0, idx + 2 < count);
            };
            compute_quarter(Q0{}, cur);
            if (more && stage_q == 0) stage_a();
            compute_quarter(Q1{}, cur);
            if (kSplitD && more && stage_q == 1) stage_a();
            compute_quarter(Q2{}, cur);
            if (kSplitD && more && stage_q == 0) stage_b();
            if (!kSplitD && more && stage_q == 1) stage_a();
            compute_quarter(Q3{}, cur);
            if (kSplitD && more && stage_q == 1) stage_b();
            __syncthreads();
            cur ^= 1;
        }
    } else {
        float* lx = lds;
        float* ld = lds + XSZ;
        // scalar staging for ragged shapes
        for (int item = first; item < last; ++item) {
            const int n = item / tiles, t = item - n * tiles;
            const int tx0 = (t % p.tiles_x) * TW, ty0 = (t / p.tiles_x) * TH;
            const float* xin = p.x + (size_t)n * p.cin * hw;
            const float* din = p.dy + (size_t)n * p.cout * hw;
            __syncthreads();
            for (int e = tid; e < CI_T * PW * PH; e += NT) {
                const int c = e / (PW * PH), rem = e - c * (PW * PH);
                const int py = rem / PW, px = rem - py * PW;
                const int gc = ci0 + c, gy = ty0 + py - 1, gx = tx0 + px - 1;
                float v = 0.f;
                if (gc < p.cin && gy >= 0 && gy < p.h && gx >= 0 && gx < p.wd) {
                    v = xin[(unsigned)gc * uhw + (unsigned)gy * (unsigned)p.wd + (unsigned)gx];
                    if (pro) v = pro_apply(v, p.in_scale[gc], p.in_shift[gc], p.in_relu);
                }
                lx[c * PP + rem] = v;
            }
            for (int e = tid; e < CO_T * TW * TH; e += NT) {
                const int c = e / (TW * TH), rem = e - c * (TW * TH);
                const int py = rem / TW, px = rem - py * TW;
                const int gc = co0 + c, gy = ty0 + py, gx = tx0 + px;
                float v = 0.f;
                if (gc < p.cout && gy < p.h && gx < p.wd)
                    v = din[(unsigned)gc * uhw + (unsigned)gy * (unsigned)p.wd + (unsigned)gx];
                ld[c * DP + rem] = v;
            }
            __syncthreads();
            compute_quarter(Q0{}, 0);
            compute_quarter(Q1{}, 0);
            compute_quarter(Q2{}, 0);
            compute_quarter(Q3{}, 0);
        }
    }

    // K-split partner waves fold into k = 0 through LDS in the Winograd domain, one (ci,co) block per
    // round (fixed order)
    const int q = w_co * WCI + w_ci;
#pragma unroll 1
    for (int k = 1; k < KSPL; ++k) {
#pragma unroll 1
        for (int qq = 0; qq < NQ; ++qq) {
            __syncthreads();
            if (w_k == k && q == qq) {
#pragma unroll
                for (int c = 0; c < 8; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) lds[(pg * 8 + c) * 1024 + r * 64 + lane] = acc[c][r];
            }
            __syncthreads();
            if (w_k == 0 && q == qq) {
#pragma unroll
                for (int c = 0; c < 8; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[c][r] += lds[(pg * 8 + c) * 1024 + r * 64 + lane];
            }
        }
    }

    // G^T M G.  Each wave applies G on the right to its two position rows (column 3 enters with the
    // sign taken in D): P[0] = M0 + (M1+M2)/2, P[1] = (M1-M2)/2, P[2] = (M1+M2)/2 - M3.  P1 and P2 are
    // exchanged through LDS; wave g = 0 forms filter rows 0 and 1, g = 1 filter row 2:
    //   dW0 = P0 + (P1+P2)/2,  dW1 = (P1-P2)/2,  dW2 = (P1+P2)/2 - P3  (P3 entered with its sign taken)
    auto prow = [&](int h, int s, int r) {  // P[s] of the wave's position row h (0 or 1)
        const float m0 = acc[h * 4][r], m1 = acc[h * 4 + 1][r], m2 = acc[h * 4 + 2][r], m3 = acc[h * 4 + 3][r];
        const float hs = (m1 + m2) * 0.5f;
        return s == 0 ? m0 + hs : (s == 1 ? (m1 - m2) * 0.5f : hs - m3);
    };
    float* xch = lds + (size_t)q * (2 * 3 * 1024);
    __syncthreads();  // the staging buffers / K-split scratch are no longer read
    if (w_k == 0) {  // g = 0 publishes P1 (its second row), g = 1 publishes P2 (its first)
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                xch[(pg * 3 + s) * 1024 + r * 64 + lane] = pg ? prow(0, s, r) : prow(1, s, r);
    }
    __syncthreads();
    if (w_k == 0) {
        float* out = p.part + (size_t)blk.x * p.cin * 9 * p.cout;
        const int co = co0 + w_co * 32 + j;
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p1 = xch[s * 1024 + r * 64 + lane], p2 = xch[(3 + s) * 1024 + r * 64 + lane];
                const float hs = (p1 + p2) * 0.5f;
                const int ci = ci0 + w_ci * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                if (ci < p.cin && co < p.cout) {
                    float* o = out + ((size_t)ci * 9 + s) * p.cout + co;
                    if (pg == 0) {
                        o[0] = prow(0, s, r) + hs;
                        o[3 * p.cout] = (p1 - p2) * 0.5f;
                    } else {
                        o[6 * p.cout] = hs - prow(1, s, r);
                    }
                }
            }
    }
}

// Small-Cin 3x3 wgrad (the stem, Cin*9 <= 32): D[(ci,tap)][co] — the 27 (ci, tap) pairs ride
// the MFMA's M dimension, so a pixel pair costs ONE MFMA per 32 output channels instead of 9.
// Tile 32 x 8; 4 waves split the 8 rows; X patch [cin][10][34] (+ one zero plane for the
// unused M rows), dY tile [32][256].  grid = (splits, 1, cout/32 blocks).
template <int TW, int TH>
__global__ __launch_bounds__(kThreads, 4) void wgrad_smallcin_kernel(WgradArgs p) {
    constexpr int PW = TW + 2, PH = TH + 2, PP = PW * PH;
    constexpr int DP = (TW * TH) | 1;
    constexpr int MAXC = 3;
    constexpr int TW4 = TW / 4;
    __shared__ float lds[(MAXC + 1) * PP + 32 * DP];
    float* lx = lds;
    float* ld = lds + (MAXC + 1) * PP;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int khalf = lane >> 5, j = lane & 31;
    const int co0 = blockIdx.z * 32;
    const size_t hw = (size_t)p.h * p.wd;
    const unsigned uhw = (unsigned)hw;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // lane j < cin*9 reads channel j/9 at tap j%9; other lanes read the zero plane
    const int ktot = p.cin * 9;
    const int aci = j < ktot ? j / 9 : MAXC, atap = j < ktot ? j % 9 : 0;
    const int abase = aci * PP + (atap / 3) * PW + (atap % 3) + khalf;
    const int bbase = j * DP + khalf;
    for (int i = tid; i < PP; i += kThreads) lx[MAXC * PP + i] = 0.f;
    const int first = blockIdx.x * p.items_per_split;
    const int last = min(first + p.items_per_split, p.items);
    const int tiles = p.tiles_x * p.tiles_y;
    const bool pro = p.in_scale != nullptr;
    const bool bn = p.bn_y != nullptr;  // dY = BatchNorm backward of p.dy, formed while staging
    __shared__ float lbn[5 * 32];
    if (bn) {
        for (int e = tid; e < 5 * 32; e += kThreads) {
            const int kk = e / 32, gc = co0 + (e - kk * 32);
            lbn[e] = gc < p.cout ? p.bn_coef[(size_t)kk * p.cout + gc] : 0.f;
        }
    }
    constexpr int ROWS = TH / 4;
    for (int item = first; item < last; ++item) {
        const int n = item / tiles, t = item - n * tiles;
        const int tx0 = (t % p.tiles_x) * TW, ty0 = (t / p.tiles_x) * TH;
        const float* xin = p.x + (size_t)n * p.cin * hw;
        const float* din = p.dy + (size_t)n * p.cout * hw;
        __syncthreads();
        for (int e = tid; e < p.cin * PP; e += kThreads) {
            const int c = e / PP, rem = e - c * PP;
            const int py = rem / PW, px = rem - py * PW;
            const int gy = ty0 + py - 1, gx = tx0 + px - 1;
            float v = 0.f;
            if (gy >= 0 && gy < p.h && gx >= 0 && gx < p.wd) {
                v = xin[(unsigned)c * uhw + (unsigned)gy * (unsigned)p.wd + (unsigned)gx];
                if (pro) v = pro_apply(v, p.in_scale[c], p.in_shift[c], p.in_relu);
            }
            lx[e] = v;
        }
        if (p.vec_ok) {
#pragma unroll
            for (int i = 0; i < 32 * TH * TW4 / kThreads; ++i) {
                const int e = tid + i * kThreads;
                const int c = e / (TH * TW4), rem = e - c * (TH * TW4);
                const int py = rem / TW4, slot = rem - py * TW4;
                const int gc = co0 + c, gy = ty0 + py;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gc < p.cout && gy < p.h) {
                    const size_t off = (size_t)gc * uhw + (size_t)gy * p.wd + tx0 + 4 * slot;
                    v = *reinterpret_cast<const float4*>(din + off);
                    if (bn) {
                        const float4 yv = *reinterpret_cast<const float4*>(
                            p.bn_y + (size_t)n * p.cout * hw + off);
                        const float al = p.bn_alpha ? p.bn_alpha[(size_t)n * p.cout + gc] : 1.f;
                        const float ad = p.bn_add ? p.bn_add[(size_t)n * p.cout + gc] : 0.f;
                        const float c0 = lbn[c], c1 = lbn[32 + c], c2 = lbn[64 + c], c3 = lbn[96 + c],
                                    c4 = lbn[128 + c];
                        v.x = bn_dy1(v.x, yv.x, al, ad, c0, c1, c2, c3, c4, p.bn_relu);
                        v.y = bn_dy1(v.y, yv.y, al, ad, c0, c1, c2, c3, c4, p.bn_relu);
                        v.z = bn_dy1(v.z, yv.z, al, ad, c0, c1, c2, c3, c4, p.bn_relu);
                        v.w = bn_dy1(v.w, yv.w, al, ad, c0, c1, c2, c3, c4, p.bn_relu);
                        if (blockIdx.y == 0 && p.dy_out != nullptr)
                            *reinterpret_cast<float4*>(p.dy_out + (size_t)n * p.cout * hw + off) = v;
                    }
                }
                float* dst = ld + c * DP + rem * 4;
                dst[0] = v.x;
                dst[1] = v.y;
                dst[2] = v.z;
                dst[3] = v.w;
            }
        } else {
            for (int e = tid; e < 32 * TW * TH; e += kThreads) {
                const int c = e / (TW * TH), rem = e - c * (TW * TH);
                const int py = rem / TW, px = rem - py * TW;
                const int gc = co0 + c, gy = ty0 + py, gx = tx0 + px;
                float v = 0.f;
                if (gc < p.cout && gy < p.h && gx < p.wd)
                    v = din[(unsigned)gc * uhw + (unsigned)gy * (unsigned)p.wd + (unsigned)gx];
                ld[c * DP + rem] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            const int row = wid * ROWS + rr;
#pragma unroll 8
            for (int xx = 0; xx < TW; xx += 2) {
                const float a = lx[abase + row * PW + xx];
                const float b = ld[bbase + row * TW + xx];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
        }
    }
    // fold the 4 row-split waves through LDS
#pragma unroll 1
    for (int k = 1; k < 4; ++k) {
        __syncthreads();
        if (wid == k)
#pragma unroll
            for (int r = 0; r < 16; ++r) lds[r * 64 + lane] = acc[r];
        __syncthreads();
        if (wid == 0)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] += lds[r * 64 + lane];
    }
    if (wid == 0) {
        float* out = p.part + (size_t)blockIdx.x * p.cin * 9 * p.cout;
        const int co = co0 + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kidx = (r & 3) + 8 * (r >> 2) + 4 * khalf;  // = ci*9 + tap
            if (kidx < ktot && co < p.cout) out[(size_t)kidx * p.cout + co] = acc[r];
        }
    }
}

// dst[g][i] = sum over slabs s in group g of part[s][i]; with one group and dw given this is
// the final dw = beta*dw + sum.  Fixed order -> deterministic.
__global__ __launch_bounds__(kThreads) void slab_reduce_kernel(const float* __restrict__ part,
                                                               float* __restrict__ dst, size_t count,
                                                               int nslabs, int per_group, float beta,
                                                               int final_pass) {
    const int g = blockIdx.y;
    const int s0 = g * per_group, s1 = min(s0 + per_group, nslabs);
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < count;
         i += (size_t)gridDim.x * kThreads) {
        float s = 0.f;
        for (int k = s0; k < s1; ++k) s += part[(size_t)k * count + i];
        float* o = dst + (size_t)g * count + i;
        *o = (final_pass && beta != 0.f) ? fmaf(beta, *o, s) : s;
    }
}

// [Cin][T][Cout] -> dgrad weights [Cout][T flipped][Cin]
__global__ __launch_bounds__(kThreads) void weight_dgrad_kernel(const float* __restrict__ w,
                                                                float* __restrict__ wt, int cin,
                                                                int taps, int cout) {
    const int total = cin * taps * cout;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < total; i += gridDim.x * kThreads) {
        const int ci = i % cin, t = (i / cin) % taps, co = i / (cin * taps);
        wt[i] = w[((size_t)ci * taps + (taps - 1 - t)) * cout + co];
    }
}

// The 3x3 filters in the Winograd domain, once per layer, role and step: w [Cin][9][Cout] ->
// U = G g G^T, 16 floats per filter.  Forward role: u[ci][co] from the taps of w[ci][.][co].  Input-gradient
// role (dgrad != 0): the convolution's channels swap and its taps flip, u[co][ci] from w[ci][8 - tap][co]
// (what weight_dgrad_kernel followed by the forward role gives, in one launch).
// Layout [Cin'][Cout'][16] (primed: the convolution's own channels in that role): the slice conv_wino_kernel
// stages per K-chunk and cout tile is then one run of CT * 64 contiguous bytes per channel, every filter
// 64-byte aligned whatever Cout is, so the copy takes 16-byte lanes on the ragged shapes too.  (Position-major
// [16][Cin][Cout] would cut the same slice into 16 * kKC runs of CT * 4 bytes.)
__global__ __launch_bounds__(kThreads) void wino_filters_kernel(const float* __restrict__ w,
                                                                float* __restrict__ u, int cin, int cout,
                                                                int dgrad) {
    const int total = cin * cout;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < total; i += gridDim.x * kThreads) {
        const int ci = i / cout, co = i - ci * cout;
        float g[9], t[16];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) g[tap] = w[((size_t)ci * 9 + (dgrad ? 8 - tap : tap)) * cout + co];
        wino_filter(g, t);
        float4* dst = reinterpret_cast<float4*>(u + (dgrad ? (size_t)co * cin + ci : (size_t)i) * 16);
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) dst[q4] = make_float4(t[4 * q4], t[4 * q4 + 1], t[4 * q4 + 2], t[4 * q4 + 3]);
    }
}

// ---------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------
// ct: the direct kernel's cout tile (launch_fwd gives the Winograd kernels' own)
struct FwdVariant {
    int tw, th, ct;
};
constexpr FwdVariant kFwdVariants[] = {{32, 8, 32}, {32, 8, 64}, {16, 16, 32}, {16, 16, 64},
                                       {28, 8, 128}, {32, 8, 128}, {56, 8, 64}};
constexpr int kNumFwd = sizeof(kFwdVariants) / sizeof(kFwdVariants[0]);

inline long long padded_work(const FwdVariant& v, int h, int w, int cout) {
    const long long tx = (w + v.tw - 1) / v.tw, ty = (h + v.th - 1) / v.th,
                    tc = (cout + v.ct - 1) / v.ct;
    return tx * v.tw * ty * v.th * tc * v.ct;
}

// the stem (Cin = 3) takes its own instantiation of variant 0
inline bool fwd_small_cin(int taps, int variant, int cin) { return taps == 9 && variant == 0 && cin <= 4; }

// the shape half of ConvArgs::vec_ok (the other half: 16-byte aligned x and w)
inline bool fwd_vec_shape(int wd, int cout) { return wd % 4 == 0 && cout % 4 == 0; }

// K-chunk of 8 input channels everywhere (16 measured slower in the direct kernel: more prefetch registers,
// fewer resident waves).
// gx x gz: tiles x strips; grid.y = cout / the kernel's cout tile.
int launch_fwd(int ksize, int variant, const ConvArgs& a, unsigned gx, unsigned gz, hipStream_t s) {
    const auto grid = [&](int ct) { return dim3(gx, (a.cout + ct - 1) / ct, gz); };
    const dim3 g = grid(kFwdVariants[variant].ct);  // the direct kernel's cout tile
    if (ksize == 3 && fwd_small_cin(9, variant, a.cin)) {
        // the stem (Cin = 3): a 4-channel K-chunk instead of 8 halves the MFMAs spent on zeros
        conv_mfma_kernel<9, 32, 8, 1, 1, 4, 2, 4><<<g, kThreads, 0, s>>>(a);
        return LF_OK;
    }
    if (ksize == 3) {
        // Every other 3x3 launch runs Winograd F(2x2,3x3).  The kernel keeps the variant's spatial
        // tile (the statistics partials are laid out per tile) but takes 32 couts (16 for the
        // 112-tile 56x8 variant): 16 positions x 4 accumulators per (cout, tile) leave room for 128
        // per wave.  Variants 1, 3 and 5 have the tile of 0, 2 and 0 with a wider ct, so the 3x3
        // argmin never picks them.
        switch (variant) {
            case 0: conv_wino_kernel<32, 8, 2, 1, false><<<grid(32), kThreads, 0, s>>>(a); break;
            case 2: conv_wino_kernel<16, 16, 2, 1, false><<<grid(32), kThreads, 0, s>>>(a); break;
            case 4: conv_wino_kernel<28, 8, 2, 1, true><<<grid(32), kThreads, 0, s>>>(a); break;
            case 6: conv_wino_kernel<56, 8, 1, 2, false><<<grid(16), kThreads, 0, s>>>(a); break;
            default: return LF_ERR_INVALID;
        }
        return LF_OK;
    }
    switch (variant) {
        case 0: conv_mfma_kernel<1, 32, 8, 1, 1, 4, 2, 8><<<g, kThreads, 0, s>>>(a); break;
        case 1: conv_mfma_kernel<1, 32, 8, 1, 2, 4, 2, 8><<<g, kThreads, 0, s>>>(a); break;
        case 2: conv_mfma_kernel<1, 16, 16, 1, 1, 4, 2, 8><<<g, kThreads, 0, s>>>(a); break;
        case 3: conv_mfma_kernel<1, 16, 16, 1, 2, 4, 2, 8><<<g, kThreads, 0, s>>>(a); break;
        case 4: conv_mfma_kernel<1, 28, 8, 4, 1, 1, 7, 8, true><<<g, kThreads, 0, s>>>(a); break;
        case 5: conv_mfma_kernel<1, 32, 8, 2, 2, 2, 4, 8><<<g, kThreads, 0, s>>>(a); break;
        case 6: conv_mfma_kernel<1, 56, 8, 2, 1, 2, 7, 8><<<g, kThreads, 0, s>>>(a); break;
        default: return LF_ERR_INVALID;
    }
    return LF_OK;
}

struct WgVariant {
    int tw, th, ci_t, co_t, kspl;
};
constexpr WgVariant kWgVariants[] = {{32, 4, 32, 32, 4}, {16, 8, 32, 64, 2}, {16, 4, 64, 64, 1},
                                     {28, 2, 64, 64, 1}};
constexpr int kWgSmallCin = 5;  // variant id of wgrad_smallcin_kernel<32, 8> (4 is not used)

// wgrad3 uses more than the 64 KB of LDS a kernel gets by default: raise the limit once
template <int TW, int TH, int WCI, int WCO, int KSPL>
int launch_wgrad3(const WgradArgs& a, dim3 grid, hipStream_t s) {
    constexpr size_t bytes = (size_t)wgrad3_lds_floats<TW, TH, WCI, WCO, KSPL>() * sizeof(float);
    static bool raised = false;
    if (!raised) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad3_kernel<TW, TH, WCI, WCO, KSPL>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
            lf::set_error("lf_conv2d_wgrad: cannot reserve %zu bytes of LDS", bytes);
            return LF_ERR_LAUNCH;
        }
        raised = true;
    }
    wgrad3_kernel<TW, TH, WCI, WCO, KSPL><<<grid, 64 * 2 * WCI * WCO * KSPL, bytes, s>>>(a);
    return LF_OK;
}

int launch_wgrad(int ksize, int variant, const WgradArgs& a, dim3 grid, hipStream_t s) {
    if (ksize == 3) {
        switch (variant) {
            case 0: return launch_wgrad3<32, 4, 1, 1, 4>(a, grid, s);
            case 1: return launch_wgrad3<16, 8, 1, 2, 2>(a, grid, s);
            case 2: return launch_wgrad3<16, 4, 2, 2, 1>(a, grid, s);
            case 3: return launch_wgrad3<28, 2, 2, 2, 1>(a, grid, s);
            default: return LF_ERR_INVALID;
        }
    } else {
        switch (variant) {
            case 0: wgrad_mfma_kernel<32, 4, 1, 1, 4><<<grid, kThreads, 0, s>>>(a); break;
            case 1: wgrad_mfma_kernel<16, 8, 1, 2, 2><<<grid, kThreads, 0, s>>>(a); break;
            case 2: wgrad_mfma_kernel<16, 4, 2, 2, 1><<<grid, kThreads, 0, s>>>(a); break;
            case 3: wgrad_mfma_kernel<28, 2, 2, 2, 1><<<grid, kThreads, 0, s>>>(a); break;
            default: return LF_ERR_INVALID;
        }
    }
    return LF_OK;
}

struct WgPlan {
    int variant, tw, tiles_x, tiles_y, items, splits, items_per_split, gy, gz;
};

WgPlan plan_wgrad(int n, int cin, int cout, int h, int w, int ksize) {
    WgPlan best{};
    if (ksize == 3 && cin * 9 <= 32) {
        best.variant = kWgSmallCin;
        best.tw = 32;
        best.tiles_x = (w + 31) / 32;
        best.tiles_y = (h + 7) / 8;
        best.gy = 1;
        best.gz = (cout + 31) / 32;
    } else {
        long long best_cost = -1;
        for (int v = 0; v < (int)(sizeof(kWgVariants) / sizeof(kWgVariants[0])); ++v) {
            const WgVariant& k = kWgVariants[v];
            const long long tx = (w + k.tw - 1) / k.tw, ty = (h + k.th - 1) / k.th;
            const long long gy = (cin + k.ci_t - 1) / k.ci_t, gz = (cout + k.co_t - 1) / k.co_t;
            const long long cost = tx * k.tw * ty * k.th * gy * k.ci_t * gz * k.co_t;
            if (best_cost < 0 || cost < best_cost) {
                best_cost = cost;
                best.variant = v;
                best.tw = k.tw;
                best.tiles_x = (int)tx;
                best.tiles_y = (int)ty;
                best.gy = (int)gy;
                best.gz = (int)gz;
            }
        }
    }
    best.items = n * best.tiles_x * best.tiles_y;
    // every split gets the same number of items
    // resident workgroups per CU: the 3x3 kernels 1 (x2 rounds), the others ~3
    int splits = (256 * (ksize == 3 && best.variant != kWgSmallCin ? 2 : 3)) / (best.gy * best.gz);
    if (splits < 1) splits = 1;
    if (splits > best.items) splits = best.items;
    best.items_per_split = (best.items + splits - 1) / splits;
    best.splits = (best.items + best.items_per_split - 1) / best.items_per_split;
    return best;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// proj_bwd_kernel: Cin 32 or 64 with Cout = 2 Cin (its instantiations), whole items, 32-bit byte offsets within
// an image, a 32-bit item count
struct ProjPlan {
    int cib, items_per_image, items, splits, items_per_split;
};
inline bool proj_bwd_shape(int n, int cin, int h, int wd, int cout) {
    if (n <= 0 || cin <= 0 || cout <= 0 || h <= 0 || wd <= 0) return false;
    if (cin % 32 != 0 || cout % 32 != 0 || (long long)cin * cout > 8192) return false;
    if ((cin != 32 && cin != 64) || cout != 2 * cin) return false;
    const long long hw = (long long)h * wd;
    return hw % kProjP == 0 && cout * hw < (1ll << 30) && n * (hw / kProjP) < (1ll << 31);
}
inline ProjPlan plan_proj_bwd(int n, int cin, int h, int wd) {
    ProjPlan pl;
    pl.cib = cin / 32;
    pl.items_per_image = h * wd / kProjP;
    pl.items = n * pl.items_per_image;
    // two waves per SIMD are resident (the kernel's register budget): 8 waves per CU
    const int resident = 256 * 8 / (2 * pl.cib);
    const int splits = resident < pl.items ? resident : pl.items;
    pl.items_per_split = (pl.items + splits - 1) / splits;
    pl.splits = (pl.items + pl.items_per_split - 1) / pl.items_per_split;
    return pl;
}

// Images per workgroup strip: 2 when the 28x8 tile would leave the last tile of every image
// half empty (H = 28: 3.5 tiles) and the shape meets what the strip path needs (full-width
// vector tiles, Cin a whole number of K-chunks, two images within 32-bit byte offsets).
inline int conv_stack(int variant, int n, int cin, int h, int wd, int cout) {
    const FwdVariant& v = kFwdVariants[variant];
    if (variant != 4 || n < 2 || v.th > h) return 1;
    if (h % v.th == 0 || (2 * h) % v.th != 0) return 1;
    if (wd % v.tw != 0 || wd % 4 != 0 || cout % 4 != 0 || cin % 8 != 0) return 1;
    if ((size_t)2 * cin * h * wd >= (1ull << 29) || (size_t)2 * cout * h * wd >= (1ull << 30)) return 1;
    return 2;
}

}  // namespace

void lf::reduce_slabs(float* part, float* dst, size_t count, int splits, float beta, hipStream_t s) {
    const unsigned gx = lf::stream_grid(count, kThreads, 1024);
    if (slab_stages(splits) == 1) {
        slab_reduce_kernel<<<dim3(gx, 1), kThreads, 0, s>>>(part, dst, count, splits, splits, beta, 1);
    } else {
        const int groups = slab_groups(splits);
        float* stage = part + (size_t)splits * count;
        slab_reduce_kernel<<<dim3(gx, groups), kThreads, 0, s>>>(part, stage, count, splits, kSlabGroup, 0.f, 0);
        slab_reduce_kernel<<<dim3(gx, 1), kThreads, 0, s>>>(stage, dst, count, groups, groups, beta, 1);
    }
}

extern "C" {

int lf_conv2d_wgrad_bn_supported(int n, int cin, int h, int wd, int cout, int ksize);

int lf_conv2d_variant(int h, int wd, int cout, int ksize) {
    int best = 0;
    long long bw = -1;
    for (int v = 0; v < kNumFwd; ++v) {
        const long long c = padded_work(kFwdVariants[v], h, wd, cout);
        // 1x1 convolutions are bandwidth-bound: among equally padded tilings take the widest
        // cout tile, so that the input tile is read once instead of once per cout tile
        const bool better = bw < 0 || c < bw ||
                            (ksize == 1 && c == bw && kFwdVariants[v].ct > kFwdVariants[best].ct);
        if (better) {
            bw = c;
            best = v;
        }
    }
    return best;
}

int lf_conv2d_wgrad_variant(int n, int cin, int h, int wd, int cout, int ksize) {
    if (n <= 0 || cin <= 0 || cout <= 0 || h <= 0 || wd <= 0) return -1;
    return plan_wgrad(n, cin, cout, h, wd, ksize).variant;
}

int lf_conv2d_plan(int n, int cin, int h, int wd, int cout, int ksize, int* out) {
    LF_REQUIRE(out, "lf_conv2d_plan: null out");
    LF_REQUIRE(n > 0 && cin > 0 && cout > 0 && h > 0 && wd > 0 && (ksize == 1 || ksize == 3),
               "lf_conv2d_plan: bad dims");
    const int best = lf_conv2d_variant(h, wd, cout, ksize);
    out[0] = best;
    out[1] = fwd_small_cin(ksize * ksize, best, cin) ? 1 : 0;
    out[2] = conv_stack(best, n, cin, h, wd, cout);
    out[3] = fwd_vec_shape(wd, cout) ? 1 : 0;
    return LF_OK;
}

int lf_conv2d_wgrad_plan(int n, int cin, int h, int wd, int cout, int ksize, int* out) {
    LF_REQUIRE(out, "lf_conv2d_wgrad_plan: null out");
    LF_REQUIRE(n > 0 && cin > 0 && cout > 0 && h > 0 && wd > 0 && (ksize == 1 || ksize == 3),
               "lf_conv2d_wgrad_plan: bad dims");
    const WgPlan pl = plan_wgrad(n, cin, cout, h, wd, ksize);
    out[0] = pl.variant;
    out[1] = pl.items_per_split < 3 ? pl.items_per_split : 3;   // 1, 2, or 3+: the steady-state prefetch
    out[2] = lf::slab_stages(pl.splits);
    out[3] = lf_conv2d_wgrad_bn_supported(n, cin, h, wd, cout, ksize);
    return LF_OK;
}

// every 3x3 launch but the stem's runs conv_wino_kernel, which reads the prepared U instead of w
static inline bool fwd_takes_wino_filters(int cin, int h, int wd, int cout, int ksize) {
    return ksize == 3 && !fwd_small_cin(9, lf_conv2d_variant(h, wd, cout, ksize), cin);
}

static int conv2d_launch(const char* who, const float* x, const float* w, const float* wino_u, float* y, int n, int cin,
                         int h, int wd, int cout, int ksize, const float* in_scale,
                         const float* in_shift, int in_relu, int accumulate, float* stat_part,
                         const float* stat_pivot, const float* stat_mask_y, const float* mask_scale,
                         const float* mask_shift, int mask_relu, lf_stream_t stream) {
    LF_REQUIRE(x && y, "%s: null buffer", who);
    LF_REQUIRE(n > 0 && cin > 0 && cout > 0 && h > 0 && wd > 0,
               "%s: bad dims n=%d cin=%d cout=%d h=%d w=%d", who, n, cin, cout, h, wd);
    LF_REQUIRE(ksize == 3 || ksize == 1, "%s: ksize must be 1 or 3 (got %d)", who, ksize);
    LF_REQUIRE((in_scale == nullptr) == (in_shift == nullptr),
               "%s: in_scale/in_shift must both be set", who);
    LF_REQUIRE(n <= 65535, "%s: batch too large for grid.z", who);
    LF_REQUIRE((size_t)cin * h * wd < (1ull << 30) && (size_t)cin * ksize * ksize * cout < (1ull << 30),
               "%s: per-image tensor too large for 32-bit offsets", who);
    const int best = lf_conv2d_variant(h, wd, cout, ksize);
    const FwdVariant& v = kFwdVariants[best];
    const bool wino = fwd_takes_wino_filters(cin, h, wd, cout, ksize);
    if (wino) {
        // no in-kernel transform to fall back to: w is not read and may be null
        LF_REQUIRE(wino_u, "%s: this 3x3 convolution runs in the Winograd domain and needs wino_u "
                   "(lf_conv2d_wino_filters_f32)", who);
        LF_REQUIRE(aligned16(wino_u), "%s: wino_u must be 16-byte aligned", who);
        LF_REQUIRE((size_t)cin * cout * 16 < (1ull << 30) && cout <= (1 << 20), "%s: wino_u too large for 32-bit offsets", who);
    } else {
        LF_REQUIRE(w, "%s: null buffer", who);
    }
    ConvArgs a;
    a.x = x; a.w = w; a.y = y;
    a.wino_u = wino ? wino_u : nullptr;
    a.in_scale = in_scale; a.in_shift = in_shift;
    a.n = n; a.cin = cin; a.cout = cout; a.h = h; a.wd = wd;
    a.in_relu = in_relu;
    a.accumulate = accumulate;
    a.vec_ok = fwd_vec_shape(wd, cout) && aligned16(x) && aligned16(wino ? nullptr : w);
    a.stack = conv_stack(best, n, cin, h, wd, cout);
    if (a.stack > 1 && !a.vec_ok) {
        if (stat_part != nullptr) {  // the tile count the caller sized its buffers for assumes it
            lf::set_error("%s: the statistics epilogue needs 16-byte aligned x / w", who);
            return LF_ERR_INVALID;
        }
        a.stack = 1;
    }
    a.tiles_x = (wd + v.tw - 1) / v.tw;
    a.tiles_y = (a.stack * h + v.th - 1) / v.th;
    a.stat_part = stat_part;
    a.stat_pivot = stat_pivot;
    a.stat_mask_y = stat_mask_y; a.mask_scale = mask_scale; a.mask_shift = mask_shift;
    a.mask_relu = mask_relu;
    const int gz = (n + a.stack - 1) / a.stack;
    a.stat_tiles = (long long)gz * a.tiles_x * a.tiles_y;
    const int rc = launch_fwd(ksize, best, a, a.tiles_x * a.tiles_y, gz, lf::as_stream(stream));
    if (rc != LF_OK) return rc;
    return lf::check_launch(who);
}

int lf_conv2d_f32(const float* x, const float* w, float* y, int n, int cin, int h, int wd, int cout,
                  int ksize, const float* in_scale, const float* in_shift, int in_relu,
                  int accumulate, lf_stream_t stream, const float* wino_u) {
    return conv2d_launch("lf_conv2d", x, w, wino_u, y, n, cin, h, wd, cout, ksize, in_scale, in_shift, in_relu,
                         accumulate, nullptr, nullptr, nullptr, nullptr, nullptr, 0, stream);
}

long long lf_conv2d_stats_tiles(int n, int cin, int h, int wd, int cout, int ksize) {
    if (n <= 0 || cin <= 0 || h <= 0 || wd <= 0 || cout <= 0) return 0;
    const int best = lf_conv2d_variant(h, wd, cout, ksize);
    const FwdVariant& v = kFwdVariants[best];
    const int stack = conv_stack(best, n, cin, h, wd, cout);
    return (long long)((n + stack - 1) / stack) * ((wd + v.tw - 1) / v.tw) * ((stack * h + v.th - 1) / v.th);
}

// the per-tile sums of a statistics epilogue: [lf_conv2d_stats_tiles][cout][2] floats
static int check_tile_part(const char* who, size_t tile_part_bytes, int n, int cin, int h, int wd, int cout, int ksize) {
    const long long tiles = lf_conv2d_stats_tiles(n, cin, h, wd, cout, ksize);
    if (tile_part_bytes >= (size_t)tiles * (size_t)(cout > 0 ? cout : 0) * 2 * sizeof(float)) return LF_OK;
    lf::set_error("%s: tile_part %zu bytes < %lld tiles x %d channels x 8", who, tile_part_bytes, tiles, cout);
    return LF_ERR_WORKSPACE;
}

int lf_conv2d_stats_f32(const float* x, const float* w, float* y, int n, int cin, int h, int wd,
                        int cout, int ksize, const float* in_scale, const float* in_shift,
                        int in_relu, const float* pivot, float* tile_part, size_t tile_part_bytes,
                        lf_stream_t stream, const float* wino_u) {
    LF_REQUIRE(tile_part, "lf_conv2d_stats: null tile_part");
    if (const int rc = check_tile_part("lf_conv2d_stats", tile_part_bytes, n, cin, h, wd, cout, ksize)) return rc;
    return conv2d_launch("lf_conv2d_stats", x, w, wino_u, y, n, cin, h, wd, cout, ksize, in_scale, in_shift,
                         in_relu, 0, tile_part, pivot, nullptr, nullptr, nullptr, 0, stream);
}

int lf_conv2d_bnbwd_f32(const float* x, const float* w, float* y, int n, int cin, int h, int wd,
                        int cout, int ksize, int accumulate, const float* mask_y,
                        const float* mask_scale, const float* mask_shift, int mask_relu,
                        float* tile_part, size_t tile_part_bytes, lf_stream_t stream, const float* wino_u) {
    LF_REQUIRE(tile_part && mask_y && mask_scale && mask_shift, "lf_conv2d_bnbwd: null buffer");
    if (const int rc = check_tile_part("lf_conv2d_bnbwd", tile_part_bytes, n, cin, h, wd, cout, ksize)) return rc;
    return conv2d_launch("lf_conv2d_bnbwd", x, w, wino_u, y, n, cin, h, wd, cout, ksize, nullptr, nullptr, 0,
                         accumulate, tile_part, nullptr, mask_y, mask_scale, mask_shift, mask_relu,
                         stream);
}

int lf_conv2d_dgrad_weights_f32(const float* w, float* wt, int cin, int ksize, int cout,
                                lf_stream_t stream) {
    LF_REQUIRE(w && wt, "lf_conv2d_dgrad_weights: null buffer");
    LF_REQUIRE(cin > 0 && cout > 0 && (ksize == 1 || ksize == 3), "lf_conv2d_dgrad_weights: bad dims");
    const int total = cin * ksize * ksize * cout;
    weight_dgrad_kernel<<<lf::stream_grid(total, kThreads), kThreads, 0, lf::as_stream(stream)>>>(
        w, wt, cin, ksize * ksize, cout);
    return lf::check_launch("lf_conv2d_dgrad_weights");
}

int lf_conv2d_takes_wino_filters(int cin, int h, int wd, int cout, int ksize) {
    if (cin <= 0 || cout <= 0 || h <= 0 || wd <= 0) return 0;
    return fwd_takes_wino_filters(cin, h, wd, cout, ksize) ? 1 : 0;
}

int lf_conv2d_wino_filters_f32(const float* w, float* u, int cin, int cout, int dgrad, lf_stream_t stream) {
    LF_REQUIRE(w && u, "lf_conv2d_wino_filters: null buffer");
    LF_REQUIRE(cin > 0 && cout > 0 && (size_t)cin * cout * 16 < (1ull << 30), "lf_conv2d_wino_filters: bad dims");
    LF_REQUIRE(aligned16(u), "lf_conv2d_wino_filters: u must be 16-byte aligned");
    wino_filters_kernel<<<lf::stream_grid((size_t)cin * cout, kThreads), kThreads, 0, lf::as_stream(stream)>>>(
        w, u, cin, cout, dgrad ? 1 : 0);
    return lf::check_launch("lf_conv2d_wino_filters");
}

size_t lf_conv2d_wgrad_workspace(int n, int cin, int h, int wd, int cout, int ksize) {
    if (n <= 0 || cin <= 0 || cout <= 0 || h <= 0 || wd <= 0) return 0;
    const WgPlan pl = plan_wgrad(n, cin, cout, h, wd, ksize);
    const size_t count = (size_t)cin * ksize * ksize * cout;
    return ((size_t)pl.splits + lf::slab_groups(pl.splits)) * count * sizeof(float);
}

static int wgrad_launch(const char* who, const float* x, const float* dy, int n, int cin, int h,
                        int wd, int cout, int ksize, const float* in_scale, const float* in_shift,
                        int in_relu, const float* bn_y, const float* bn_alpha, const float* bn_add,
                        const float* bn_coef, int bn_relu, float* dy_out, void* workspace,
                        size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(x && dy && workspace, "%s: null buffer", who);
    LF_REQUIRE(n > 0 && cin > 0 && cout > 0 && h > 0 && wd > 0,
               "%s: bad dims n=%d cin=%d cout=%d h=%d w=%d", who, n, cin, cout, h, wd);
    LF_REQUIRE(ksize == 3 || ksize == 1, "%s: ksize must be 1 or 3 (got %d)", who, ksize);
    LF_REQUIRE((in_scale == nullptr) == (in_shift == nullptr),
               "%s: in_scale/in_shift must both be set", who);
    LF_REQUIRE((size_t)cin * h * wd < (1ull << 30) && (size_t)cout * h * wd < (1ull << 30),
               "%s: per-image tensor too large for 32-bit offsets", who);
    const WgPlan pl = plan_wgrad(n, cin, cout, h, wd, ksize);
    if (ws_bytes < lf_conv2d_wgrad_workspace(n, cin, h, wd, cout, ksize)) {
        lf::set_error("%s: workspace %zu < %zu bytes", who, ws_bytes,
                      lf_conv2d_wgrad_workspace(n, cin, h, wd, cout, ksize));
        return LF_ERR_WORKSPACE;
    }
    WgradArgs a;
    a.x = x; a.dy = dy; a.part = static_cast<float*>(workspace);
    a.in_scale = in_scale; a.in_shift = in_shift;
    a.n = n; a.cin = cin; a.cout = cout; a.h = h; a.wd = wd;
    a.tiles_x = pl.tiles_x; a.tiles_y = pl.tiles_y; a.items = pl.items;
    a.items_per_split = pl.items_per_split;
    a.in_relu = in_relu;
    a.vec_ok = (wd % pl.tw == 0) && (wd % 4 == 0) && aligned16(x) && aligned16(dy);
    a.bn_y = bn_y; a.bn_alpha = bn_alpha; a.bn_add = bn_add; a.bn_coef = bn_coef;
    a.dy_out = dy_out; a.bn_relu = bn_relu;
    if (bn_y != nullptr) {
        LF_REQUIRE(bn_coef, "%s: bn_coef missing", who);
        LF_REQUIRE(bn_add == nullptr || bn_alpha != nullptr, "%s: bn_add needs bn_alpha", who);
        LF_REQUIRE(lf_conv2d_wgrad_bn_supported(n, cin, h, wd, cout, ksize) && a.vec_ok &&
                       aligned16(bn_y) && (dy_out == nullptr || aligned16(dy_out)),
                   "%s: shape/alignment not supported by the fused BatchNorm-backward path "
                   "(ask lf_conv2d_wgrad_bn_supported first)", who);
    }
    dim3 grid(pl.splits, pl.gy, pl.gz);
    hipStream_t s = lf::as_stream(stream);
    int rc = LF_OK;
    if (pl.variant == kWgSmallCin)
        wgrad_smallcin_kernel<32, 8><<<grid, kThreads, 0, s>>>(a);
    else
        rc = launch_wgrad(ksize, pl.variant, a, grid, s);
    if (rc != LF_OK) return rc;
    return lf::check_launch(who);
}

int lf_conv2d_wgrad_f32(const float* x, const float* dy, int n, int cin, int h, int wd, int cout,
                        int ksize, const float* in_scale, const float* in_shift, int in_relu,
                        void* workspace, size_t ws_bytes, lf_stream_t stream) {
    return wgrad_launch("lf_conv2d_wgrad", x, dy, n, cin, h, wd, cout, ksize, in_scale, in_shift,
                        in_relu, nullptr, nullptr, nullptr, nullptr, 0, nullptr, workspace, ws_bytes,
                        stream);
}

int lf_conv2d_wgrad_bn_supported(int n, int cin, int h, int wd, int cout, int ksize) {
    if (n <= 0 || cin <= 0 || cout <= 0 || h <= 0 || wd <= 0 || (ksize != 3 && ksize != 1)) return 0;
    const WgPlan pl = plan_wgrad(n, cin, cout, h, wd, ksize);
    return (wd % pl.tw == 0) && (wd % 4 == 0);
}

int lf_conv2d_wgrad_bn_f32(const float* x, const float* g, const float* bn_y,
                           const float* alpha_nc, const float* add_nc, const float* coef,
                           int bn_relu, float* dy_out, int n, int cin, int h, int wd, int cout,
                           int ksize, const float* in_scale, const float* in_shift, int in_relu,
                           void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(bn_y, "lf_conv2d_wgrad_bn: null bn_y");
    return wgrad_launch("lf_conv2d_wgrad_bn", x, g, n, cin, h, wd, cout, ksize, in_scale, in_shift,
                        in_relu, bn_y, alpha_nc, add_nc, coef, bn_relu, dy_out, workspace, ws_bytes,
                        stream);
}

int lf_conv2d_wgrad_reduce_f32(void* workspace, float* dw, int n, int cin, int h, int wd, int cout,
                               int ksize, float beta, lf_stream_t stream) {
    LF_REQUIRE(workspace && dw, "lf_conv2d_wgrad_reduce: null buffer");
    LF_REQUIRE(n > 0 && cin > 0 && cout > 0 && h > 0 && wd > 0 && (ksize == 1 || ksize == 3),
               "lf_conv2d_wgrad_reduce: bad dims");
    const WgPlan pl = plan_wgrad(n, cin, cout, h, wd, ksize);
    const size_t count = (size_t)cin * ksize * ksize * cout;
    lf::reduce_slabs(static_cast<float*>(workspace), dw, count, pl.splits, beta, lf::as_stream(stream));
    return lf::check_launch("lf_conv2d_wgrad_reduce");
}

int lf_conv2d_proj_bwd_supported(const float* x, const float* g, const float* bn_y, const float* w,
                                 const float* dx, int n, int cin, int h, int wd, int cout) {
    if (!x || !g || !bn_y || !w || !dx) return 0;
    if (!aligned16(x) || !aligned16(g) || !aligned16(bn_y) || !aligned16(w) || !aligned16(dx)) return 0;
    return proj_bwd_shape(n, cin, h, wd, cout) ? 1 : 0;
}

int lf_conv2d_proj_bwd_plan(int n, int cin, int h, int wd, int cout, int* out) {
    LF_REQUIRE(out, "lf_conv2d_proj_bwd_plan: null out");
    LF_REQUIRE(proj_bwd_shape(n, cin, h, wd, cout), "lf_conv2d_proj_bwd_plan: unsupported shape");
    const ProjPlan pl = plan_proj_bwd(n, cin, h, wd);
    out[0] = kProjP;
    out[1] = pl.items_per_split < 3 ? pl.items_per_split : 3;  // 1, 2, or 3+: how far the prefetch runs
    out[2] = lf::slab_stages(pl.splits);
    return LF_OK;
}

size_t lf_conv2d_proj_bwd_workspace(int n, int cin, int h, int wd, int cout) {
    if (!proj_bwd_shape(n, cin, h, wd, cout)) return 0;
    const ProjPlan pl = plan_proj_bwd(n, cin, h, wd);
    return ((size_t)pl.splits + lf::slab_groups(pl.splits)) * cin * cout * sizeof(float);
}

int lf_conv2d_proj_bwd_f32(const float* x, const float* g, const float* bn_y, const float* coef, int bn_relu,
                           const float* w, float* dx, float* dw, int n, int cin, int h, int wd, int cout,
                           void* workspace, size_t ws_bytes, lf_stream_t stream) {
    const char* who = "lf_conv2d_proj_bwd";
    LF_REQUIRE(x && g && bn_y && coef && w && dx && dw && workspace, "%s: null buffer", who);
    LF_REQUIRE(lf_conv2d_proj_bwd_supported(x, g, bn_y, w, dx, n, cin, h, wd, cout),
               "%s: shape/alignment not supported (ask lf_conv2d_proj_bwd_supported first)", who);
    if (ws_bytes < lf_conv2d_proj_bwd_workspace(n, cin, h, wd, cout)) {
        lf::set_error("%s: workspace %zu < %zu bytes", who, ws_bytes,
                      lf_conv2d_proj_bwd_workspace(n, cin, h, wd, cout));
        return LF_ERR_WORKSPACE;
    }
    const ProjPlan pl = plan_proj_bwd(n, cin, h, wd);
    ProjBwdArgs a;
    a.x = x; a.g = g; a.bn_y = bn_y; a.coef = coef; a.w = w; a.dx = dx;
    a.part = static_cast<float*>(workspace);
    a.hw = h * wd; a.items_per_image = pl.items_per_image; a.items = pl.items;
    a.items_per_split = pl.items_per_split;
    a.bn_relu = bn_relu;
    hipStream_t s = lf::as_stream(stream);
    if (pl.cib == 1)
        proj_bwd_kernel<1><<<pl.splits, 128, 0, s>>>(a);
    else
        proj_bwd_kernel<2><<<pl.splits, 256, 0, s>>>(a);
    if (const int rc = lf::check_launch(who)) return rc;
    lf::reduce_slabs(a.part, dw, (size_t)cin * cout, pl.splits, 0.f, s);
    return lf::check_launch(who);
}

}  // extern "C"
