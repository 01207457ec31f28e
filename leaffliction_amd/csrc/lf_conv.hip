// libleafhip — conv2d forward / dgrad as implicit GEMM on the fp32 MFMA
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
// The weight gradients and the projection shortcut's backward live in lf_wgrad.hip, a translation unit of their own:
// this file is built without the superword-level vectoriser (see the Makefile), which suits conv_wino_kernel and
// costs those kernels their packed f32 arithmetic.  What both files use is in lf_conv_f32.h.
#include <type_traits>

#include "lf_conv_f32.h"

namespace {

using namespace lf::conv_f32;

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

extern "C" {

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

}  // extern "C"
