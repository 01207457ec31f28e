// libleafhip — conv2d weight gradients as implicit GEMM on the fp32 MFMA (v_mfma_f32_32x32x2_f32: exact f32,
// bitwise an fmaf chain), and the backward of a projection shortcut.  Layouts as in lf_conv.hip: activations NCHW
// f32, conv weights "IKO" = [Cin][kh*kw][Cout]; stride 1, "same" zero padding.
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
//
// Built with the common flags only: unlike lf_conv.hip this file keeps the superword-level vectoriser, whose packed
// f32 instructions these kernels' staging and epilogues gain from (profiles/r10_a_wgrad_build.md).
#include <type_traits>

#include "lf_conv_f32.h"

namespace {

using namespace lf::conv_f32;
using lf::bn_dy1;
using lf::pro_apply;

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

// ---- staging rules the kernels below share.  None holds a barrier or a wait of its own except fold_ksplit, whose
// rounds are barriers; all take the kernel's own pointers, so where a kernel loads and stores stays in the kernel.

// Work item -> image n, tile t of the image, and the tile's origin, for TW x TH tiles
struct TileItem {
    int n, t, tx0, ty0;
};
template <int TW, int TH>
__device__ __forceinline__ TileItem tile_item(int item, int tiles, int tiles_x) {
    TileItem it;
    it.n = item / tiles;
    it.t = item - it.n * tiles;
    it.tx0 = (it.t % tiles_x) * TW;
    it.ty0 = (it.t / tiles_x) * TH;
    return it;
}

// Flat staging index e -> the float4 it stands for in a block of channels x ROWS rows x TW4 float4s: channel c, row
// py, float4 `slot` of the row; rem = the float4's index inside the channel plane
struct Slot4 {
    int c, py, slot, rem;
};
template <int ROWS, int TW4>
__device__ __forceinline__ Slot4 slot4(int e) {
    Slot4 s;
    s.c = e / (ROWS * TW4);
    s.rem = e - s.c * (ROWS * TW4);
    s.py = s.rem / TW4;
    s.slot = s.rem - s.py * TW4;
    return s;
}

// The producer BatchNorm's scale / shift of channels ci0 .. ci0 + ci_t - 1 -> lsc[c] / lsc[kMaxProC / 4 + c], neutral
// (1, 0) beyond cin
__device__ __forceinline__ void stage_pro_consts(float* lsc, const float* scale, const float* shift, int ci0, int ci_t,
                                                 int cin, int tid, int threads) {
    for (int c = tid; c < ci_t; c += threads) {
        const int gc = ci0 + c;
        lsc[c] = gc < cin ? scale[gc] : 1.f;
        lsc[kMaxProC / 4 + c] = gc < cin ? shift[gc] : 0.f;
    }
}
__device__ __forceinline__ float4 pro_apply4(float4 v, const float* lsc, int c, int relu) {
    const float sc = lsc[c], sh = lsc[kMaxProC / 4 + c];
    return make_float4(pro_apply(v.x, sc, sh, relu), pro_apply(v.y, sc, sh, relu), pro_apply(v.z, sc, sh, relu),
                       pro_apply(v.w, sc, sh, relu));
}

// The BatchNorm-backward coefficients coef[5][cout] of channels co0 .. co0 + CO_T - 1 -> lbn[5][CO_T], zero beyond
// cout.  WHOLE: the block is the tensor (co0 = 0, cout = CO_T), copied without bounds.
template <int CO_T, bool WHOLE = false>
__device__ __forceinline__ void stage_bn_coef(float* lbn, const float* coef, int co0, int cout, int tid, int threads) {
    for (int e = tid; e < 5 * CO_T; e += threads) {
        if (WHOLE) {
            lbn[e] = coef[e];
        } else {
            const int kk = e / CO_T, gc = co0 + (e - kk * CO_T);
            lbn[e] = gc < cout ? coef[(size_t)kk * cout + gc] : 0.f;
        }
    }
}
// bn_dy1 on the four lanes of a float4 of channel c of the staged block
template <int CO_T>
__device__ __forceinline__ float4 bn_dy4(float4 g, float4 y, float al, float ad, const float* lbn, int c, int relu) {
    const float c0 = lbn[c], c1 = lbn[CO_T + c], c2 = lbn[2 * CO_T + c], c3 = lbn[3 * CO_T + c], c4 = lbn[4 * CO_T + c];
    return make_float4(bn_dy1(g.x, y.x, al, ad, c0, c1, c2, c3, c4, relu), bn_dy1(g.y, y.y, al, ad, c0, c1, c2, c3, c4, relu),
                       bn_dy1(g.z, y.z, al, ad, c0, c1, c2, c3, c4, relu), bn_dy1(g.w, y.w, al, ad, c0, c1, c2, c3, c4, relu));
}
// dy_out is written by the workgroups of ci-block 0 alone: each element exactly once
__device__ __forceinline__ bool writes_dy_out(const float* dy_out, int ci_block) {
    return ci_block == 0 && dy_out != nullptr;
}

// A float4 into LDS planes of odd pitch: no 16-byte alignment, four scalar stores
__device__ __forceinline__ void lds_put4(float* dst, float4 v) {
    dst[0] = v.x;
    dst[1] = v.y;
    dst[2] = v.z;
    dst[3] = v.w;
}

// Scalar (ragged-shape) staging by all `threads` threads, any W and alignment.
// The haloed X patch of a TW x TH tile at (tx0, ty0): `nch` planes of (TW + 2) x (TH + 2) at pitch `pitch`, zero
// outside the image and for channels ci0 + c >= cin, through the producer's prologue (scale null: none).
template <int TW, int TH>
__device__ __forceinline__ void stage_x_patch_scalar(float* lx, int pitch, int nch, const float* xin, int ci0, int cin,
                                                     int tx0, int ty0, int h, int wd, unsigned uhw, const float* scale,
                                                     const float* shift, int relu, int tid, int threads) {
    constexpr int PW = TW + 2, PH = TH + 2;
    for (int e = tid; e < nch * PW * PH; e += threads) {
        const int c = e / (PW * PH), rem = e - c * (PW * PH);
        const int py = rem / PW, px = rem - py * PW;
        const int gc = ci0 + c, gy = ty0 + py - 1, gx = tx0 + px - 1;
        float v = 0.f;
        if (gc < cin && gy >= 0 && gy < h && gx >= 0 && gx < wd) {
            v = xin[(unsigned)gc * uhw + (unsigned)gy * (unsigned)wd + (unsigned)gx];
            if (scale != nullptr) v = pro_apply(v, scale[gc], shift[gc], relu);
        }
        lx[c * pitch + rem] = v;
    }
}
// The dY tile: `nch` planes of TW x TH at pitch `pitch`, zero outside the image and for channels co0 + c >= cout.
template <int TW, int TH>
__device__ __forceinline__ void stage_dy_tile_scalar(float* ld, int pitch, int nch, const float* din, int co0, int cout,
                                                     int tx0, int ty0, int h, int wd, unsigned uhw, int tid,
                                                     int threads) {
    for (int e = tid; e < nch * TW * TH; e += threads) {
        const int c = e / (TW * TH), rem = e - c * (TW * TH);
        const int py = rem / TW, px = rem - py * TW;
        const int gc = co0 + c, gy = ty0 + py, gx = tx0 + px;
        float v = 0.f;
        if (gc < cout && gy < h && gx < wd) v = din[(unsigned)gc * uhw + (unsigned)gy * (unsigned)wd + (unsigned)gx];
        ld[c * pitch + rem] = v;
    }
}

// Row of the 32x32 result that accumulator register r of a v_mfma_f32_32x32x2_f32 holds in lane half khalf (its
// column is lane & 31)
__device__ __forceinline__ constexpr int mfma32_row(int r, int khalf) { return (r & 3) + 8 * (r >> 2) + 4 * khalf; }

// K-split fold: the waves w_k = 1 .. KSPL - 1 add their A accumulators into wave w_k = 0 of the same (ci, co) block q
// (of NQ) through LDS, one writer and one reader per round, in a fixed order (deterministic); accumulator a, register
// r goes through slab[a * 1024 + r * 64 + lane].  Every wave of the workgroup calls it: the rounds are barriers.
template <int A, int KSPL, int NQ>
__device__ __forceinline__ void fold_ksplit(f32x16* acc, float* slab, int w_k, int q, int lane) {
#pragma unroll 1
    for (int k = 1; k < KSPL; ++k) {
#pragma unroll 1
        for (int qq = 0; qq < NQ; ++qq) {
            __syncthreads();
            if (w_k == k && q == qq) {
#pragma unroll
                for (int a = 0; a < A; ++a)
#pragma unroll
                    for (int r = 0; r < 16; ++r) slab[a * 1024 + r * 64 + lane] = acc[a][r];
            }
            __syncthreads();
            if (w_k == 0 && q == qq) {
#pragma unroll
                for (int a = 0; a < A; ++a)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[a][r] += slab[a * 1024 + r * 64 + lane];
            }
        }
    }
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
        if (pro) stage_pro_consts(lsc, p.in_scale, p.in_shift, ci0, CI_T, p.cin, tid, kThreads);
        // optional: dY = BatchNorm backward of p.dy, formed while staging (see WgradArgs)
        const bool bn = p.bn_y != nullptr;
        float4 yv[DPT];
        float dal[DPT], dad[DPT];
        unsigned dok = 0;
        __shared__ float lbn[5 * CO_T];
        if (bn) stage_bn_coef<CO_T>(lbn, p.bn_coef, co0, p.cout, tid, kThreads);
        // the next item's loads stay in registers over the MFMAs
        auto load_x = [&](int item) {
            const TileItem it = tile_item<TW, TH>(item, tiles, p.tiles_x);
            const float* xin = p.x + (size_t)it.n * p.cin * hw;
            xok = 0;
#pragma unroll
            for (int i = 0; i < XPT; ++i) {
                const int e = tid + i * kThreads;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                const Slot4 s = slot4<TH, TW4>(e);
                const int gc = ci0 + s.c, gy = it.ty0 + s.py;
                if (e < NXI && gc < p.cin && gy < p.h) {
                    v = *reinterpret_cast<const float4*>(xin + (unsigned)gc * uhw +
                                                         (unsigned)gy * (unsigned)p.wd + it.tx0 + 4 * s.slot);
                    xok |= 1u << i;
                }
                xv[i] = v;
            }
        };
        auto load_d = [&](int item) {
            const TileItem it = tile_item<TW, TH>(item, tiles, p.tiles_x);
            const int n = it.n;
            const float* din = p.dy + (size_t)n * p.cout * hw;
            dok = 0;
#pragma unroll
            for (int i = 0; i < DPT; ++i) {
                const int e = tid + i * kThreads;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                const Slot4 s = slot4<TH, TW4>(e);
                const int gc = co0 + s.c, gy = it.ty0 + s.py;
                if (e < NDI && gc < p.cout && gy < p.h) {
                    v = *reinterpret_cast<const float4*>(din + (unsigned)gc * uhw +
                                                         (unsigned)gy * (unsigned)p.wd + it.tx0 + 4 * s.slot);
                    dok |= 1u << i;
                }
                dv[i] = v;
            }
            if (bn) {
                const float* yin = p.bn_y + (size_t)n * p.cout * hw;
#pragma unroll
                for (int i = 0; i < DPT; ++i) {
                    const Slot4 s = slot4<TH, TW4>(tid + i * kThreads);
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (dok >> i & 1u)
                        v = *reinterpret_cast<const float4*>(yin + (unsigned)(co0 + s.c) * uhw +
                                                             (unsigned)(it.ty0 + s.py) * (unsigned)p.wd + it.tx0 +
                                                             4 * s.slot);
                    yv[i] = v;
                }
#pragma unroll
                for (int i = 0; i < DPT; ++i) {
                    const int gc = min(co0 + slot4<TH, TW4>(tid + i * kThreads).c, p.cout - 1);
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
                    const Slot4 s = slot4<TH, TW4>(e);
                    float4 v = xv[i];
                    if (pro && (xok >> i & 1u)) v = pro_apply4(v, lsc, s.c, p.in_relu);
                    lds_put4(lx + s.c * PP + s.py * TW + 4 * s.slot, v);
                }
            }
        };
        auto store_d = [&](int item) {
            const TileItem it = tile_item<TW, TH>(item, tiles, p.tiles_x);
#pragma unroll
            for (int i = 0; i < DPT; ++i) {
                const int e = tid + i * kThreads;
                if (e < NDI) {
                    const Slot4 s = slot4<TH, TW4>(e);
                    float4 v = dv[i];
                    if (bn && (dok >> i & 1u)) {
                        v = bn_dy4<CO_T>(v, yv[i], dal[i], dad[i], lbn, s.c, p.bn_relu);
                        if (writes_dy_out(p.dy_out, blk.y))
                            *reinterpret_cast<float4*>(p.dy_out + ((size_t)it.n * p.cout + co0 + s.c) * hw +
                                                       (size_t)(it.ty0 + s.py) * p.wd + it.tx0 + 4 * s.slot) = v;
                    }
                    lds_put4(ld + s.c * PP + s.rem * 4, v);
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
            const TileItem it = tile_item<TW, TH>(item, tiles, p.tiles_x);
            const float* xin = p.x + (size_t)it.n * p.cin * hw;
            const float* din = p.dy + (size_t)it.n * p.cout * hw;
            __syncthreads();
            if (slot < POS) {
                const int gy = it.ty0 + spy, gx = it.tx0 + spx;
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
    fold_ksplit<1, KSPL, WCI * WCO>(&acc, lds, w_k, w_co * WCI + w_ci, lane);
    if (w_k == 0) {
        float* out = p.part + (size_t)blk.x * p.cin * p.cout;
        const int co = co0 + w_co * 32 + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = ci0 + w_ci * 32 + mfma32_row(r, khalf);
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

// Work item -> image n and the item's first pixel px0 of the flat plane
struct ProjItem {
    int n;
    size_t px0;
};
__device__ __forceinline__ ProjItem proj_item(int item, int items_per_image) {
    ProjItem it;
    it.n = item / items_per_image;
    it.px0 = (size_t)(item - it.n * items_per_image) * kProjP;
    return it;
}

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

    stage_bn_coef<COUT, true>(lbn, p.coef, 0, COUT, tid, NT);
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
        const ProjItem it = proj_item(item, p.items_per_image);
        const __amdgpu_buffer_rsrc_t rx = buf_rsrc(p.x + (size_t)it.n * CIN * p.hw + it.px0, xbytes);
        const __amdgpu_buffer_rsrc_t rg = buf_rsrc(p.g + (size_t)it.n * COUT * p.hw + it.px0, dbytes);
        const __amdgpu_buffer_rsrc_t ry = buf_rsrc(p.bn_y + (size_t)it.n * COUT * p.hw + it.px0, dbytes);
#pragma unroll
        for (int i = 0; i < XPT; ++i) xv[i] = buf_load4(rx, goff + (unsigned)i * gstep);
#pragma unroll
        for (int i = 0; i < DPT; ++i) gv[i] = buf_load4(rg, goff + (unsigned)i * gstep);
#pragma unroll
        for (int i = 0; i < DPT; ++i) yv[i] = buf_load4(ry, goff + (unsigned)i * gstep);
    };
    auto store_item = [&]() {
#pragma unroll
        for (int i = 0; i < XPT; ++i) lds_put4(lx + loff + i * CSTEP * PP, xv[i]);
#pragma unroll
        for (int i = 0; i < DPT; ++i)
            lds_put4(ld + loff + i * CSTEP * PP,
                     bn_dy4<COUT>(gv[i], yv[i], 1.f, 0.f, lbn, c0 + i * CSTEP, p.bn_relu));
    };
    auto compute_item = [&](int item) {
        // input gradient of the item: K = co, this lane half's run of HC channels
        f32x16 accx;
#pragma unroll
        for (int r = 0; r < 16; ++r) accx[r] = 0.f;
        const float* bx = ld + khalf * HC * PP + pxb * 32 + j;
#pragma unroll
        for (int s = 0; s < HC; ++s) accx = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[s], bx[s * PP], accx, 0, 0, 0);
        const ProjItem it = proj_item(item, p.items_per_image);
        const __amdgpu_buffer_rsrc_t rdx = buf_rsrc(p.dx + (size_t)it.n * CIN * p.hw + it.px0, xbytes);
#pragma unroll
        for (int r = 0; r < 16; ++r)  // the lane half's four rows are in soff
            buf_store1(rdx, soff + 4u * (unsigned)mfma32_row(r, 0) * uhw, accx[r]);
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
            out[(a * 32 + mfma32_row(r, khalf)) * COUT + wid * 32 + j] = accw[a][r];
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

// TAB: the launch passes per-image alpha / add (bn_alpha, with bn_y), kept in the LDS table `lal`.  The launches
// without them run an instantiation that carries none of it: in one kernel the table's uniform state cost them more
// spilled SGPRs in the item loop than it saved the others (profiles/r10_a_wgrad_build.md).
template <int TW, int TH, int WCI, int WCO, int KSPL, bool TAB>
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
        // With four float4 of dY per thread (CO_T = 64 over a 128-pixel tile) a whole prefetched dY tile (dv and yv:
        // 32 registers) does not fit beside the 128 accumulators.  Those variants hold half of the
        // thread's slots at a time: slots [0, DH) are the tile's first CO_T / 2 channels, [DH, DPT) the others.
        // (The per-image alpha / add are not among them: they sit in an LDS table, `lal` below.)
        constexpr bool kSplitD = DPT > 2;
        static_assert(!kSplitD || DPT == 4, "the dY tile is prefetched whole or in two halves");
        constexpr int DH = kSplitD ? DPT / 2 : DPT;  // dY slots a thread holds in registers
        float4 xv[XPT], dv[DH], yv[DH];
        float xh[HPT];
        unsigned xok = 0, dok = 0;
        const bool bn = p.bn_y != nullptr;
        // producer BatchNorm scale/shift of this workgroup's CI_T channels, staged once in LDS
        __shared__ float lsc[kMaxProC / 2];
        // (stage_pro_consts and stage_bn_coef written out: through the helpers <16,8,1,2,2> spilled 7 and 10 more SGPRs)
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
        // The optional per-image alpha / add of the workgroup's CO_T channels: they change only when an item's image
        // does, so they live in an LDS table with one slot per image parity, lal[n & 1] = {alpha[CO_T], add[CO_T]}
        // (an item is stored while the one before it is read, so two images can be live).  The prologue fills item
        // 0's slot.  When item k + 1 opens a new image, load_item(k) asks for that image's entries behind half 0 of
        // item k's dY (threads below CO_T; the other threads' offsets are out of range and fetch nothing)
        // and store_item(k) writes them to the other slot a stage point later, behind its last wait.  They are read
        // by store_item(k + 1) during the next item: the barrier that ends item k - 1 stands between, the readers
        // before it read item k's slot, and the slot's earlier image was last read during item k - 2.
        __shared__ float lal[2][2 * CO_T];
        constexpr bool tabbed = TAB;  // the launcher instantiates TAB for the launches that pass bn_alpha
        const unsigned tbytes = 4u * (unsigned)min(CO_T, p.cout - co0);
        const unsigned tg = tid < CO_T ? 4u * (unsigned)tid : kBufOob;  // the thread's table entry
        float tal = 0.f, tad = 0.f;  // a refill in flight
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
            const Slot4 s = slot4<PH, TW4>(e);
            const bool ok = e < NXI && ci0 + s.c < p.cin;
            xg[i] = ok ? 4u * ((unsigned)s.c * uhw + (unsigned)s.py * (unsigned)p.wd + 1u + 4u * (unsigned)s.slot)
                       : kBufOob;
            xl[i] = (unsigned)(s.c * PP + s.py * PW + 1 + 4 * s.slot) | ((unsigned)s.py << 16);
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
            const Slot4 s = slot4<TH, TW4>(e);
            const bool ok = e < NDI && co0 + s.c < p.cout;
            dg[i] = ok ? 4u * ((unsigned)s.c * uhw + (unsigned)s.py * (unsigned)p.wd + 4u * (unsigned)s.slot) : kBufOob;
            dl[i] = (unsigned)(s.c * DP + s.rem * 4) | ((unsigned)s.py << 16);
        }
        const unsigned xbytes = 4u * ((unsigned)min(CI_T, p.cin - ci0) * uhw + (unsigned)p.wd + 1u);
        const unsigned dbytes = 4u * (unsigned)min(CO_T, p.cout - co0) * uhw;
        // Issue the loads of an item's X patch (with_x) and / or of half `dhalf` of its dY tile (-1: no dY; a
        // variant that holds the whole tile has only half 0).  Nothing here is conditional: where `live` is false
        // (there is no such item) every load takes the out-of-range offset, which fetches zeros and no memory.
        auto load_item = [&](int item, bool with_x, int dhalf, bool live) {
            const TileItem it = tile_item<TW, TH>(item, tiles, p.tiles_x);
            const int n = it.n, t = it.t, tx0 = it.tx0, ty0 = it.ty0;
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
                // the next item's alpha / add if it opens a new image: the newest loads of the item, on a uniform
                // branch, so the waits for the loads above are counted as they are without it
                if (dhalf == 0 && tabbed && live && t + 1 == tiles && item + 1 < last) {
                    const size_t row = (size_t)(n + 1) * p.cout + co0;
                    const bool add = p.bn_add != nullptr;
                    tal = buf_load1(buf_rsrc(p.bn_alpha + row, tbytes), tg);
                    tad = buf_load1(buf_rsrc(add ? p.bn_add + row : p.bn_alpha, add ? tbytes : 0u), tg);
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
                    float4 v = xv[i];  // padding was fetched as zeros
                    if (pro && (xok >> i & 1u)) v = pro_apply4(v, lsc, slot4<PH, TW4>(tid + i * NT).c, p.in_relu);
                    lds_put4(lx + (xl[i] & 0xffffu), v);
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
            const TileItem it = tile_item<TW, TH>(item, tiles, p.tiles_x);
            const int sn = it.n;
            float* dyo = bn ? p.dy_out + ((size_t)sn * p.cout + co0) * hw + (size_t)it.ty0 * p.wd + it.tx0 : nullptr;
            const float* tb = lal[sn & 1];
#pragma unroll
            for (int i = 0; i < DH; ++i) {
                if (tid + (s0 + i) * NT < NDI) {
                    const int c = slot4<TH, TW4>(tid + (s0 + i) * NT).c;
                    float4 v = dv[i];
                    if (bn && (dok >> i & 1u)) {
                        const float al = tabbed ? tb[c] : 1.f, ad = tabbed ? tb[CO_T + c] : 0.f;
                        v = bn_dy4<CO_T>(v, yv[i], al, ad, lbn, c, p.bn_relu);
                        if (writes_dy_out(p.dy_out, blk.y)) *reinterpret_cast<float4*>(dyo + (dg[s0 + i] >> 2)) = v;
                    }
                    lds_put4(ld + (dl[s0 + i] & 0xffffu), v);
                }
            }
            // the next item's image, asked for by load_item(item): the newest of its loads, so this wait is the last
            if (tabbed && dhalf == 0 && it.t + 1 == tiles && item + 1 < last && tid < CO_T) {
                lal[(sn + 1) & 1][tid] = tal;
                lal[(sn + 1) & 1][CO_T + tid] = tad;
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
            if (tabbed && tid < CO_T && co0 + tid < p.cout) {  // item 0's slot, before the first barrier
                const int n0 = first / tiles;
                const size_t r0 = (size_t)n0 * p.cout + co0 + tid;
                lal[n0 & 1][tid] = p.bn_alpha[r0];
                lal[n0 & 1][CO_T + tid] = p.bn_add != nullptr ? p.bn_add[r0] : 0.f;
            }
            __syncthreads();  // lsc / lbn / lal are staged
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
            const TileItem it = tile_item<TW, TH>(item, tiles, p.tiles_x);
            __syncthreads();
            stage_x_patch_scalar<TW, TH>(lx, PP, CI_T, p.x + (size_t)it.n * p.cin * hw, ci0, p.cin, it.tx0, it.ty0, p.h,
                                         p.wd, uhw, p.in_scale, p.in_shift, p.in_relu, tid, NT);
            stage_dy_tile_scalar<TW, TH>(ld, DP, CO_T, p.dy + (size_t)it.n * p.cout * hw, co0, p.cout, it.tx0, it.ty0,
                                         p.h, p.wd, uhw, tid, NT);
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
    fold_ksplit<8, KSPL, NQ>(acc, lds + pg * 8 * 1024, w_k, q, lane);

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
                const int ci = ci0 + w_ci * 32 + mfma32_row(r, khalf);
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
    const bool bn = p.bn_y != nullptr;  // dY = BatchNorm backward of p.dy, formed while staging
    __shared__ float lbn[5 * 32];
    if (bn) stage_bn_coef<32>(lbn, p.bn_coef, co0, p.cout, tid, kThreads);
    constexpr int ROWS = TH / 4;
    for (int item = first; item < last; ++item) {
        const TileItem it = tile_item<TW, TH>(item, tiles, p.tiles_x);
        const int n = it.n;
        const float* din = p.dy + (size_t)n * p.cout * hw;
        __syncthreads();
        stage_x_patch_scalar<TW, TH>(lx, PP, p.cin, p.x + (size_t)n * p.cin * hw, 0, p.cin, it.tx0, it.ty0, p.h, p.wd,
                                     uhw, p.in_scale, p.in_shift, p.in_relu, tid, kThreads);
        if (p.vec_ok) {
#pragma unroll
            for (int i = 0; i < 32 * TH * TW4 / kThreads; ++i) {
                const Slot4 s = slot4<TH, TW4>(tid + i * kThreads);
                const int gc = co0 + s.c, gy = it.ty0 + s.py;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gc < p.cout && gy < p.h) {
                    const size_t off = (size_t)gc * uhw + (size_t)gy * p.wd + it.tx0 + 4 * s.slot;
                    v = *reinterpret_cast<const float4*>(din + off);
                    if (bn) {
                        const float4 yv = *reinterpret_cast<const float4*>(
                            p.bn_y + (size_t)n * p.cout * hw + off);
                        const float al = p.bn_alpha ? p.bn_alpha[(size_t)n * p.cout + gc] : 1.f;
                        const float ad = p.bn_add ? p.bn_add[(size_t)n * p.cout + gc] : 0.f;
                        v = bn_dy4<32>(v, yv, al, ad, lbn, s.c, p.bn_relu);
                        if (writes_dy_out(p.dy_out, blockIdx.y))
                            *reinterpret_cast<float4*>(p.dy_out + (size_t)n * p.cout * hw + off) = v;
                    }
                }
                lds_put4(ld + s.c * DP + s.rem * 4, v);
            }
        } else {
            stage_dy_tile_scalar<TW, TH>(ld, DP, 32, din, co0, p.cout, it.tx0, it.ty0, p.h, p.wd, uhw, tid, kThreads);
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
    // the 4 row-split waves fold as a K-split of one (ci, co) block
    fold_ksplit<1, 4, 1>(&acc, lds, wid, 0, lane);
    if (wid == 0) {
        float* out = p.part + (size_t)blockIdx.x * p.cin * 9 * p.cout;
        const int co = co0 + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kidx = mfma32_row(r, khalf);  // = ci*9 + tap
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

// The tile variants, stated once: plan_wgrad's cost loop and both dispatches (launch_wgrad) walk this table.  A
// variant's id is its index (bench.py labels kernels by it): it runs wgrad3_kernel (3x3) or wgrad_mfma_kernel (1x1) as
// <tw, th, ci_t / 32, co_t / 32, kspl>.
struct WgVariant {
    int tw, th, ci_t, co_t, kspl;
};
constexpr WgVariant kWgVariants[] = {{32, 4, 32, 32, 4}, {16, 8, 32, 64, 2}, {16, 4, 64, 64, 1},
                                     {28, 2, 64, 64, 1}};
constexpr int kNumWgVariants = (int)(sizeof(kWgVariants) / sizeof(kWgVariants[0]));
// wgrad_smallcin_kernel: its tile (4 waves split the rows; the (ci, tap) pairs are the one 32-row ci block) and its
// variant id (4 is not used)
constexpr WgVariant kWgSmallCinTile = {32, 8, 32, 32, 4};
constexpr int kWgSmallCin = 5;

// wgrad3 uses more than the 64 KB of LDS a kernel gets by default: raise the limit once
// TAB: the launch passes per-image alpha / add (the kernel's LDS table)
template <int TW, int TH, int WCI, int WCO, int KSPL, bool TAB>
int launch_wgrad3_tab(const WgradArgs& a, dim3 grid, hipStream_t s) {
    constexpr size_t bytes = (size_t)wgrad3_lds_floats<TW, TH, WCI, WCO, KSPL>() * sizeof(float);
    static bool raised = false;
    if (!raised) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad3_kernel<TW, TH, WCI, WCO, KSPL, TAB>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
            lf::set_error("lf_conv2d_wgrad: cannot reserve %zu bytes of LDS", bytes);
            return LF_ERR_LAUNCH;
        }
        raised = true;
    }
    wgrad3_kernel<TW, TH, WCI, WCO, KSPL, TAB><<<grid, 64 * 2 * WCI * WCO * KSPL, bytes, s>>>(a);
    return LF_OK;
}
template <int TW, int TH, int WCI, int WCO, int KSPL>
int launch_wgrad3(const WgradArgs& a, dim3 grid, hipStream_t s) {
    if (a.bn_y != nullptr && a.bn_alpha != nullptr && a.vec_ok)
        return launch_wgrad3_tab<TW, TH, WCI, WCO, KSPL, true>(a, grid, s);
    return launch_wgrad3_tab<TW, TH, WCI, WCO, KSPL, false>(a, grid, s);
}

// Variant `variant` of the KS x KS kernel: a compile-time walk over kWgVariants, one instantiation per entry
template <int KS, int V = 0>
int launch_wgrad(int variant, const WgradArgs& a, dim3 grid, hipStream_t s) {
    if constexpr (V == kNumWgVariants) {
        return LF_ERR_INVALID;
    } else {
        if (variant != V) return launch_wgrad<KS, V + 1>(variant, a, grid, s);
        constexpr WgVariant k = kWgVariants[V];
        if constexpr (KS == 3) {
            return launch_wgrad3<k.tw, k.th, k.ci_t / 32, k.co_t / 32, k.kspl>(a, grid, s);
        } else {
            wgrad_mfma_kernel<k.tw, k.th, k.ci_t / 32, k.co_t / 32, k.kspl><<<grid, kThreads, 0, s>>>(a);
            return LF_OK;
        }
    }
}

struct WgPlan {
    int variant, tw, tiles_x, tiles_y, items, splits, items_per_split, gy, gz;
};

// Variant v (tile k) on a shape: its tiles and channel blocks, and what plan_wgrad minimises, the work padded to them
long long tile_shape(WgPlan& pl, int v, const WgVariant& k, int cin, int cout, int h, int w) {
    pl.variant = v;
    pl.tw = k.tw;
    pl.tiles_x = (w + k.tw - 1) / k.tw;
    pl.tiles_y = (h + k.th - 1) / k.th;
    pl.gy = (cin + k.ci_t - 1) / k.ci_t;
    pl.gz = (cout + k.co_t - 1) / k.co_t;
    return (long long)pl.tiles_x * k.tw * pl.tiles_y * k.th * pl.gy * k.ci_t * pl.gz * k.co_t;
}

WgPlan plan_wgrad(int n, int cin, int cout, int h, int w, int ksize) {
    WgPlan best{};
    if (ksize == 3 && cin * 9 <= 32) {
        tile_shape(best, kWgSmallCin, kWgSmallCinTile, cin, cout, h, w);
    } else {
        long long best_cost = -1;
        for (int v = 0; v < kNumWgVariants; ++v) {
            WgPlan cand{};
            const long long cost = tile_shape(cand, v, kWgVariants[v], cin, cout, h, w);
            if (best_cost < 0 || cost < best_cost) {
                best_cost = cost;
                best = cand;
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

// the "workspace too small" answer of the entries that take one
int require_workspace(const char* who, size_t have, size_t need) {
    if (have >= need) return LF_OK;
    lf::set_error("%s: workspace %zu < %zu bytes", who, have, need);
    return LF_ERR_WORKSPACE;
}

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

int lf_conv2d_wgrad_variant(int n, int cin, int h, int wd, int cout, int ksize) {
    if (n <= 0 || cin <= 0 || cout <= 0 || h <= 0 || wd <= 0) return -1;
    return plan_wgrad(n, cin, cout, h, wd, ksize).variant;
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
    if (const int rc = require_workspace(who, ws_bytes, lf_conv2d_wgrad_workspace(n, cin, h, wd, cout, ksize)))
        return rc;
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
        wgrad_smallcin_kernel<kWgSmallCinTile.tw, kWgSmallCinTile.th><<<grid, kThreads, 0, s>>>(a);
    else
        rc = ksize == 3 ? launch_wgrad<3>(pl.variant, a, grid, s) : launch_wgrad<1>(pl.variant, a, grid, s);
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
    if (const int rc = require_workspace(who, ws_bytes, lf_conv2d_proj_bwd_workspace(n, cin, h, wd, cout))) return rc;
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
