// libleafhip — streaming bf16 convolution for the layers that dominate the mixed-precision
// training step: the 224x224 and 112x112 stages, where Cin and Cout are at most 64 and the
// tensors are 0.8 - 1.6 GB per batch.  With bf16 storage these convolutions are HBM-bound (72
// FLOP per byte at 32->32 against a ridge of ~310), so the kernel is organised around the
// memory stream, not around the MFMA:
//
//   * the whole filter bank (<= 36 KB of bf16) is copied into LDS ONCE per workgroup and stays
//     there;
//   * a workgroup walks DOWN a column strip of an image (TW pixels wide), tile after tile, and the
//     patch in LDS is a RING of TH + 2 pixel rows: a tile brings in only its TH new rows, the two
//     rows it shares with the tile above are still there (round 3; before, every tile staged its
//     own TH + 2 rows and the input crossed the fabric 1.5x for the halo rows alone — PMC,
//     profiles/pmc_latest_bf16.json of round 2: 2.59 GB per forward launch against 1.64 GB).  The
//     strips of one image go to neighbouring workgroups of one XCD, which walk them at the same
//     pace: the halo columns and the 128-byte lines two strips share are found in that XCD's L2;
//   * the NEW rows of the next tile are in flight in registers while the current tile's MFMAs
//     and epilogue run (all input channels at once: no K-chunk loop, no barrier per chunk);
//   * the patch sits in LDS as [pixel][channel] rows (64 B per pixel at 32 channels) with the
//     16-byte channel groups XOR-swizzled by the pixel index: the B operand of a lane (one pixel,
//     eight consecutive channels) is ONE aligned ds_read_b128 whatever the tap offset, and the
//     A operand (one output channel, eight input channels of one tap) is one ds_read_b128 of the
//     resident weights — 3 LDS reads per 2 MFMAs;
//   * the producer's BatchNorm+ReLU is applied in fp32 while staging (the f32 -> bf16 packing
//     pairs channels of a pixel, which is the transposition);
//   * BatchNorm statistics / BatchNorm-backward sums of the rounded output are accumulated per
//     lane across ALL tiles of the workgroup and reduced once at the end: one partial per
//     workgroup instead of one per tile.
//
// Every global access is 16 bytes per lane: the vector memory pipe moves ~5.3 TB/s with 16-byte
// lanes but only ~3 TB/s with 8-byte and ~1.5 TB/s with 4-byte lanes
// (scripts/microbench/seg_bw.hip, profiles/r02_microbench_seg_bw.txt).  The MFMA leaves a lane with
// ONE pixel column of 16 channels (D[row = output channel][col = pixel]), i.e. 2-byte pieces; the
// accumulators therefore go through LDS once (fp32, [channel][pixel]) and come back as eight
// consecutive pixels of one channel per lane: 16-byte stores, 16-byte loads of the read-modify-
// write operands (old value when accumulating, the BatchNorm input for the backward sums — both
// requested BEFORE the MFMAs), and the statistics of a channel live in one half-wave.
// Replaces Conv2D forward and its input-gradient (srcs/model/cnn.py:27-29 under the mixed_float16
// policy of train.py:179-190).
//
// Launched by conv_bf16_launch (lf_conv_bf16.hip) for the shapes bf16_route sends here: lf_conv2d_bf16_train for every
// shape plan_s covers, the inference entries for the 16- and 32-channel layers.
//
// A 16-channel output block (C16: the 16-wide stage of the tiny preset, and the input gradients that flow back
// into it) runs the same 32x32x16 MFMA: rows 16-31 of the A operand repeat rows 0-15, the rows of D they produce
// (accumulator registers 8-15) are never looked at, and the epilogue is the first of a 32-channel block's two
// passes.  Nothing of a channel >= 16 is stored, loaded or summed.  These layers wait for memory, not for the
// MFMA pipe, which a 32->32 layer already keeps only about a fifth busy.
#include "lf_common.h"

namespace {

constexpr int kT = 256;

using lf::bf16_down;
using lf::bf16_up;
using lf::bf16x8;
using lf::f32x16;
using lf::u32x2;
using lf::pack_bf16;

template <int TAPS, int CI, int NCO, int TW, int TH, bool C16 = false>
struct SShape {
    static constexpr int HALO = TAPS == 9 ? 1 : 0;
    static constexpr int PW = TW + 2 * HALO, PH = TH + 2 * HALO, PPIX = PW * PH;
    static constexpr int ROWB = CI * 2;                     // bytes per pixel row of the patch image
    static constexpr int R = 256 / ROWB, C = ROWB / 16;    // rows per 256-byte bank window, 16-byte groups per row
    static constexpr int COUT = C16 ? 16 : 32 * NCO, CH = CI / 16;
    static constexpr int NJ = C16 ? 2 : 4;                  // rows of 8 channels to an output block
    static constexpr int WBYTES = CH * TAPS * 2 * COUT * 16;
    static constexpr int PBYTES = (PPIX * ROWB + 15) / 16 * 16;
    // The epilogue's transpose buffer: fp32 accumulators of HALF a 32-channel block (16 channels x 256 pixels), a
    // quarter of it private to each wave.  It has LDS of its own: with the row ring the patch is never dead (the
    // rows the next tile keeps would be overwritten), and a wave may write its accumulators while slower waves are
    // still reading the patch — no barrier in front of the epilogue.
    static constexpr int EBYTES = 16 * 256 * 4;
    static constexpr int LDS = WBYTES + PBYTES + EBYTES;
};

// RMW = false: a launch with no read-modify-write operand (no accumulate, no BatchNorm-backward mask): the
// 32 registers those operands wait in are free, which is what lets three workgroups share a CU (12 waves at
// <= 168 registers) where the filter bank and the patch are small enough.
template <int TAPS, int CI, int NCO, int TW, int TH, bool XBF, bool RMW, bool C16 = false>
__global__ __launch_bounds__(kT, (SShape<TAPS, CI, NCO, TW, TH, C16>::LDS <= 52 * 1024 && !RMW)
                                     ? 3 : (SShape<TAPS, CI, NCO, TW, TH, C16>::LDS <= 80 * 1024 ? 2 : 1))
void conv_bf16s_kernel(lf::ConvBf16Args p) {
    using S = SShape<TAPS, CI, NCO, TW, TH, C16>;
    static_assert(!C16 || NCO == 1, "a 16-channel output block is half of ONE 32-row MFMA block");
    static_assert(TW * TH == 256 && TW % 8 == 0, "tile = 4 waves x 64 pixels, whole 8-pixel groups");
    static_assert(XBF || CI == 16, "fp32 input: the stem only (3 channels padded to one 16-channel group)");
    constexpr int HALO = S::HALO, PW = S::PW, PH = S::PH, ROWB = S::ROWB, COUT = S::COUT, CH = S::CH, NJ = S::NJ;
    constexpr int G = XBF ? 8 : 4;           // pixels per staging unit: 16 bytes of bf16 / of fp32
    constexpr int PGS = TW / G, NB = 2;
    typedef unsigned uvec __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned char* lw = lds;
    unsigned char* lp = lds + S::WBYTES;
    float* le = reinterpret_cast<float*>(lp + S::PBYTES);  // [16 channels][256 pixels]
    __shared__ float lsc[2 * CI];
    __shared__ float lst[2 * COUT];
    __shared__ float los[2 * COUT];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, px = lane & 31, kh = lane >> 5;
    const size_t hw = (size_t)p.h * p.w;
    const bool pro = p.in_scale != nullptr;
    const bool stats = p.stat_part != nullptr || p.unit_sums != nullptr, masked = RMW && p.stat_mask_y != nullptr;
    const bool accumulate = RMW && p.accumulate;
    // What a workgroup walks: SEGMENTS of column strips (a strip = TW columns of one image; a segment = seg_tiles
    // consecutive tiles of it, top to bottom — whole strips when the launch has enough of them to fill the chip).
    // interleave = 1: image i belongs to XCD i % 8 (workgroups k, k+8, ... run on XCD k), whose workgroups take that
    // XCD's segments in order — the strips of one image by NEIGHBOURING workgroups, started together —, so what two
    // strips share (halo columns, 128-byte lines that straddle a strip boundary) crosses the fabric once.
    // interleave = 0 (small launches): segments dealt round-robin over the grid.
    const lf::StripWalk walk(p.n, p.tiles_x, p.tiles_y, p.seg_tiles, p.segs, p.interleave);

    // ---- one-time: filter bank -> LDS as [chunk][tap][k half][cout][8 channels] (16 B per entry)
    {
        constexpr int NW = CH * TAPS * COUT * 2;
        for (int e = tid; e < NW; e += kT) {
            const int h2 = e & 1, co = (e >> 1) % COUT, ct = (e >> 1) / COUT;  // ct = chunk * TAPS + tap
            const lf::u32x4 v = *reinterpret_cast<const lf::u32x4*>(p.wprep + ((size_t)ct * p.cout + co) * 16 + 8 * h2);
            *reinterpret_cast<lf::u32x4*>(lw + ((ct * 2 + h2) * COUT + co) * 16) = v;
        }
        if (pro)
            for (int c = tid; c < CI; c += kT) {
                lsc[c] = c < p.cin ? p.in_scale[c] : 1.f;
                lsc[CI + c] = c < p.cin ? p.in_shift[c] : 0.f;
            }
        for (int c = tid; c < COUT; c += kT) {  // per-channel epilogue constants: pivot | mask scale, mask shift
            lst[c] = masked ? p.mask_scale[c] : ((stats && p.stat_pivot != nullptr) ? p.stat_pivot[c] : 0.f);
            lst[COUT + c] = masked ? p.mask_shift[c] : 0.f;
            los[c] = p.out_scale != nullptr ? p.out_scale[c] : 1.f;
            los[COUT + c] = p.out_scale != nullptr ? p.out_shift[c] : 0.f;
        }
        if (!XBF)  // channels 4..15 of the stem's rows are never written by the staging: zero them once
            for (int e = tid; e < S::PBYTES / 16; e += kT)
                *reinterpret_cast<lf::u32x4*>(lp + 16 * e) = lf::u32x4{0u, 0u, 0u, 0u};
    }

    auto poff = [&](unsigned pp, unsigned c16) -> unsigned {  // byte offset of 16-byte group c16 of patch pixel pp
        return pp * ROWB + ((c16 ^ ((pp / S::R) % S::C)) << 4);
    };

    // ---- staging units: 4 channels x G pixels (interior: one 16-byte load per channel), 4 channels x 1
    // pixel (halo columns).  One staging pass covers up to TH image rows gy0 .. gy0 + nrows - 1 of the strip; row gy
    // lives in ring slot (gy + HALO) mod PH.
    constexpr int QD = XBF ? CI / 4 : 1;  // channel quads that carry data
    constexpr int NXU = QD * TH * PGS, XPT = (NXU + kT - 1) / kT;
    constexpr int NHU = QD * TH * 2 * HALO, HPT = (NHU + kT - 1) / kT;
    static_assert(2 * HALO <= TH, "the two rows that prime a strip go through the same staging registers");
    uvec rx[XPT][XBF ? 4 : 3];
    unsigned rh[HPT > 0 ? HPT : 1][XBF ? 4 : 3];   // raw loads: combining them here would wait for them here
    unsigned xmask = 0, hmask = 0;
    int st_slot = 0, st_rows = 0;   // of the pass in flight: ring slot of its first row, its row count

    auto issue = [&](int n, int tx0, int gy0, int nrows) {
        xmask = hmask = 0;
        st_rows = nrows;
        st_slot = (gy0 + HALO) % PH;   // gy0 >= -HALO
        const uint16_t* xb = static_cast<const uint16_t*>(p.x) + (XBF ? (size_t)n * p.cin * hw : 0);
        const float* xf = static_cast<const float*>(p.x) + (XBF ? 0 : (size_t)n * p.cin * hw);
#pragma unroll
        for (int k = 0; k < XPT; ++k) {
            const int u = tid + k * kT;
            const int pg = u % PGS, t1 = u / PGS, quad = t1 % QD, pr = t1 / QD;
            const int gy = gy0 + pr, gx = tx0 + G * pg;
            const bool ok = pr < nrows && gy >= 0 && gy < p.h && gx < p.w && 4 * quad < p.cin;
            xmask |= (ok ? 1u : 0u) << k;
            if (!ok) continue;
            const size_t o = (size_t)(4 * quad) * hw + (size_t)gy * p.w + gx;
            if (XBF) {
#pragma unroll
                for (int i = 0; i < 4; ++i) rx[k][i] = *reinterpret_cast<const uvec*>(xb + o + (size_t)i * hw);
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (i < p.cin) rx[k][i] = *reinterpret_cast<const uvec*>(xf + o + (size_t)i * hw);
            }
        }
#pragma unroll
        for (int k = 0; k < HPT; ++k) {
            const int u = tid + k * kT;
            const int side = u & 1, t1 = u >> 1, quad = t1 % QD, pr = t1 / QD;
            const int gy = gy0 + pr, gx = side ? tx0 + TW : tx0 - 1;
            const bool ok = pr < nrows && gy >= 0 && gy < p.h && gx >= 0 && gx < p.w && 4 * quad < p.cin;
            hmask |= (ok ? 1u : 0u) << k;
            if (!ok) continue;
            const size_t o = (size_t)(4 * quad) * hw + (size_t)gy * p.w + gx;
            if (XBF) {
#pragma unroll
                for (int i = 0; i < 4; ++i) rh[k][i] = xb[o + (size_t)i * hw];
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) rh[k][i] = i < p.cin ? __float_as_uint(xf[o + (size_t)i * hw]) : 0u;
            }
        }
    };

    // the producer's BatchNorm (+ReLU) on the values v of channel c, in fp32
    auto prologue = [&](int c, auto& v) {
        if (!pro) return;
        const float sc = lsc[c], sh = lsc[CI + c];
#pragma unroll
        for (int e = 0; e < (int)(sizeof(v) / sizeof(float)); ++e) v[e] = lf::pro_apply(v[e], sc, sh, p.in_relu);
    };
    auto commit = [&]() {
#pragma unroll
        for (int k = 0; k < XPT; ++k) {
            const int u = tid + k * kT;
            const int pg = u % PGS, t1 = u / PGS, quad = t1 % QD, pr = t1 / QD;
            if (pr >= st_rows) continue;
            const bool ok = xmask >> k & 1u;
            int slot = st_slot + pr;
            slot = slot >= PH ? slot - PH : slot;
            const unsigned pi = (unsigned)(slot * PW + HALO + G * pg);
            auto store = [&](int e, int pair, unsigned dword) {
                *reinterpret_cast<unsigned*>(lp + poff(pi + e, (unsigned)quad >> 1) + 8 * (quad & 1) + 4 * pair) = dword;
            };
            if constexpr (XBF) {
                lf::stage_quad<G>(rx[k], ok, [&](int i, float (&v)[G]) { prologue(4 * quad + i, v); }, store);
            } else {
                // the stem: three fp32 channels and a zero one
                float v[4][G];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int e = 0; e < G; ++e) v[i][e] = 0.f;  // zero padding stays exactly zero
                    if (ok && i < 3 && i < p.cin) {
#pragma unroll
                        for (int e = 0; e < G; ++e) v[i][e] = __uint_as_float(rx[k][i < 3 ? i : 0][e]);
                        prologue(i, v[i]);
                    }
                }
#pragma unroll
                for (int e = 0; e < G; ++e) {
                    store(e, 0, pack_bf16(v[0][e], v[1][e]));
                    store(e, 1, pack_bf16(v[2][e], v[3][e]));
                }
            }
        }
#pragma unroll
        for (int k = 0; k < HPT; ++k) {
            const int u = tid + k * kT;
            const int side = u & 1, t1 = u >> 1, quad = t1 % QD, pr = t1 / QD;
            if (pr >= st_rows) continue;
            // (the stem: three fp32 channels, the fourth stays zero)
            const u32x2 o = lf::stage_halo_quad(
                hmask >> k & 1u,
                [&](int i) { return XBF ? bf16_up(rh[k][i]) : (i < 3 ? __uint_as_float(rh[k][i]) : 0.f); },
                [&](int i, float (&v)[1]) { if (XBF || i < 3) prologue(4 * quad + i, v); });
            int slot = st_slot + pr;
            slot = slot >= PH ? slot - PH : slot;
            const unsigned pi = (unsigned)(slot * PW + (side ? PW - 1 : 0));
            *reinterpret_cast<u32x2*>(lp + poff(pi, (unsigned)quad >> 1) + 8 * (quad & 1)) = o;
        }
    };

    // MFMA geometry: the wave owns 64 consecutive flat tile positions; lane px holds positions 2*px
    // (block 0) and 2*px + 1 (block 1): the same row, adjacent columns
    const int f0 = 64 * wv + 2 * px;
    const int prow = f0 / TW, pcol = f0 - prow * TW;
    // epilogue geometry: thread = (pixel group eg of 8 consecutive flat positions, channel ec + 8*j), the groups
    // of a wave being the 64 positions whose accumulators the wave itself holds: what a wave reads back from `le`
    // it has written itself, so the transposition needs no workgroup barrier
    const int eg = 8 * wv + (lane & 7), ec = lane >> 3;
    const int erow = (8 * eg) / TW, ecol = (8 * eg) - erow * TW;

    f32x16 acc[NB][NCO];
    float s1[NCO][NJ], s2[NCO][NJ];  // running sums of this thread's channels over all its pixels and tiles
#pragma unroll
    for (int cb = 0; cb < NCO; ++cb)
#pragma unroll
        for (int j = 0; j < NJ; ++j) s1[cb][j] = s2[cb][j] = 0.f;
    uvec rold[NCO][NJ], rmask[NCO][NJ];  // eight pixels of one channel each, as stored

    // A tile's new rows are gy = ty * TH + HALO .. + TH - 1; a segment's first tile also needs the 2 * HALO rows above
    // them (the "prime" pass: staged when the segment starts, its latency exposed once per segment).  (The first
    // rows of a unit are issued in two places, written out: behind a lambda of their own the 1x1 variants, which
    // sit at 168 registers, spilled two.)
    if (walk.units > 0) {
        const lf::StripUnit u = walk.unit(0);
        issue(u.n, u.strip * TW, u.t_first * TH + HALO, TH);
    }
    for (int ui = 0; ui < walk.units; ++ui) {
    const lf::StripUnit un = walk.unit(ui);
    const int n = un.n, tx0 = un.strip * TW, t_first = un.t_first, t_count = un.t_count;
    for (int tt = 0; tt < t_count; ++tt) {
        __syncthreads();  // the previous tile's operand reads are done (first pass: weights / lsc / lst staged)
        const int ty0 = (t_first + tt) * TH;
        commit();
        if (HALO > 0 && tt == 0) {
            issue(n, tx0, ty0 - HALO, 2 * HALO);
            commit();
        }
        // the next tile's new rows: in flight during the MFMAs and the epilogue
        if (tt + 1 < t_count) {
            issue(n, tx0, ty0 + TH + HALO, TH);
        } else if (ui + 1 < walk.units) {
            const lf::StripUnit u = walk.unit(ui + 1);
            issue(u.n, u.strip * TW, u.t_first * TH + HALO, TH);
        }
        // the epilogue's read-modify-write operands: requested now, consumed after the MFMAs
        uint16_t* yb = static_cast<uint16_t*>(p.y) + (size_t)n * p.cout * hw;
        const int gy = ty0 + erow, gx = tx0 + ecol;
        const bool ok = gy < p.h && gx < p.w;  // the 8-pixel group is inside or outside as a whole (w % 8 == 0)
        const size_t po = ok ? (size_t)gy * p.w + gx : 0;
        if (accumulate) lf::row8_request(rold, yb, 0, ec, hw, po);
        if (masked) lf::row8_request(rmask, p.stat_mask_y + (size_t)n * p.cout * hw, 0, ec, hw, po);
        __syncthreads();
        // patch row r of this tile (image row ty0 - HALO + r) sits in ring slot (ty0 + r) mod PH
        unsigned rowpp[TAPS == 9 ? 3 : 1];
        {
            int slot = (ty0 + prow) % PH;
#pragma unroll
            for (int dy = 0; dy < (TAPS == 9 ? 3 : 1); ++dy) {
                rowpp[dy] = (unsigned)(slot * PW + pcol);
                slot = slot + 1 >= PH ? 0 : slot + 1;
            }
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int cb = 0; cb < NCO; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[nb][cb][r] = 0.f;
        // One GROUP = one 16-channel chunk of one filter row: its three taps read four neighbouring patch pixels between
        // them (dx + nb = 0 .. 3), so a group is 4 B reads + 3 A reads (per output block) for 6 MFMAs (per output
        // block) — and all of a group's reads are issued before its first MFMA, so that they are in flight beside the
        // PREVIOUS group's MFMAs (the compiler kept two or three reads in flight, every MFMA behind an operand
        // requested one MFMA earlier).  Measured: 32->32 @224 forward 593-606 -> 582 us, input gradient with accumulate
        // 622-630 -> 606 us (-3 %); the same software pipelining of the weight-gradient kernel's k-steps changed
        // nothing and was not kept.  The order of the contributions to each accumulator — (chunk, filter row, tap) —
        // is unchanged: same bits.
        constexpr int ROWS = TAPS == 9 ? 3 : 1, TPR = TAPS / ROWS, NBP = TPR + NB - 1, NG = CH * ROWS;
        // With one output block per workgroup the registers allow TWO groups' operands: group g + 1 is requested,
        // whole, before group g's MFMAs are issued (scheduling barriers keep the compiler from sinking the reads back
        // to their uses).  Two output blocks (NCO = 2) are at their register budget and keep the compiler's order.
        // (the stem variant runs three workgroups per CU at 168 registers; so does 32 -> 16, which spilled 24 with two
        // groups in flight)
        constexpr bool DEEP = NCO == 1 && CI >= 32 && !C16;
        bf16x8 A[DEEP ? 2 : 1][TPR][NCO], B[DEEP ? 2 : 1][NBP];
        auto fetch = [&](int g, int buf) {
            const int ch = g / ROWS, dy = g - ch * ROWS;
#pragma unroll
            for (int j = 0; j < NBP; ++j)
                B[buf][j] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const lf::u32x4*>(
                    lp + poff(rowpp[dy] + (unsigned)j, (unsigned)(2 * ch + kh))));
#pragma unroll
            for (int dx = 0; dx < TPR; ++dx)
#pragma unroll
                for (int cb = 0; cb < NCO; ++cb)
                    A[buf][dx][cb] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const lf::u32x4*>(
                        lw + ((((ch * TAPS + dy * TPR + dx) * 2 + kh) * COUT) + cb * 32 + (C16 ? px & 15 : px)) * 16));
        };
        if (DEEP) fetch(0, 0);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int buf = DEEP ? (g & 1) : 0;
            if (DEEP) {
                if (g + 1 < NG) fetch(g + 1, buf ^ 1);
                __builtin_amdgcn_sched_barrier(0);
            } else {
                fetch(g, 0);
            }
#pragma unroll
            for (int dx = 0; dx < TPR; ++dx)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int cb = 0; cb < NCO; ++cb)
                        acc[nb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[buf][dx][cb], B[buf][dx + nb],
                                                                              acc[nb][cb], 0, 0, 0);
            if (DEEP) __builtin_amdgcn_sched_barrier(0);
        }
        // ---- epilogue, one 32-channel block at a time through LDS: lane (pixel pair, 16 channels)
        // -> thread (8 pixels, 4 channels); then 16-byte stores and the sums of the rounded values
#pragma unroll
        for (int cb = 0; cb < NCO; ++cb)
#pragma unroll
        for (int hf = 0; hf < NJ / 2; ++hf) {
#pragma unroll
            for (int r = 8 * hf; r < 8 * hf + 8; ++r) {
                const int cl = 8 * ((r >> 2) & 1) + 4 * kh + (r & 3);   // channel within the half block
                *reinterpret_cast<float2*>(le + cl * 256 + 64 * wv + 2 * px) = make_float2(acc[0][cb][r], acc[1][cb][r]);
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's own LDS writes (no other wave reads them)
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 2 * hf; j < 2 * hf + 2; ++j) {
                const int cl = 8 * j + ec, co = cb * 32 + cl;
                const uvec o = lf::row8_finish(le + (cl & 15) * 256 + 8 * eg, accumulate, rold[cb][j],
                                               p.out_scale != nullptr, &los[co], &los[COUT + co], p.out_relu);
                if (ok) *reinterpret_cast<uvec*>(yb + (size_t)co * hw + po) = o;
                if (!stats || !ok) continue;
                float a = 0.f, b = 0.f;
                lf::row8_sums(o, masked, &lst[co], &lst[co], &lst[COUT + co], rmask[cb][j], p.mask_relu, a, b);
                s1[cb][j] += a;
                s2[cb][j] += b;
            }
            __builtin_amdgcn_wave_barrier();   // the reads above stay in front of the next block's writes
        }
    }
    if (p.unit_sums != nullptr) {
        // inference: this segment's channel sums of the stored activation (the squeeze of the block's SE gate adds
        // them up per image).  The patch is dead between segments: the reduction scratch lies over it.
        __syncthreads();
        float* red = reinterpret_cast<float*>(lp);   // [4 waves][COUT]
#pragma unroll
        for (int cb = 0; cb < NCO; ++cb)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float a = s1[cb][j];
#pragma unroll
                for (int m = 1; m < 8; m <<= 1) a += __shfl_xor(a, m, 64);
                if ((lane & 7) == 0) red[wv * COUT + cb * 32 + 8 * j + ec] = a;
                s1[cb][j] = s2[cb][j] = 0.f;
            }
        __syncthreads();
        for (int c = tid; c < COUT; c += kT)
            p.unit_sums[((size_t)n * (p.tiles_x * p.segs) + un.rem) * p.cout + c] =
                (red[c] + red[COUT + c]) + (red[2 * COUT + c] + red[3 * COUT + c]);
    }
    }
    if (p.stat_part != nullptr) {
        // one partial per workgroup: a channel's pixel groups are 8 lanes (lane & 7) in each of the four waves
        __syncthreads();
        float* red = reinterpret_cast<float*>(lp);   // [4 waves][COUT][2], over the patch (dead now)
#pragma unroll
        for (int cb = 0; cb < NCO; ++cb)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                float a = s1[cb][j], b = s2[cb][j];
#pragma unroll
                for (int m = 1; m < 8; m <<= 1) {
                    a += __shfl_xor(a, m, 64);
                    b += __shfl_xor(b, m, 64);
                }
                if ((lane & 7) == 0) {
                    red[(wv * COUT + cb * 32 + 8 * j + ec) * 2] = a;
                    red[(wv * COUT + cb * 32 + 8 * j + ec) * 2 + 1] = b;
                }
            }
        __syncthreads();
        lf::write_stat_part<4, COUT>(p.stat_part, p.stat_tiles, p.cout, blockIdx.x, 0, red, tid, kT);
    }
}

lf::ConvBf16sPlan plan_s(int n, int cin, int h, int w, int cout, int ksize, int x_bf16) {
    lf::ConvBf16sPlan pl{};
    pl.ok = false;
    if (cout != 16 && cout != 32 && cout != 64) return pl;
    if (w % 8 != 0) return pl;                              // 16-byte rows
    pl.xbf = x_bf16 ? 1 : 0;
    pl.c16 = cout == 16 ? 1 : 0;
    if (!x_bf16) {
        if (cin > 3 || ksize != 3 || cout > 32) return pl;
        pl.ci = 16;
    } else {
        if (cin != 16 && cin != 32 && cin != 64) return pl;
        pl.ci = cin;
    }
    pl.nco = pl.c16 ? 1 : cout / 32;
    // The 16-channel blocks that exist are those a 16-wide stage and its neighbours launch, forward and backward:
    // 16 <-> 16 and 16 <-> 32 (1x1: the projection 16 -> 32 and its input gradient 32 -> 16).
    if ((pl.c16 || pl.ci == 16) && x_bf16 && (pl.ci > 32 || cout > 32)) return pl;
    if (ksize == 1 && !(pl.ci == 32 && pl.nco == 2) && !(pl.ci == 64 && pl.nco == 1) &&
        !(pl.ci == 16 && cout == 32) && !(pl.ci == 32 && pl.c16))
        return pl;
    // Rows of a tile are the unit of every global access (64 px = 128 bytes of bf16 per channel row): measured
    // on 32->32 @224, 64x4 tiles against 32x8: forward 687 -> 659 us, input gradient with accumulate + mask +
    // sums 1167 -> 913 us; 64->64 @112 against 16x16: 724 -> 513 and 1043 -> 699 us — although an eighth of
    // the last tile of a 224- or 112-pixel row is empty (scripts/microbench/conv_modes.py).
    if (w >= 64) { pl.tw = 64; pl.th = 4; }
    else if (w % 32 == 0) { pl.tw = 32; pl.th = 8; }
    else { pl.tw = 16; pl.th = 16; }
    pl.tiles_x = (w + pl.tw - 1) / pl.tw;
    pl.tiles_y = (h + pl.th - 1) / pl.th;
    // Column strips are cut into segments only when there are too few of them to fill the chip twice over (small
    // batches): a segment re-stages the two rows above it, so whole strips are what the full-size step gets
    // (batch 256 @224: 1,024 strips of 56 tiles; @112: 512 strips in two segments of 14 tiles).
    const int strips = n * pl.tiles_x;
    lf::strip_segments(strips, 4 * 256, pl.tiles_y, &pl.seg_tiles, &pl.segs);
    const int units = strips * pl.segs;
    pl.wgs = units < 256 * 2 ? units : 256 * 2;
    pl.interleave = (pl.wgs % 8 == 0 && n >= 8) ? 1 : 0;
    pl.ok = true;
    return pl;
}

template <int TAPS, int CI, int NCO, int TW, int TH, bool XBF, bool RMW, bool C16>
int launch_s2(const lf::ConvBf16Args& a, int wgs, hipStream_t s) {
    using S = SShape<TAPS, CI, NCO, TW, TH, C16>;
    static bool raised = false;
    if (!raised) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_bf16s_kernel<TAPS, CI, NCO, TW, TH, XBF, RMW, C16>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, S::LDS) != hipSuccess) {
            lf::set_error("lf_conv2d_bf16_train: cannot reserve %d bytes of LDS", S::LDS);
            return LF_ERR_LAUNCH;
        }
        raised = true;
    }
    conv_bf16s_kernel<TAPS, CI, NCO, TW, TH, XBF, RMW, C16><<<wgs, kT, S::LDS, s>>>(a);
    return LF_OK;
}

template <int TAPS, int CI, int NCO, int TW, int TH, bool XBF, bool C16 = false>
int launch_s(const lf::ConvBf16Args& a, int wgs, hipStream_t s) {
    return lf::conv_bf16s_rmw(a.accumulate, a.stat_mask_y != nullptr)
               ? launch_s2<TAPS, CI, NCO, TW, TH, XBF, true, C16>(a, wgs, s)
               : launch_s2<TAPS, CI, NCO, TW, TH, XBF, false, C16>(a, wgs, s);
}

template <int TW, int TH>
int dispatch_s(const lf::ConvBf16sPlan& pl, int ksize, const lf::ConvBf16Args& a, hipStream_t s) {
    if (!pl.xbf)   // the stem: fp32 input, three channels in one 16-channel group
        return pl.c16 ? launch_s<9, 16, 1, TW, TH, false, true>(a, pl.wgs, s)
                      : launch_s<9, 16, 1, TW, TH, false>(a, pl.wgs, s);
    if (ksize == 3) {
        if (pl.ci == 16 && pl.c16) return launch_s<9, 16, 1, TW, TH, true, true>(a, pl.wgs, s);
        if (pl.ci == 16 && pl.nco == 1) return launch_s<9, 16, 1, TW, TH, true>(a, pl.wgs, s);
        if (pl.ci == 32 && pl.c16) return launch_s<9, 32, 1, TW, TH, true, true>(a, pl.wgs, s);
        if (pl.ci == 32 && pl.nco == 1) return launch_s<9, 32, 1, TW, TH, true>(a, pl.wgs, s);
        if (pl.ci == 32 && pl.nco == 2) return launch_s<9, 32, 2, TW, TH, true>(a, pl.wgs, s);
        if (pl.ci == 64 && pl.nco == 1) return launch_s<9, 64, 1, TW, TH, true>(a, pl.wgs, s);
        if (pl.ci == 64 && pl.nco == 2) return launch_s<9, 64, 2, TW, TH, true>(a, pl.wgs, s);
    } else {
        if (pl.ci == 16 && pl.nco == 1 && !pl.c16) return launch_s<1, 16, 1, TW, TH, true>(a, pl.wgs, s);
        if (pl.ci == 32 && pl.c16) return launch_s<1, 32, 1, TW, TH, true, true>(a, pl.wgs, s);
        if (pl.ci == 32 && pl.nco == 2) return launch_s<1, 32, 2, TW, TH, true>(a, pl.wgs, s);
        if (pl.ci == 64 && pl.nco == 1) return launch_s<1, 64, 1, TW, TH, true>(a, pl.wgs, s);
    }
    lf::set_error("lf_conv2d_bf16_train: no streaming kernel for cin %d nco %d c16 %d ksize %d", pl.ci, pl.nco, pl.c16,
                  ksize);
    return LF_ERR_INVALID;
}

}  // namespace

namespace lf {

ConvBf16sPlan conv_bf16s_plan(int n, int cin, int h, int w, int cout, int ksize, int x_bf16) {
    return plan_s(n, cin, h, w, cout, ksize, x_bf16);
}

int conv_bf16s_launch(ConvBf16Args a, const ConvBf16sPlan& pl, int ksize, hipStream_t s) {
    if (!pl.ok) {
        set_error("lf_conv2d_bf16_train: shape not covered by the streaming kernel");
        return LF_ERR_INVALID;
    }
    a.tiles_x = pl.tiles_x; a.tiles_y = pl.tiles_y; a.seg_tiles = pl.seg_tiles; a.segs = pl.segs;
    a.interleave = pl.interleave;
    if (pl.tw == 64) return dispatch_s<64, 4>(pl, ksize, a, s);
    return pl.tw == 32 ? dispatch_s<32, 8>(pl, ksize, a, s) : dispatch_s<16, 16>(pl, ksize, a, s);
}

}  // namespace lf
