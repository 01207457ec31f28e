// libleafhip — the K-chunked convolution with bf16 operands and fp32 accumulation.
//
// The reference trains and predicts under Keras' `mixed_float16` policy unless told otherwise
// (train.py:53-117, `--no-mixed-precision`); BASELINE configs[4] asks for reduced-precision
// inference.  This kernel serves that mode at inference and in the mixed-precision training step
// (forward and input-gradient convolutions the streaming kernel of lf_conv_bf16s.hip does not take).
// Input and output are fp32 or bf16 NCHW (XBF / YBF); the operands are rounded to bf16 while staged
// and multiplied on `v_mfma_f32_32x32x16_bf16` with fp32 accumulators — 16x the matrix rate of the
// fp32 path, so the kernel is bound by staging and HBM, not by the MFMA pipe.  Epilogues: inference
// applies the layer's folded BatchNorm(+ReLU) before rounding; training (TR) accumulates into the
// output and leaves per-tile BatchNorm statistics or BatchNorm-backward sums of the stored values.
//
// Implicit GEMM D[co][pixel] = sum_k W[co][k] X[k][pixel], K = (input channel, tap).  Workgroup =
// 32x8 output pixels x 64 output channels (32x16 x 32 when cout is an odd multiple of 32); per 16-channel chunk the input patch sits in LDS as
// eight planes of channel PAIRS (one dword = bf16(ci), bf16(ci+1) of one pixel), so the B operand of
// a lane (one pixel, eight consecutive channels) is four conflict-free ds_read_b32 and staging is
// one ds_write_b128 per four pixels of a pair plane; weights are pre-packed once per model to
// [chunk][tap][cout][16] bf16 so the A operand (one output channel, eight channels) is one 16-byte
// LDS read.
//
// Every bf16 convolution entry (lf_conv2d_bf16_act, _act_mean, _train, _f32) goes through conv_bf16_launch below, which
// runs this kernel or the streaming one as bf16_route decides.
#include "lf_common.h"
#include <stdlib.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 32;            // output tile width; height = 4 waves x NB rows
constexpr int kPW = 40;           // patch row pitch in dwords: columns x0-4 .. x0+35
constexpr int kKC = 2;             // 16-channel k-steps per staged chunk (32 input channels)
constexpr int kMaxPrologueCin = 512;   // input channels a fused prologue (scale, shift) may have

using lf::bf16x8;
using lf::f32x16;
using lf::f32x4;
using lf::u32x2;
using lf::half_sum32;
using lf::pack_bf16;
using lf::bf16_down;
using lf::bf16_up;

// (three or four workgroups per CU would need <= 168 / 128 registers: the spills cost more than the
// occupancy brings — 40.4 k and 24.5 k img/s against 47.3 k for the whole forward pass)
template <int TAPS, int NCO, int NB, bool XBF, bool YBF, bool TR = false, bool WIDE = false>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_bf16_kernel(lf::ConvBf16Args p) {
    static_assert(!WIDE || (YBF && NCO == 2 && NB == 2), "the 16-byte epilogue: bf16 output, 32x8 tile");
    static_assert(!TR || YBF, "the training epilogue stores bf16");
    constexpr int kTH = 4 * NB;
    constexpr int R = TAPS == 9 ? 1 : 0, PH = kTH + 2 * R, KS = TAPS == 9 ? 3 : 1;
    // one LDS buffer: input patch | weight slice; the training epilogue's transpose buffer (fp32
    // [32 channels][256 pixels]) reuses it once the chunk loop is done
    constexpr int KC = kKC;   // 16-channel k-steps staged per barrier pair
    constexpr int kPatchB = KC * 8 * PH * kPW * 4, kWlB = KC * TAPS * NCO * 32 * 2 * 16;
    constexpr bool kWide = WIDE;   // bf16 output, 32x8 tile, w % 8 == 0: 16-byte epilogue through LDS
    constexpr int kSmemB = (kWide && kPatchB + kWlB < 32 * 256 * 4) ? 32 * 256 * 4 : kPatchB + kWlB;
    __shared__ __attribute__((aligned(16))) unsigned char smem[kSmemB];
    uint32_t (*patch)[PH][kPW] = reinterpret_cast<uint32_t (*)[PH][kPW]>(smem);
    lf::u32x4* wl = reinterpret_cast<lf::u32x4*>(smem + kPatchB);
    __shared__ float eps[2][NCO * 32];  // epilogue scale / shift of this workgroup's output channels
    // The prologue's per-channel scale / shift, read from LDS while staging: fetched from global memory there
    // (one dependent round trip per staged channel pair, between the two barriers of every chunk) they were
    // what the kernel waited for.
    __shared__ float lsc[2][kMaxPrologueCin];
    // XCD-aware order (see lf_conv.hip): XCD k walks the k-th contiguous share of the
    // (tile, channel group, image) space, so tiles that share halo rows meet in one L2
    const lf::Block3 blk = lf::xcd_block3();
    const int n = blk.z, cog = blk.y, tile = blk.x;
    const int tiles_x = (p.w + kTW - 1) / kTW;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int x0 = tx * kTW, y0 = ty * kTH;
    const int co0 = cog * (NCO * 32);
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, px = lane & 31, half = lane >> 5;
    const size_t hw = (size_t)p.h * p.w;

    f32x16 acc[NB][NCO];
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NCO; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

    // Staging is software-pipelined through registers: the global loads of chunk c+1 are issued before
    // the MFMAs of chunk c and land in LDS after them.  A chunk is 32 input channels (two MFMA k-steps per
    // tap): measured on 128->128 @56, batch 256 (scripts/microbench/conv_modes.py, ablation builds), the
    // matrix phase alone takes 212 us and the loads + LDS stores alone 190 us, but with 16-channel chunks
    // (31 KB in flight per workgroup, two workgroups per CU, one MFMA phase of ~0.5 us to land in) the two
    // added up to 547 us: the L2 -> CU path needs more bytes in flight, for longer, to run at its rate.
    // The loads are buffer loads: an offset past the end of the resource returns zero WITHOUT a memory
    // access, which gives the image border, the channel padding and the chunk past the last for free and
    // keeps every load unconditional.
    constexpr int kPatchItems = KC * 8 * PH * (kPW / 4);
    constexpr int NP = (kPatchItems + kThreads - 1) / kThreads;
    constexpr int kWItems = KC * TAPS * NCO * 64;
    constexpr int NW = (kWItems + kThreads - 1) / kThreads;
    struct Raw {  // four pixels of one channel as loaded
        f32x4 f;
        u32x2 h;
    };
    Raw ra[NP], rb[NP];
    lf::u32x4 rw[NW];
    constexpr unsigned kEl = XBF ? 2u : 4u;   // bytes per input element
    const unsigned plane_b = (unsigned)hw * kEl;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(static_cast<const unsigned char*>(p.x)) + (size_t)n * p.cin * hw * kEl, 0,
        (unsigned)p.cin * plane_b, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint16_t*>(p.wprep), 0, (unsigned)((size_t)p.chunks16 * TAPS * p.cout * 32), 0x00020000);

    // Per-slot geometry does not depend on the chunk.  A slot's flat index (pair plane, patch row,
    // column group) is also its LDS position / 4, so only the global side needs a register: the
    // byte offset of its four pixels inside a channel plane, or kOutside (past every resource).
    constexpr unsigned kOutside = 0x80000000u;
    unsigned g_off[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int it = tid + k * kThreads;
        const int pl = it / (PH * (kPW / 4)), rem = it - pl * (PH * (kPW / 4));
        const int row = rem / (kPW / 4), q = rem - row * (kPW / 4);
        const int gy = y0 - R + row, gx = x0 - 4 + 4 * q;
        // w % 4 == 0: a group of four columns is inside the image or outside it as a whole
        const bool inside = it < kPatchItems && gy >= 0 && gy < p.h && gx >= 0 && gx < p.w;
        g_off[k] = inside ? ((unsigned)gy * (unsigned)p.w + (unsigned)gx) * kEl : kOutside;
    }
    auto plane_of = [&](int k) { return (tid + k * kThreads) / (PH * (kPW / 4)); };
    auto load_raw = [&](Raw& r, unsigned off) {
        if (XBF)
            r.h = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(xr, off, 0, 0));
        else
            r.f = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
    };
    const unsigned wchunk_b = (unsigned)(TAPS * p.cout * 32);   // one 16-channel slice of the packed weights
    auto issue = [&](int c) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            // channel >= cin (padding of the last chunk, or the chunk past the last): past the resource
            const unsigned o = (unsigned)(c * (16 * KC) + 2 * plane_of(k)) * plane_b + g_off[k];
            load_raw(ra[k], g_off[k] == kOutside ? kOutside : o);
            load_raw(rb[k], g_off[k] == kOutside ? kOutside : o + plane_b);
        }
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int it = tid + k * kThreads;
            const int kk = it / (TAPS * NCO * 64), r1 = it - kk * (TAPS * NCO * 64);
            const int tap = r1 / (NCO * 64), rem = r1 - tap * (NCO * 64);
            const unsigned o = (unsigned)(c * KC + kk) * wchunk_b +
                               (unsigned)((tap * p.cout + co0 + (rem >> 1)) * 32 + 16 * (rem & 1));
            rw[k] = __builtin_bit_cast(lf::u32x4, __builtin_amdgcn_raw_buffer_load_b128(wr, it < kWItems ? o : kOutside, 0, 0));
        }
    };
    auto widen = [&](const Raw& r, int ci) -> f32x4 {  // fp32 values with the fused prologue applied
        f32x4 v;
        if (XBF)
            lf::unpack_bf16<4>(r.h, v);
        else
            v = r.f;
        // (this kernel alone also takes a ReLU without a scale — its entries do not forbid it —, so the two are
        // applied apart and not through lf::pro_apply)
        if (p.in_scale) {
            const float sc = lsc[0][ci], sh = lsc[1][ci];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaf(v[e], sc, sh);
        }
        if (p.in_relu)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
        return v;
    };
    const bool passthrough = XBF && p.in_scale == nullptr && !p.in_relu;  // bf16 in, no prologue
    uint32_t* patch_flat = &patch[0][0][0];
    auto commit = [&](int c) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            if (tid + k * kThreads >= kPatchItems) continue;
            const int ci0 = c * (16 * KC) + 2 * plane_of(k);
            lf::u32x4 o;
            if (passthrough) {
                // the stored values are the operands (what was not loaded is exactly zero): interleave the
                // two channels' bf16 pixels
                const u32x2 a = ra[k].h, b = rb[k].h;
                o.x = (a.x & 0xffffu) | (b.x << 16);
                o.y = (a.x >> 16) | (b.x & 0xffff0000u);
                o.z = (a.y & 0xffffu) | (b.y << 16);
                o.w = (a.y >> 16) | (b.y & 0xffff0000u);
            } else {
                const bool inside = g_off[k] != kOutside;   // the prologue must not touch the padding
                f32x4 a = {0.0f, 0.0f, 0.0f, 0.0f}, b = {0.0f, 0.0f, 0.0f, 0.0f};
                if (inside && ci0 < p.cin) a = widen(ra[k], ci0);
                if (inside && ci0 + 1 < p.cin) b = widen(rb[k], ci0 + 1);
                o.x = pack_bf16(a[0], b[0]);
                o.y = pack_bf16(a[1], b[1]);
                o.z = pack_bf16(a[2], b[2]);
                o.w = pack_bf16(a[3], b[3]);
            }
            *reinterpret_cast<lf::u32x4*>(patch_flat + 4 * (tid + k * kThreads)) = o;
        }
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int it = tid + k * kThreads;
            if (it >= kWItems) break;
            wl[it] = rw[k];
        }
    };

    if (p.in_scale)   // read back after the first barrier of the chunk loop
        for (int c = tid; c < p.cin; c += kThreads) {
            lsc[0][c] = p.in_scale[c];
            lsc[1][c] = p.in_shift[c];
        }
    if (p.out_scale && tid < NCO * 32) {  // read back after the chunk loop's barriers
        eps[0][tid] = p.out_scale[co0 + tid];
        eps[1][tid] = p.out_shift[co0 + tid];
    }
    // training, 32x8 tile, 16-byte rows: the epilogue works on (8 consecutive pixels, one channel)
    // per thread — its read-modify-write operands are requested now and arrive during the MFMAs
    const bool wide = kWide;
    const int eg = tid & 31, ec = tid >> 5;
    const int egy = y0 + (eg >> 2), egx = x0 + 8 * (eg & 3);
    const bool eok = egy < p.h && egx < p.w;
    const size_t epo = eok ? (size_t)egy * p.w + egx : 0;
    lf::u32x4 rold[(kWide && TR) ? NCO : 1][4], rmask[(kWide && TR) ? NCO : 1][4];
    if (wide && TR) {  // (inference: nothing is read back)
        if (p.accumulate)
            lf::row8_request(rold, static_cast<const uint16_t*>(p.y) + (size_t)n * p.cout * hw, co0, ec, hw, epo);
        if (p.stat_mask_y != nullptr) lf::row8_request(rmask, p.stat_mask_y + (size_t)n * p.cout * hw, co0, ec, hw, epo);
    }
    issue(0);
    for (int c = 0; c < p.chunks; ++c) {
        __syncthreads();  // the previous chunk's LDS reads are done
        commit(c);
        issue(c + 1);     // past the last chunk: no memory access
        __syncthreads();
        // One B operand (a patch row shifted by dx) serves every (output row, dy) pair that reads
        // it: NB + KS - 1 LDS fetches per dx instead of NB * KS.
#pragma unroll
        for (int kd = 0; kd < KC * KS; ++kd) {
            const int kk = kd / KS, dx = kd - kk * KS;
            bf16x8 A[KS][NCO];
#pragma unroll
            for (int dy = 0; dy < KS; ++dy)
#pragma unroll
                for (int cb = 0; cb < NCO; ++cb)
                    A[dy][cb] = __builtin_bit_cast(
                        bf16x8, wl[((((kk * KS + dy) * KS + dx) * NCO + cb) * 32 + px) * 2 + half]);
            const int col = 4 + px + dx - R;
#pragma unroll
            for (int prow = 0; prow < NB + KS - 1; ++prow) {
                const int row = NB * wv + prow;
                lf::u32x4 bv;
                bv.x = patch[8 * kk + 4 * half + 0][row][col];
                bv.y = patch[8 * kk + 4 * half + 1][row][col];
                bv.z = patch[8 * kk + 4 * half + 2][row][col];
                bv.w = patch[8 * kk + 4 * half + 3][row][col];
                const bf16x8 B = __builtin_bit_cast(bf16x8, bv);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const int dy = prow - nb;
                    if (dy < 0 || dy >= KS) continue;
#pragma unroll
                    for (int cb = 0; cb < NCO; ++cb)
                        acc[nb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[dy][cb], B, acc[nb][cb], 0, 0, 0);
                }
            }
        }
    }
    // D[row = output channel][col = pixel]: register r of a lane is channel 8*(r/4) + 4*half + r%4
    float* yn = static_cast<float*>(p.y) + (YBF ? 0 : (size_t)n * p.cout * hw);
    uint16_t* yb = static_cast<uint16_t*>(p.y) + (YBF ? (size_t)n * p.cout * hw : 0);
    const int gx = x0 + px;
    const bool stats = p.stat_part != nullptr, masked = p.stat_mask_y != nullptr;
    if (wide) {
        // through LDS: lane (pixel, 16 channels) -> thread (8 pixels, one channel): 16-byte stores,
        // and a channel's whole tile sits in one half-wave (no cross-wave reduction)
        float* le = reinterpret_cast<float*>(smem);
        uint16_t* yout = static_cast<uint16_t*>(p.y) + (size_t)n * p.cout * hw;
        const long long tg = (long long)n * gridDim.x + tile;
#pragma unroll
        for (int cb = 0; cb < NCO; ++cb) {
            __syncthreads();  // every wave is done with the staging LDS / with the previous block
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cl = 8 * (r >> 2) + 4 * half + (r & 3);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) le[cl * 256 + (NB * wv + nb) * 32 + px] = acc[nb][cb][r];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cl = 8 * j + ec, co = co0 + cb * 32 + cl;
                const lf::u32x4 o = lf::row8_finish(le + cl * 256 + 8 * eg, TR && p.accumulate, rold[TR ? cb : 0][j],
                                                    p.out_scale != nullptr, &eps[0][cb * 32 + cl], &eps[1][cb * 32 + cl],
                                                    p.out_relu);
                if (eok) *reinterpret_cast<lf::u32x4*>(yout + (size_t)co * hw + epo) = o;
                if (!TR || !stats) continue;
                float a = 0.f, b = 0.f;
                if (eok)
                    lf::row8_sums(o, masked, p.stat_pivot != nullptr ? p.stat_pivot + co : nullptr, p.mask_scale + co,
                                  p.mask_shift + co, rmask[TR ? cb : 0][j], p.mask_relu, a, b);
                a = half_sum32(a);
                b = half_sum32(b);
                if (eg == 31) {
                    float* dst = p.stat_part + ((size_t)co * (size_t)p.stat_tiles + (size_t)tg) * 2;
                    dst[0] = a;
                    dst[1] = b;
                }
            }
        }
        return;
    }
    if (!TR) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int gy = y0 + NB * wv + nb;
            if (gy >= p.h || gx >= p.w) continue;
#pragma unroll
            for (int cb = 0; cb < NCO; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int col = cb * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
                    const int co = co0 + col;
                    const size_t o = (size_t)co * hw + (size_t)gy * p.w + gx;
                    float v = acc[nb][cb][r];
                    if (p.out_scale) v = fmaf(v, eps[0][col], eps[1][col]);
                    if (p.out_relu) v = fmaxf(v, 0.0f);
                    if (YBF)
                        yb[o] = bf16_down(v);
                    else
                        yn[o] = v;
                }
        }
        return;
    }
    // ---- training: bf16 store (optionally on top of the old value) + per-tile channel sums of
    // the rounded values

    const uint16_t* my = masked ? p.stat_mask_y + (size_t)n * p.cout * hw : nullptr;
    float* red = reinterpret_cast<float*>(smem);  // [4 waves][NCO*32][2]
    static_assert(4 * NCO * 32 * 2 <= 8 * PH * kPW, "statistics scratch must fit the patch LDS");
    if (stats) __syncthreads();  // every wave is done with the staging LDS
    bool ok[NB];
    unsigned po[NB];  // pixel offset inside a channel plane (0 when outside the image)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int gy = y0 + NB * wv + nb;
        ok[nb] = gy < p.h && gx < p.w;
        po[nb] = ok[nb] ? (unsigned)gy * (unsigned)p.w + (unsigned)gx : 0u;
    }
#pragma unroll
    for (int cb = 0; cb < NCO; ++cb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int col = cb * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
            const int co = co0 + col;
            const size_t cbase = (size_t)co * hw;
            float oldv[NB], yv[NB];
            if (p.accumulate)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) oldv[nb] = bf16_up(yb[cbase + po[nb]]);
            if (masked)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) yv[nb] = bf16_up(my[cbase + po[nb]]);
            float s1 = 0.f, s2 = 0.f;
            const float pv = (stats && !masked && p.stat_pivot != nullptr) ? p.stat_pivot[co] : 0.f;
            const float msc = masked ? p.mask_scale[co] : 0.f, msh = masked ? p.mask_shift[co] : 0.f;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                float v = acc[nb][cb][r];
                if (p.accumulate) v += oldv[nb];
                if (p.out_scale) v = fmaf(v, eps[0][col], eps[1][col]);   // inference with sums: the folded BatchNorm
                if (p.out_relu) v = fmaxf(v, 0.0f);
                const uint16_t vb = bf16_down(v);
                if (ok[nb]) yb[cbase + po[nb]] = vb;
                if (!stats) continue;
                const float vr = bf16_up(vb);
                if (!masked) lf::stat_accumulate(vr, ok[nb], false, pv, 0.f, 0.f, 0.f, 0, s1, s2);
                else lf::stat_accumulate(vr, ok[nb], true, 0.f, yv[nb], msc, msh, p.mask_relu, s1, s2);
            }
            if (stats) {
                s1 = half_sum32(s1);
                s2 = half_sum32(s2);
                if (px == 31) {
                    red[(wv * (NCO * 32) + col) * 2] = s1;
                    red[(wv * (NCO * 32) + col) * 2 + 1] = s2;
                }
            }
        }
    }
    if (stats) {
        __syncthreads();
        lf::write_stat_part<4, NCO * 32>(p.stat_part, p.stat_tiles, p.cout, (long long)n * gridDim.x + tile, co0, red,
                                         tid, kThreads);
    }
}

// fp32 [cin][taps][cout] -> bf16 [chunk][tap][cout][16] (channels past cin are zero)
__global__ void prep_weights_bf16_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int cin,
                                         int taps, int cout, int chunks) {
    const size_t total = (size_t)chunks * taps * cout * 16;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i & 15);
        const size_t rest = i >> 4;
        const int co = (int)(rest % cout);
        const size_t rest2 = rest / cout;
        const int tap = (int)(rest2 % taps), c = (int)(rest2 / taps);
        const int ci = c * 16 + j;
        const float v = ci < cin ? w[((size_t)ci * taps + tap) * cout + co] : 0.0f;
        out[i] = __builtin_bit_cast(uint16_t, (__bf16)v);
    }
}

}  // namespace

namespace {

// cout % 64 == 0: two 32-channel blocks per workgroup share one staged 32x8 patch (four measured
// the same); cout == 32 (+64k): one block, and a 32x16 tile instead so that a staged patch
// still feeds 16 accumulator tiles per wave
inline int bf16_nco(int cout) { return cout % 64 == 0 ? 2 : 1; }
constexpr int bf16_nb(int nco) { return nco == 2 ? 2 : 4; }   // rows per wave: the tile is 4 * NB rows high
inline int bf16_tiles(int h, int w, int cout) {
    const int th = 4 * bf16_nb(bf16_nco(cout));
    return ((w + kTW - 1) / kTW) * ((h + th - 1) / th);
}

// rows of 16 bytes: the epilogue through LDS
inline bool bf16_wide(bool ybf, int nco, int w) { return ybf && nco == 2 && w % 8 == 0; }

// The entry points' routing, asked once per call: the streaming kernel (lf_conv_bf16s.hip) or the K-chunked one, and
// the partial sums either leaves.  The training convolution streams every shape the streaming kernel covers; the
// inference ones (kBf16Act, kBf16ActMean) only the 16- and 32-channel layers with bf16 output (16 output channels
// have no other kernel: the K-chunked one works in 32-channel blocks):
// the 224x224 stage (stem, 32->32): the streaming kernel (resident filter bank, 16-byte accesses).
// The 64-channel layers of the 112x112 stage stay on the K-chunked kernel: it was well ahead there
// without a read-modify-write epilogue (1.7 ms against 3.2 ms at 64->64, batch 1,024) and is level with
// the streaming kernel since that one got 64x4 tiles and per-XCD tile rows (whole forward pass
// 52.4 k img/s as routed here, 52.7 k with every covered layer on the streaming kernel).
enum { kBf16Act = 0, kBf16ActMean = 1, kBf16Train = 2 };
struct Bf16Route {
    bool streams;
    lf::ConvBf16sPlan s;   // streams: the streaming kernel's plan
    int units;             // partial sums per image and channel: segments (streaming) or tiles
    long long parts;       // statistics partials per channel: the streaming grid, or n * tiles
};
Bf16Route bf16_route(int entry, int y_bf16, int n, int cin, int h, int w, int cout, int ksize, int x_bf16) {
    Bf16Route r{};
    if (n <= 0 || cin <= 0 || h <= 0 || w <= 0 || cout <= 0) return r;
    if (entry == kBf16Train || (y_bf16 && (cout == 32 || cout == 16))) r.s = lf::conv_bf16s_plan(n, cin, h, w, cout, ksize, x_bf16);
    r.streams = r.s.ok;
    r.units = r.streams ? r.s.tiles_x * r.s.segs : bf16_tiles(h, w, cout);
    r.parts = r.streams ? r.s.wgs : (long long)n * r.units;
    return r;
}

template <int TAPS, bool XBF, bool YBF, bool TR>
void launch_conv_bf16_taps(const lf::ConvBf16Args& a, hipStream_t s) {
    const int nco = bf16_nco(a.cout);
    dim3 grid(bf16_tiles(a.h, a.w, a.cout), a.cout / (32 * nco), a.n);
    if (nco == 1) conv_bf16_kernel<TAPS, 1, bf16_nb(1), XBF, YBF, TR, false><<<grid, kThreads, 0, s>>>(a);
    else if (bf16_wide(YBF, nco, a.w)) conv_bf16_kernel<TAPS, 2, bf16_nb(2), XBF, YBF, TR, YBF><<<grid, kThreads, 0, s>>>(a);
    else conv_bf16_kernel<TAPS, 2, bf16_nb(2), XBF, YBF, TR, false><<<grid, kThreads, 0, s>>>(a);
}

template <bool YBF, bool TR>
void launch_conv_bf16(lf::ConvBf16Args a, int ksize, int x_bf16, hipStream_t s) {
    a.chunks16 = (a.cin + 15) / 16;
    a.chunks = (a.chunks16 + kKC - 1) / kKC;
    if (ksize == 3) x_bf16 ? launch_conv_bf16_taps<9, true, YBF, TR>(a, s) : launch_conv_bf16_taps<9, false, YBF, TR>(a, s);
    else x_bf16 ? launch_conv_bf16_taps<1, true, YBF, TR>(a, s) : launch_conv_bf16_taps<1, false, YBF, TR>(a, s);
}

// means[n][c] = scale * sum over the image's partial sums: `unit` layout part[(n * units + u) * c_total + c] (the
// streaming kernel's segments) or `tile` layout part[((c * n_total + n) * units + u) * 2] (the K-chunked kernel's
// per-tile statistics, sum in element 0).  Fixed order: deterministic.
__global__ void partial_sums_mean_kernel(const float* __restrict__ part, float* __restrict__ means, int n, int c,
                                         int units, int tile_layout, float scale) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * c) return;
    const int im = i / c, ch = i - im * c;
    float acc = 0.f;
    for (int u = 0; u < units; ++u)
        acc += tile_layout ? part[(((size_t)ch * n + im) * units + u) * 2] : part[((size_t)im * units + u) * c + ch];
    means[i] = acc * scale;
}

}  // namespace

extern "C" {

size_t lf_conv2d_bf16_weight_elems(int cin, int cout, int ksize) {
    if (cin <= 0 || cout <= 0 || (ksize != 1 && ksize != 3)) return 0;
    return (size_t)((cin + 15) / 16) * ksize * ksize * cout * 16;
}

int lf_conv2d_bf16_prep_weights(const float* w_iko, uint16_t* wprep, int cin, int cout, int ksize,
                                lf_stream_t stream) {
    LF_REQUIRE(w_iko && wprep, "lf_conv2d_bf16_prep_weights: null buffer");
    LF_REQUIRE(cin > 0 && cout > 0 && (ksize == 1 || ksize == 3), "lf_conv2d_bf16_prep_weights: bad dims");
    const int chunks = (cin + 15) / 16;
    const size_t total = lf_conv2d_bf16_weight_elems(cin, cout, ksize);
    prep_weights_bf16_kernel<<<lf::stream_grid(total, 256), 256, 0, lf::as_stream(stream)>>>(
        w_iko, wprep, cin, ksize * ksize, cout, chunks);
    return lf::check_launch("lf_conv2d_bf16_prep_weights");
}

// The one launch path of the bf16 convolutions: validates, fills the arguments and launches the kernel `r` (the
// caller's bf16_route for `entry`) names.  `a` arrives with the entry's pointers and flags set.
static int conv_bf16_launch(const char* who, int entry, const Bf16Route& r, lf::ConvBf16Args a, int x_bf16, int y_bf16,
                            int ksize, lf_stream_t stream) {
    LF_REQUIRE(a.x && a.wprep && a.y, "%s: null buffer", who);
    LF_REQUIRE(a.n > 0 && a.cin > 0 && a.h > 0 && a.w > 0 && a.cout > 0, "%s: bad dims", who);
    LF_REQUIRE(ksize == 1 || ksize == 3, "%s: ksize must be 1 or 3", who);
    LF_REQUIRE(a.w % 4 == 0, "%s: width must be a multiple of 4 (got %d)", who, a.w);
    LF_REQUIRE(r.streams || a.cout % 32 == 0,
               "%s: cout must be a multiple of 32, or a 16-channel shape of the streaming kernel (got cin %d cout %d)",
               who, a.cin, a.cout);
    LF_REQUIRE((a.in_scale == nullptr) == (a.in_shift == nullptr), "%s: scale/shift must both be set", who);
    LF_REQUIRE(a.in_scale == nullptr || a.cin <= kMaxPrologueCin,
               "%s: a fused prologue takes at most %d input channels (got %d)", who, kMaxPrologueCin, a.cin);
    LF_REQUIRE((a.out_scale == nullptr) == (a.out_shift == nullptr), "%s: out_scale/out_shift must both be set", who);
    // 32-bit buffer offsets: one image's input (plus the two staged chunks past its end that the pipeline asks
    // for and gets zeros back) and the packed weights must each stay below 2 GiB
    LF_REQUIRE((size_t)(a.cin + 2 * 16 * kKC) * a.h * a.w * (x_bf16 ? 2 : 4) < ((size_t)1 << 31) &&
                   lf_conv2d_bf16_weight_elems(a.cin, a.cout, ksize) * 2 < ((size_t)1 << 31),
               "%s: image or weights too large for 32-bit buffer offsets", who);
    LF_REQUIRE(a.n <= 65535, "%s: batch too large for grid.z", who);
    LF_REQUIRE(((reinterpret_cast<size_t>(a.x) | reinterpret_cast<size_t>(a.wprep)) & 15) == 0,
               "%s: x and wprep must be 16-byte aligned", who);
    hipStream_t s = lf::as_stream(stream);
    a.stat_tiles = r.parts;
    if (r.streams) {
        const int rc = lf::conv_bf16s_launch(a, r.s, ksize, s);
        if (rc != LF_OK) return rc;
    } else if (entry != kBf16Act) {
        launch_conv_bf16<true, true>(a, ksize, x_bf16, s);
    } else if (y_bf16) {
        launch_conv_bf16<true, false>(a, ksize, x_bf16, s);
    } else {
        launch_conv_bf16<false, false>(a, ksize, x_bf16, s);
    }
    return lf::check_launch(who);
}

// the arguments every entry has
static lf::ConvBf16Args bf16_args(const void* x, const uint16_t* wprep, void* y, int n, int cin, int h, int w, int cout,
                                  const float* in_scale, const float* in_shift, int in_relu) {
    lf::ConvBf16Args a{};
    a.x = x; a.wprep = wprep; a.y = y; a.n = n; a.cin = cin; a.h = h; a.w = w; a.cout = cout;
    a.in_scale = in_scale; a.in_shift = in_shift; a.in_relu = in_relu;
    return a;
}

int lf_conv2d_bf16_act(const void* x, int x_bf16, const uint16_t* wprep, void* y, int y_bf16, int n, int cin,
                       int h, int w, int cout, int ksize, const float* in_scale, const float* in_shift,
                       int in_relu, const float* out_scale, const float* out_shift, int out_relu,
                       lf_stream_t stream) {
    lf::ConvBf16Args a = bf16_args(x, wprep, y, n, cin, h, w, cout, in_scale, in_shift, in_relu);
    a.out_scale = out_scale; a.out_shift = out_shift; a.out_relu = out_relu;
    return conv_bf16_launch("lf_conv2d_bf16", kBf16Act, bf16_route(kBf16Act, y_bf16, n, cin, h, w, cout, ksize, x_bf16),
                            a, x_bf16, y_bf16, ksize, stream);
}

long long lf_conv2d_bf16_stats_tiles(int n, int cin, int h, int w, int cout, int ksize, int x_bf16) {
    return bf16_route(kBf16Train, 1, n, cin, h, w, cout, ksize, x_bf16).parts;
}

int lf_conv2d_bf16_train(const void* x, int x_bf16, const uint16_t* wprep, uint16_t* y, int n, int cin, int h,
                         int w, int cout, int ksize, const float* in_scale, const float* in_shift, int in_relu,
                         int accumulate, float* tile_part, size_t tile_part_bytes, const float* pivot,
                         const uint16_t* mask_y, const float* mask_scale, const float* mask_shift,
                         int mask_relu, lf_stream_t stream) {
    LF_REQUIRE(mask_y == nullptr || (tile_part && mask_scale && mask_shift),
               "lf_conv2d_bf16_train: mask_y needs tile_part and mask_scale / mask_shift");
    const Bf16Route r = bf16_route(kBf16Train, 1, n, cin, h, w, cout, ksize, x_bf16);
    if (tile_part != nullptr) {
        const size_t need = (size_t)r.parts * (size_t)cout * 2 * sizeof(float);
        if (tile_part_bytes < need) {
            lf::set_error("lf_conv2d_bf16_train: tile_part %zu bytes < %zu", tile_part_bytes, need);
            return LF_ERR_WORKSPACE;
        }
    }
    lf::ConvBf16Args a = bf16_args(x, wprep, y, n, cin, h, w, cout, in_scale, in_shift, in_relu);
    a.accumulate = accumulate;
    a.stat_part = tile_part; a.stat_pivot = pivot;
    a.stat_mask_y = mask_y; a.mask_scale = mask_scale; a.mask_shift = mask_shift; a.mask_relu = mask_relu;
    return conv_bf16_launch("lf_conv2d_bf16_train", kBf16Train, r, a, x_bf16, 1, ksize, stream);
}

// (the same routing as lf_conv2d_bf16_act: the streaming kernel for the 16- and 32-channel layers only, so that the
// stored activation is bit-equal with and without the means)
static size_t bf16_mean_workspace(const Bf16Route& r, int n, int cout) {
    return (size_t)n * r.units * cout * (r.streams ? 1 : 2) * sizeof(float);
}

size_t lf_conv2d_bf16_act_mean_workspace(int n, int cin, int h, int w, int cout, int ksize, int x_bf16) {
    return bf16_mean_workspace(bf16_route(kBf16ActMean, 1, n, cin, h, w, cout, ksize, x_bf16), n, cout);
}

int lf_conv2d_bf16_act_mean(const void* x, int x_bf16, const uint16_t* wprep, uint16_t* y, int n, int cin, int h, int w,
                            int cout, int ksize, const float* in_scale, const float* in_shift, int in_relu,
                            const float* out_scale, const float* out_shift, int out_relu, float* means,
                            void* workspace, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(means && workspace, "lf_conv2d_bf16_act_mean: null buffer");
    const Bf16Route r = bf16_route(kBf16ActMean, 1, n, cin, h, w, cout, ksize, x_bf16);
    const size_t need = bf16_mean_workspace(r, n, cout);
    if (ws_bytes < need) {
        lf::set_error("lf_conv2d_bf16_act_mean: workspace %zu < %zu bytes", ws_bytes, need);
        return LF_ERR_WORKSPACE;
    }
    lf::ConvBf16Args a = bf16_args(x, wprep, y, n, cin, h, w, cout, in_scale, in_shift, in_relu);
    a.out_scale = out_scale; a.out_shift = out_shift; a.out_relu = out_relu;
    float* part = static_cast<float*>(workspace);   // the streaming kernel's unit sums, or tile statistics (pivot 0)
    (r.streams ? a.unit_sums : a.stat_part) = part;
    const int rc = conv_bf16_launch("lf_conv2d_bf16_act_mean", kBf16ActMean, r, a, x_bf16, 1, ksize, stream);
    if (rc != LF_OK) return rc;
    partial_sums_mean_kernel<<<(n * cout + 255) / 256, 256, 0, lf::as_stream(stream)>>>(
        part, means, n, cout, r.units, r.streams ? 0 : 1, 1.0f / (float)((size_t)h * w));
    return lf::check_launch("lf_conv2d_bf16_act_mean");
}

int lf_conv2d_bf16_plan(int n, int cin, int h, int w, int cout, int ksize, int x_bf16, int y_bf16, int entry,
                        int accumulate, int mask, int* out) {
    LF_REQUIRE(out, "lf_conv2d_bf16_plan: null out");
    LF_REQUIRE(n > 0 && cin > 0 && h > 0 && w > 0 && cout > 0 && (ksize == 1 || ksize == 3),
               "lf_conv2d_bf16_plan: bad dims");
    LF_REQUIRE(entry == kBf16Act || entry == kBf16ActMean || entry == kBf16Train, "lf_conv2d_bf16_plan: bad entry");
    const int ybf = entry == kBf16Act ? (y_bf16 ? 1 : 0) : 1;
    for (int i = 0; i < 14; ++i) out[i] = 0;
    out[1] = ksize * ksize;
    out[7] = x_bf16 ? 1 : 0;
    out[8] = ybf;
    const Bf16Route r = bf16_route(entry, ybf, n, cin, h, w, cout, ksize, x_bf16);
    LF_REQUIRE(r.streams || cout % 32 == 0, "lf_conv2d_bf16_plan: no kernel covers cin %d cout %d", cin, cout);
    if (r.streams) {
        out[0] = 1;
        out[2] = r.s.ci;
        out[3] = r.s.c16 ? 0 : r.s.nco;
        out[5] = r.s.tw;
        out[6] = r.s.th;
        out[7] = r.s.xbf;                // dispatch_s: fp32 input is the stem (one padded 16-channel group)
        out[10] = lf::conv_bf16s_rmw(entry == kBf16Train ? accumulate : 0, entry == kBf16Train && mask) ? 1 : 0;
        out[11] = r.s.segs > 1 ? 1 : 0;
        out[12] = r.s.interleave;
        out[13] = lf::max_units_per_workgroup(n, r.units, r.s.wgs, r.s.interleave) > 1 ? 1 : 0;
        return LF_OK;
    }
    const int nco = bf16_nco(cout);
    out[3] = nco;
    out[4] = bf16_nb(nco);
    out[5] = kTW;
    out[6] = 4 * bf16_nb(nco);
    out[9] = entry == kBf16Act ? 0 : 1;
    out[10] = bf16_wide(ybf, nco, w) ? 1 : 0;
    return LF_OK;
}

int lf_conv2d_bf16_f32(const float* x, const uint16_t* wprep, float* y, int n, int cin, int h, int w,
                       int cout, int ksize, const float* in_scale, const float* in_shift, int in_relu,
                       lf_stream_t stream) {
    return lf_conv2d_bf16_act(x, 0, wprep, y, 0, n, cin, h, w, cout, ksize, in_scale, in_shift, in_relu, nullptr,
                              nullptr, 0, stream);
}

}  // extern "C"
