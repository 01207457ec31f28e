// libleafhip — depthwise 3x3 convolution (fp32, NCHW, padding "same", depth multiplier 1): the first half of the
// separable conv block of leaf_cnn (srcs/model/cnn.py:22-25); the pointwise half is lf_conv2d_* with ksize == 1.
//
//   forward   y[n,c,i,j]  = sum_t w[c,t] * a[n,c,i+ky-1,j+kx-1],  t = ky*3+kx
//   backward  dw[c,t]     = sum_{n,i,j} dy[n,c,i,j] * a[n,c,i+ky-1,j+kx-1]
//             dx[n,c,i,j] (+)= sum_t w[c,t] * dy[n,c,i-ky+1,j-kx+1]        (the gradient wrt a)
// a = relu?(x*in_scale[c]+in_shift[c]) is the producer's BatchNorm(+ReLU), applied while loading; a tap outside
// the image adds exactly 0 (not relu(in_shift)).
//
// Nine FMAs per four-byte element: both kernels are bandwidth kernels, and the work is to move every byte once.
// A lane owns V adjacent columns (V = 4: one 16-byte load and store per row; V = 1 serves any width and any
// alignment) of a run of rows of one (n, c) plane and walks down them with a register ring of rows, so a row
// is loaded once; the two halo columns are single loads of lines the neighbouring lanes load anyway.  The units
// (plane, row segment, column group) are numbered column group fastest and dealt to the lanes in that order:
// a wave reads whole rows of a wide plane, or the rows of several small planes (28 x 28: nine planes to a wave).
// Planes are cut into row segments (each re-reads its two halo rows) only while there are too few units to fill
// the chip: the batch-256 training shapes walk whole columns.
//
// The weight gradient has no float atomics: every lane leaves its nine sums (summed in double precision, rounded
// once) in part[t][unit], and
// dwconv_reduce_kernel adds the units of a channel in a fixed order (fixed per-thread sequences, then a fixed
// tree), so two launches on the same inputs give the same bits.
#include "lf_common.h"

namespace {

constexpr int kBlock = 256;
constexpr long long kWantUnits = 256 * 4 * 4 * 64;   // four waves on every SIMD of 256 CUs
constexpr int kMinSegRows = 8;                        // a segment re-reads two rows: at most 25 % more input

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// How a shape is cut into units: V columns to a lane, cg column groups to a row, segs segments of seg_rows rows.
struct DwPlan {
    int v, cg, segs, seg_rows;
    long long units;
};
DwPlan dw_plan(int n, int c, int h, int wd, bool vec) {
    DwPlan p;
    p.v = vec ? 4 : 1;
    p.cg = wd / p.v;
    const long long base = (long long)n * c * p.cg;
    long long s = (kWantUnits + base - 1) / base;
    const long long max_segs = (h + kMinSegRows - 1) / kMinSegRows;
    if (s > max_segs) s = max_segs;
    if (s < 1) s = 1;
    p.seg_rows = (int)((h + s - 1) / s);
    p.segs = (h + p.seg_rows - 1) / p.seg_rows;
    p.units = base * p.segs;
    return p;
}

// The unit a thread walks.
struct DwUnit {
    long long u, plane;
    int ch, r0, r1, col;
    bool ok;
};
__device__ __forceinline__ DwUnit dw_unit(int c, int h, int cg, int segs, int seg_rows, long long units, int v) {
    DwUnit t;
    t.u = (long long)blockIdx.x * kBlock + threadIdx.x;
    t.ok = t.u < units;
    const int per_plane = segs * cg;
    t.plane = t.u / per_plane;
    const int rem = (int)(t.u - t.plane * per_plane);
    const int seg = rem / cg;
    t.col = (rem - seg * cg) * v;
    t.ch = (int)(t.plane % c);
    t.r0 = seg * seg_rows;
    t.r1 = min(h, t.r0 + seg_rows);
    return t;
}

// the prologue on one value, in the precision of the row it goes to (float: lf::pro_apply's arithmetic)
template <typename T>
__device__ __forceinline__ T pro_apply(T v, T sc, T sh, int relu) {
    v = fma(v, sc, sh);
    return relu ? fmax(v, T(0)) : v;
}

// Row `row` of a plane as the lane sees it: e[0] = the column left of its V columns, e[1..V] its own, e[V+1] the
// column right of them; everything outside the image is 0.  In two steps, so that a lane can ask for several rows
// before it needs any: load_raw has no branch — the addresses of a row or halo column outside the image are
// clamped into it (h >= 1) and what they return is dropped by finish_row, which widens to T, applies the prologue
// (PRO: relu?(v*sc+sh), sc = 1 and sh = 0 where the launch has a ReLU alone; T = double: in double precision) and
// puts the zeros in.
template <int V>
__device__ __forceinline__ void load_own(float (&e)[V + 2], const float* plane, int row, int wd, int col) {
    const float* p = plane + row * wd + col;
    if constexpr (V == 4) {
        const lf::f32x4 m = *reinterpret_cast<const lf::f32x4*>(p);
        e[1] = m.x; e[2] = m.y; e[3] = m.z; e[4] = m.w;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) e[1 + k] = p[k];
    }
}
template <int V>
__device__ __forceinline__ void load_raw(float (&e)[V + 2], const float* __restrict__ plane, int row, int h, int wd,
                                         int col) {
    const int rc = min(max(row, 0), h - 1);
    load_own<V>(e, plane, rc, wd, col);
    const float* p = plane + rc * wd + col;
    e[0] = p[col > 0 ? -1 : 0];
    e[V + 1] = p[col + V < wd ? V : V - 1];
}
template <int V, bool PRO, typename T>
__device__ __forceinline__ void finish_row(T (&e)[V + 2], const float (&raw)[V + 2], int row, int h, int wd, int col,
                                           T sc, T sh, int relu) {
    const bool in = row >= 0 && row < h;
#pragma unroll
    for (int k = 0; k < V + 2; ++k) {
        T v = (T)raw[k];
        if constexpr (PRO) v = pro_apply<T>(v, sc, sh, relu);
        const bool ok = in && (k == 0 ? col > 0 : (k == V + 1 ? col + V < wd : true));
        e[k] = ok ? v : T(0);
    }
}
template <int V, typename T>
__device__ __forceinline__ void copy_row(T (&d)[V + 2], const T (&s)[V + 2]) {
#pragma unroll
    for (int k = 0; k < V + 2; ++k) d[k] = s[k];
}
template <int V>
__device__ __forceinline__ void store_own(float* __restrict__ p, const float (&o)[V]) {
    if constexpr (V == 4) {
        lf::f32x4 m;
        m.x = o[0]; m.y = o[1]; m.z = o[2]; m.w = o[3];
        *reinterpret_cast<lf::f32x4*>(p) = m;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) p[k] = o[k];
    }
}
// o[j] = sum_{ky,kx} wk[ky*3+kx] * r[ky][j+kx]: the 3x3 correlation of three ring rows, one ascending FMA chain
template <int V>
__device__ __forceinline__ void corr3(float (&o)[V], const float (&wk)[9], const float (&r0)[V + 2],
                                      const float (&r1)[V + 2], const float (&r2)[V + 2]) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float s = 0.f;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) s = fmaf(wk[kx], r0[j + kx], s);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) s = fmaf(wk[3 + kx], r1[j + kx], s);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) s = fmaf(wk[6 + kx], r2[j + kx], s);
        o[j] = s;
    }
}

// R = the rows a lane asks for before it waits for any of them: the bytes a wave keeps in flight.  Measured at
// 32 x 224 x 224, batch 256: one row per iteration with the loads under their bounds checks (a branch, then the
// prologue, per row) ran the forward at 3.8 TB/s and four such rows at 4.4; with load_raw's branch-free loads
// issued together it is 4.9 TB/s at two, four and eight rows alike, and the backward with dx went from 3.7 to
// 4.9 TB/s at two, three and four rows alike — the depth is no longer what limits them.
#ifndef LF_DW_ROWS_FWD   // development builds try other depths
#define LF_DW_ROWS_FWD 4
#endif
#ifndef LF_DW_ROWS_BWD
#define LF_DW_ROWS_BWD 2
#endif
template <int V>
struct Rows {
    static constexpr int kFwd = V == 4 ? LF_DW_ROWS_FWD : 2, kBwd = V == 4 ? LF_DW_ROWS_BWD : 2;
};

template <int V, bool PRO>
__global__ __launch_bounds__(kBlock) void dwconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            float* __restrict__ y, int c, int h, int wd, int cg,
                                                            int segs, int seg_rows, long long units,
                                                            const float* __restrict__ in_scale,
                                                            const float* __restrict__ in_shift, int in_relu) {
    constexpr int R = Rows<V>::kFwd;
    const DwUnit t = dw_unit(c, h, cg, segs, seg_rows, units, V);
    if (!t.ok) return;
    float wk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = w[t.ch * 9 + k];
    const float sc = PRO && in_scale ? in_scale[t.ch] : 1.f, sh = PRO && in_scale ? in_shift[t.ch] : 0.f;
    const size_t base = (size_t)t.plane * ((size_t)h * wd);
    const float* xp = x + base;
    float* yp = y + base;
    const int hl = min(h, t.r1 + 1);   // rows from here on are not needed by this segment: they count as zero

    float a[R + 2][V + 2];   // rows i - 1 .. i + R of the ring
    float raw[R][V + 2];
    load_raw<V>(raw[0], xp, t.r0 - 1, hl, wd, t.col);
    load_raw<V>(raw[1], xp, t.r0, hl, wd, t.col);
    finish_row<V, PRO, float>(a[0], raw[0], t.r0 - 1, hl, wd, t.col, sc, sh, in_relu);
    finish_row<V, PRO, float>(a[1], raw[1], t.r0, hl, wd, t.col, sc, sh, in_relu);
    for (int i = t.r0; i < t.r1; i += R) {
#pragma unroll
        for (int k = 0; k < R; ++k) load_raw<V>(raw[k], xp, i + k + 1, hl, wd, t.col);
#pragma unroll
        for (int k = 0; k < R; ++k)
            finish_row<V, PRO, float>(a[k + 2], raw[k], i + k + 1, hl, wd, t.col, sc, sh, in_relu);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (i + k < t.r1) {
                float o[V];
                corr3<V>(o, wk, a[k], a[k + 1], a[k + 2]);
                store_own<V>(yp + (i + k) * wd + t.col, o);
            }
        }
        copy_row<V, float>(a[0], a[R]);
        copy_row<V, float>(a[1], a[R + 1]);
    }
}

// One pass over dy and x for both gradients.  DX: the input gradient is wanted (dy then needs its ring and halo;
// without it only the lane's own columns of row i are read).  part[t][unit] receives the lane's nine dw sums.
// The dw sums run in double precision on a formed in double precision (the f64 FMA rate is far above what a
// bandwidth kernel needs): a lane's partial sum is rounded once, so dw is within (number of partials) roundings of
// the exact sum whatever the prologue, which is at most one rounding per summed term.
template <int V, bool PRO, bool DX>
__global__ __launch_bounds__(kBlock) void dwconv_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ dy, float* __restrict__ dx,
                                                            float* __restrict__ part, int c, int h, int wd, int cg,
                                                            int segs, int seg_rows, long long units,
                                                            const float* __restrict__ in_scale,
                                                            const float* __restrict__ in_shift, int in_relu,
                                                            int accumulate) {
    constexpr int R = Rows<V>::kBwd;
    static_assert(R >= 2, "the first two rows of the ring go through raw[0], raw[1]");
    const DwUnit t = dw_unit(c, h, cg, segs, seg_rows, units, V);
    if (!t.ok) return;
    float wf[9];   // the flipped taps: dx is the correlation of dy with them
#pragma unroll
    for (int k = 0; k < 9; ++k) wf[k] = DX ? w[t.ch * 9 + 8 - k] : 0.f;
    const double sc = PRO && in_scale ? (double)in_scale[t.ch] : 1.0, sh = PRO && in_scale ? (double)in_shift[t.ch] : 0.0;
    const size_t base = (size_t)t.plane * ((size_t)h * wd);
    const float* xp = x + base;
    const float* gp = dy + base;
    const int hl = min(h, t.r1 + 1);

    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    double a[R + 2][V + 2];   // rows i - 1 .. i + R of a
    float g[R + 2][V + 2];    // and of dy (DX), or g[k + 1] = the lane's own columns of row i + k
    float raw[R][V + 2], graw[R][V + 2], old[R][V + 2];
    load_raw<V>(raw[0], xp, t.r0 - 1, hl, wd, t.col);
    load_raw<V>(raw[1], xp, t.r0, hl, wd, t.col);
    if constexpr (DX) {
        load_raw<V>(graw[0], gp, t.r0 - 1, hl, wd, t.col);
        load_raw<V>(graw[1], gp, t.r0, hl, wd, t.col);
        finish_row<V, false, float>(g[0], graw[0], t.r0 - 1, hl, wd, t.col, 1.f, 0.f, 0);
        finish_row<V, false, float>(g[1], graw[1], t.r0, hl, wd, t.col, 1.f, 0.f, 0);
    }
    finish_row<V, PRO, double>(a[0], raw[0], t.r0 - 1, hl, wd, t.col, sc, sh, in_relu);
    finish_row<V, PRO, double>(a[1], raw[1], t.r0, hl, wd, t.col, sc, sh, in_relu);
    for (int i = t.r0; i < t.r1; i += R) {
        // every load of the R rows first; a row past the segment is asked for at the segment's last row (its own
        // columns: what comes back is not used)
#pragma unroll
        for (int k = 0; k < R; ++k) {
            load_raw<V>(raw[k], xp, i + k + 1, hl, wd, t.col);
            const int own = min(i + k, t.r1 - 1);
            if constexpr (DX) {
                load_raw<V>(graw[k], gp, i + k + 1, hl, wd, t.col);
                if (accumulate) load_own<V>(old[k], dx + base, own, wd, t.col);
            } else {
                load_own<V>(g[k + 1], gp, own, wd, t.col);
            }
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            finish_row<V, PRO, double>(a[k + 2], raw[k], i + k + 1, hl, wd, t.col, sc, sh, in_relu);
            if constexpr (DX) finish_row<V, false, float>(g[k + 2], graw[k], i + k + 1, hl, wd, t.col, 1.f, 0.f, 0);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const bool in = i + k < t.r1;
            if constexpr (DX) {
                if (in) {
                    float o[V];
                    corr3<V>(o, wf, g[k], g[k + 1], g[k + 2]);
                    if (accumulate)
#pragma unroll
                        for (int j = 0; j < V; ++j) o[j] += old[k][1 + j];
                    store_own<V>(dx + base + (i + k) * wd + t.col, o);
                }
            }
            // dw[ky*3+kx] += sum_j dy[i+k][j] * a[i+k+ky-1][j+kx-1]; a row past the segment counts as dy = 0
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const double gv = in ? (double)g[k + 1][1 + j] : 0.0;
                    acc[kx] = fma(gv, a[k][j + kx], acc[kx]);
                    acc[3 + kx] = fma(gv, a[k + 1][j + kx], acc[3 + kx]);
                    acc[6 + kx] = fma(gv, a[k + 2][j + kx], acc[6 + kx]);
                }
        }
        copy_row<V, double>(a[0], a[R]);
        copy_row<V, double>(a[1], a[R + 1]);
        if constexpr (DX) {
            copy_row<V, float>(g[0], g[R]);
            copy_row<V, float>(g[1], g[R + 1]);
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) part[(size_t)k * (size_t)units + (size_t)t.u] = (float)acc[k];
}

// dw[ch][t] = the sum of part[t][unit] over the units of channel ch (planes ch, ch + c, ...; per_plane units to a
// plane).  One workgroup per (ch, t): thread i adds values i, i + 256, ... of the channel's sequence in that order,
// and the 256 sums meet in a fixed tree.
__global__ __launch_bounds__(kBlock) void dwconv_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                               int n, int c, int per_plane, long long units) {
    __shared__ float red[kBlock];
    const int ch = blockIdx.x / 9, t = blockIdx.x % 9, tid = threadIdx.x;
    const float* src = part + (size_t)t * (size_t)units;
    const long long total = (long long)n * per_plane;
    float s = 0.f;
    for (long long i = tid; i < total; i += kBlock) {
        const long long im = i / per_plane;
        const int r = (int)(i - im * per_plane);
        s += src[(size_t)(im * c + ch) * (size_t)per_plane + (size_t)r];
    }
    red[tid] = s;
    __syncthreads();
#pragma unroll
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if (tid < half) red[tid] += red[tid + half];
        __syncthreads();
    }
    if (tid == 0) dw[ch * 9 + t] = red[0];
}

// what every entry point checks of a shape; the message names `who`
int dw_check_dims(const char* who, int n, int c, int h, int wd) {
    LF_REQUIRE(n > 0 && c > 0 && h > 0 && wd > 0, "%s: bad dims n=%d c=%d h=%d w=%d", who, n, c, h, wd);
    LF_REQUIRE(n <= 65535, "%s: batch too large (n=%d, at most 65535)", who, n);
    LF_REQUIRE((size_t)h * wd < (1ull << 30), "%s: plane of %d x %d is too large for 32-bit offsets", who, h, wd);
    LF_REQUIRE((long long)c * 9 < (1ll << 31) && (long long)n * c * wd < (1ll << 31),
               "%s: too many planes for one launch (n=%d c=%d w=%d)", who, n, c, wd);
    return LF_OK;
}
size_t dw_part_bytes(const DwPlan& p) { return (size_t)p.units * 9 * sizeof(float); }
unsigned dw_grid(const DwPlan& p) { return (unsigned)((p.units + kBlock - 1) / kBlock); }

}  // namespace

extern "C" {

int lf_dwconv3x3_f32(const float* x, const float* w, float* y, int n, int c, int h, int wd, const float* in_scale,
                     const float* in_shift, int in_relu, lf_stream_t stream) {
    const char* who = "lf_dwconv3x3_f32";
    LF_REQUIRE(x && w && y, "%s: null buffer", who);
    if (const int rc = dw_check_dims(who, n, c, h, wd)) return rc;
    LF_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "%s: in_scale/in_shift must both be set", who);
    const bool vec = wd % 4 == 0 && aligned16(x) && aligned16(y);
    const bool pro = in_scale != nullptr || in_relu != 0;
    const DwPlan p = dw_plan(n, c, h, wd, vec);
    hipStream_t s = lf::as_stream(stream);
    auto kernel = vec ? (pro ? dwconv_fwd_kernel<4, true> : dwconv_fwd_kernel<4, false>)
                      : (pro ? dwconv_fwd_kernel<1, true> : dwconv_fwd_kernel<1, false>);
    kernel<<<dw_grid(p), kBlock, 0, s>>>(x, w, y, c, h, wd, p.cg, p.segs, p.seg_rows, p.units, in_scale, in_shift,
                                         in_relu);
    return lf::check_launch(who);
}

size_t lf_dwconv3x3_bwd_workspace(int n, int c, int h, int wd) {
    if (n <= 0 || c <= 0 || h <= 0 || wd <= 0 || n > 65535 || (size_t)h * wd >= (1ull << 30)) return 0;
    // the launch picks the 4-column walk only for 16-byte aligned buffers: room for either
    const size_t scalar = dw_part_bytes(dw_plan(n, c, h, wd, false));
    const size_t vec = wd % 4 == 0 ? dw_part_bytes(dw_plan(n, c, h, wd, true)) : 0;
    return scalar > vec ? scalar : vec;
}

int lf_dwconv3x3_bwd_f32(const float* x, const float* w, const float* dy, float* dx, int accumulate, float* dw, int n,
                         int c, int h, int wd, const float* in_scale, const float* in_shift, int in_relu,
                         void* workspace, size_t ws_bytes, lf_stream_t stream) {
    const char* who = "lf_dwconv3x3_bwd_f32";
    LF_REQUIRE(x && w && dy && dw && workspace, "%s: null buffer", who);
    if (const int rc = dw_check_dims(who, n, c, h, wd)) return rc;
    LF_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "%s: in_scale/in_shift must both be set", who);
    LF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "%s: workspace must be 4-byte aligned", who);
    const bool vec = wd % 4 == 0 && aligned16(x) && aligned16(dy) && (dx == nullptr || aligned16(dx));
    const bool pro = in_scale != nullptr || in_relu != 0;
    const DwPlan p = dw_plan(n, c, h, wd, vec);
    LF_REQUIRE(ws_bytes >= dw_part_bytes(p), "%s: workspace of %zu bytes, %zu needed", who, ws_bytes,
               dw_part_bytes(p));
    hipStream_t s = lf::as_stream(stream);
    float* part = static_cast<float*>(workspace);
    auto pick = [&](auto v4, auto v1) { return vec ? v4 : v1; };
    auto kernel =
        dx != nullptr
            ? (pro ? pick(dwconv_bwd_kernel<4, true, true>, dwconv_bwd_kernel<1, true, true>)
                   : pick(dwconv_bwd_kernel<4, false, true>, dwconv_bwd_kernel<1, false, true>))
            : (pro ? pick(dwconv_bwd_kernel<4, true, false>, dwconv_bwd_kernel<1, true, false>)
                   : pick(dwconv_bwd_kernel<4, false, false>, dwconv_bwd_kernel<1, false, false>));
    kernel<<<dw_grid(p), kBlock, 0, s>>>(x, w, dy, dx, part, c, h, wd, p.cg, p.segs, p.seg_rows, p.units, in_scale,
                                         in_shift, in_relu, accumulate);
    if (const int rc = lf::check_launch(who)) return rc;
    dwconv_reduce_kernel<<<(unsigned)(c * 9), kBlock, 0, s>>>(part, dw, n, c, p.segs * p.cg, p.units);
    return lf::check_launch(who);
}

}  // extern "C"
