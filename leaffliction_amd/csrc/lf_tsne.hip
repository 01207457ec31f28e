// libleafhip — the embedding map: exact (dense) t-SNE of feature rows and the marks of its chart.  The rule, with the
// order of every sum, is stated in include/leafhip.h ("Embedding map") and DESIGN.md ("Embedding map").
//
// lf_tsne_perplexity_f32 and lf_tsne_symmetrize_f32 run once per fit; an iteration is lf_tsne_forces_f32 (the hot
// kernel: all n^2 pairs, P streamed once) and lf_tsne_step_f32 (one workgroup).  No float atomics anywhere: every sum
// has one order, which depends on n alone.
#include <math.h>

#include "lf_wave.h"

namespace {

using lf::f32x4;

constexpr int kMaxPoints = 16384;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

// ---------------------------------------------------------------------------------------------------------------
// Affinities

constexpr int kMaxEvals = 100;
constexpr double kEntropyTol = 1e-5;
constexpr int kRedDoubles = 16;   // [2][4] wave partials, then the two sums every thread reads back

// sums of two doubles over the workgroup of 256, the same bits in every thread (red: kRedDoubles doubles of LDS)
__device__ __forceinline__ void sum2_all(double (&v)[2], double* red) {
    lf::block_sum<2>(v, red);
    if (threadIdx.x == 0) {
        red[8] = v[0];
        red[9] = v[1];
    }
    __syncthreads();
    v[0] = red[8];
    v[1] = red[9];
}

// One workgroup per row.  d2 and p may be the same buffer: the row is in LDS before any of it is written, and no
// other workgroup touches it.
__global__ __launch_bounds__(kBlock) void perplexity_kernel(const float* d2, int n, double target, float* p,
                                                            double* __restrict__ beta_out,
                                                            int32_t* __restrict__ evals_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* red = reinterpret_cast<double*>(smem);
    float* row = reinterpret_cast<float*>(red + kRedDoubles);
    const int tid = threadIdx.x;
    const int i = blockIdx.x;
    const float* src = d2 + (size_t)i * n;

    float least = INFINITY;
    for (int j = tid; j < n; j += kBlock) {
        const float v = src[j];
        row[j] = v;
        if (j != i) least = fminf(least, v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) least = fminf(least, __shfl_xor(least, off, 64));
    if ((tid & 63) == 0) red[10 + (tid >> 6)] = (double)least;
    __syncthreads();   // the row and the waves' minima are in LDS
    const double dmin = fmin(fmin(red[10], red[11]), fmin(red[12], red[13]));

    double beta = 1.0, lo = 0.0, hi = INFINITY, total = 1.0;
    int evals = 0;
    for (;;) {
        double s[2] = {0.0, 0.0};
        for (int j = tid; j < n; j += kBlock) {
            if (j == i) continue;
            const double d = (double)row[j] - dmin;
            const double e = exp(-beta * d);
            s[0] += e;
            s[1] += d * e;
        }
        sum2_all(s, red);
        total = s[0];
        ++evals;
        const double diff = log(s[0]) + beta * s[1] / s[0] - target;
        if (fabs(diff) <= kEntropyTol || evals >= kMaxEvals) break;
        if (diff > 0.0) {
            lo = beta;
            beta = isinf(hi) ? beta * 2.0 : 0.5 * (lo + hi);
        } else {
            hi = beta;
            beta = 0.5 * (lo + hi);
        }
    }
    float* dst = p + (size_t)i * n;
    for (int j = tid; j < n; j += kBlock) {
        const double d = (double)row[j] - dmin;
        dst[j] = j == i ? 0.f : (float)(exp(-beta * d) / total);
    }
    if (tid == 0) {
        beta_out[i] = beta;
        evals_out[i] = evals;
    }
}

size_t perplexity_lds(int n) { return kRedDoubles * sizeof(double) + (size_t)n * sizeof(float); }

// ---------------------------------------------------------------------------------------------------------------
// Symmetric P

constexpr int kTile = 32;

// Workgroup (x = b, y = a) with a <= b owns tiles (a, b) and (b, a): both go to LDS, then both are written.  No
// element is read after it was overwritten, and P_ij and P_ji are the same f32 sum of the same two numbers.
__global__ __launch_bounds__(kBlock) void symmetrize_kernel(float* p, int n, float two_n) {
    const int ta = blockIdx.y, tb = blockIdx.x;
    if (ta > tb) return;
    __shared__ float sa[kTile][kTile + 1], sb[kTile][kTile + 1];
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const int ra = ta * kTile, rb = tb * kTile;
    for (int r = ty; r < kTile; r += kBlock / kTile) {
        const bool in_a = ra + r < n && rb + tx < n, in_b = rb + r < n && ra + tx < n;
        sa[r][tx] = in_a ? p[(size_t)(ra + r) * n + rb + tx] : 0.f;
        sb[r][tx] = in_b ? p[(size_t)(rb + r) * n + ra + tx] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < kTile; r += kBlock / kTile) {
        if (ra + r < n && rb + tx < n) p[(size_t)(ra + r) * n + rb + tx] = (sa[r][tx] + sb[tx][r]) / two_n;
        if (ta != tb && rb + r < n && ra + tx < n) p[(size_t)(rb + r) * n + ra + tx] = (sb[r][tx] + sa[tx][r]) / two_n;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Forces

constexpr int kChunk = 4096;       // points of y in LDS at a time: 32 KiB
constexpr int kWaveSpan = 256;     // entries of a row a wave takes per turn: four to a lane
constexpr int kMaxWaveRows = 4;    // rows a wave owns at most

// rows a wave owns: enough workgroups for every CU at a small n, fewer stagings of y at a large one
int wave_rows(int n) {
    const int r = n / 2048;
    return r < 1 ? 1 : (r > kMaxWaveRows ? kMaxWaveRows : r);
}

struct PairSums {
    double ax, ay, rx, ry, z, a, b;
};

// the pair (i, j): pv = P_ij, (yix, yiy) = y_i, (yjx, yjy) = y_j; on = j < n and j != i.  Everything in f64: the
// differences of two f32 are exact there, so a term carries the roundings of d2, w and its own products only.
template <bool KL>
__device__ __forceinline__ void add_pair(PairSums& s, float pv, double yix, double yiy, float yjx, float yjy, bool on) {
    const double dx = yix - (double)yjx, dy = yiy - (double)yjy;
    const double d2 = fma(dy, dy, dx * dx);
    const double w = on ? 1.0 / (1.0 + d2) : 0.0;
    const double pd = (double)pv;
    const double pw = pd * w, w2 = w * w;
    s.ax = fma(pw, dx, s.ax);
    s.ay = fma(pw, dy, s.ay);
    s.rx = fma(w2, dx, s.rx);
    s.ry = fma(w2, dy, s.ry);
    s.z += w;
    if (KL) {
        if (on && pv > 0.f) {
            s.a = fma(pd, log(pd), s.a);
            s.b = fma(pd, -log1p(d2), s.b);   // ln w; log1p keeps its digits where the map is small and w is 1 - 1e-8
        }
    }
}

// Wave wv of workgroup g owns rows (4 g + wv) rows_per_wave .. + rows_per_wave - 1.  The workgroup walks y in chunks
// of kChunk points through LDS (zeros past n up to the next multiple of kWaveSpan); inside a chunk the wave takes
// kWaveSpan entries of each of its rows per turn, lane l the four entries 4 l .. 4 l + 3 as one 16-byte load (VEC:
// n is a multiple of 4 and P 16-byte aligned, so every row is) or four 4-byte loads.
template <bool KL, bool VEC>
__global__ __launch_bounds__(kBlock) void forces_kernel(const float* __restrict__ p, const float* __restrict__ y,
                                                        int n, int rows_per_wave, float* __restrict__ attr,
                                                        float* __restrict__ rep, double* __restrict__ z,
                                                        double* __restrict__ kl) {
    __shared__ __attribute__((aligned(16))) float ys[2 * kChunk];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long row0 = ((long long)blockIdx.x * kWaves + wv) * rows_per_wave;

    PairSums s[kMaxWaveRows];
    double yix[kMaxWaveRows], yiy[kMaxWaveRows];
    bool live[kMaxWaveRows];
#pragma unroll
    for (int r = 0; r < kMaxWaveRows; ++r) {
        s[r] = PairSums{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        live[r] = r < rows_per_wave && row0 + r < n;
        yix[r] = live[r] ? (double)y[2 * (row0 + r)] : 0.0;
        yiy[r] = live[r] ? (double)y[2 * (row0 + r) + 1] : 0.0;
    }

    for (int c0 = 0; c0 < n; c0 += kChunk) {
        const int cn = n - c0 < kChunk ? n - c0 : kChunk;                        // points of this chunk
        const int staged = (cn + kWaveSpan - 1) / kWaveSpan * kWaveSpan;          // <= kChunk
        if (c0 != 0) __syncthreads();   // every wave has left the chunk before
        for (int e = tid; e < 2 * staged; e += kBlock) ys[e] = e < 2 * cn ? y[2 * (size_t)c0 + e] : 0.f;
        __syncthreads();
        for (int t = 0; t < cn; t += kWaveSpan) {
            const int jl = t + 4 * lane;                                           // < staged
            const f32x4 ya = *reinterpret_cast<const f32x4*>(ys + 2 * jl);
            const f32x4 yb = *reinterpret_cast<const f32x4*>(ys + 2 * jl + 4);
            f32x4 pv[kMaxWaveRows];
#pragma unroll
            for (int r = 0; r < kMaxWaveRows; ++r) {
                pv[r] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (!live[r]) continue;
                const float* prow = p + (size_t)(row0 + r) * n + c0;
                if (VEC) {
                    if (jl < cn) pv[r] = *reinterpret_cast<const f32x4*>(prow + jl);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (jl + e < cn) pv[r][e] = prow[jl + e];
                }
            }
#pragma unroll
            for (int r = 0; r < kMaxWaveRows; ++r) {
                if (!live[r]) continue;
                const long long j = (long long)c0 + jl, i = row0 + r;
                add_pair<KL>(s[r], pv[r].x, yix[r], yiy[r], ya.x, ya.y, jl + 0 < cn && j + 0 != i);
                add_pair<KL>(s[r], pv[r].y, yix[r], yiy[r], ya.z, ya.w, jl + 1 < cn && j + 1 != i);
                add_pair<KL>(s[r], pv[r].z, yix[r], yiy[r], yb.x, yb.y, jl + 2 < cn && j + 2 != i);
                add_pair<KL>(s[r], pv[r].w, yix[r], yiy[r], yb.z, yb.w, jl + 3 < cn && j + 3 != i);
            }
        }
    }

#pragma unroll
    for (int r = 0; r < kMaxWaveRows; ++r) {
        if (!live[r]) continue;   // uniform over the wave
        const double ax = lf::wave_sum(s[r].ax), ay = lf::wave_sum(s[r].ay);
        const double rx = lf::wave_sum(s[r].rx), ry = lf::wave_sum(s[r].ry);
        const double zz = lf::wave_sum(s[r].z);
        double ka = 0.0, kb = 0.0;
        if (KL) {
            ka = lf::wave_sum(s[r].a);
            kb = lf::wave_sum(s[r].b);
        }
        if (lane == 0) {
            const size_t i = (size_t)(row0 + r);
            attr[2 * i] = (float)ax;   // the one f32 rounding of each sum
            attr[2 * i + 1] = (float)ay;
            rep[2 * i] = (float)rx;
            rep[2 * i + 1] = (float)ry;
            z[i] = zz;
            if (KL) {
                kl[2 * i] = ka;
                kl[2 * i + 1] = kb;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Step

constexpr int kStepBlock = 1024;
constexpr int kStepWaves = kStepBlock / 64;

// sums of K doubles over the workgroup of 1024, the same bits in every thread: the 16 wave partials from the left
// (red: K * 16 + K doubles of LDS)
template <int K>
__device__ __forceinline__ void step_sum_all(double (&v)[K], double* red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = lf::wave_sum(v[k]);
        if (lane == 0) red[k * kStepWaves + wid] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double t = red[k * kStepWaves];
            for (int w = 1; w < kStepWaves; ++w) t += red[k * kStepWaves + w];
            red[K * kStepWaves + k] = t;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = red[K * kStepWaves + k];
}

__global__ __launch_bounds__(kStepBlock) void step_kernel(float* __restrict__ y, float* __restrict__ vel,
                                                          float* __restrict__ gain, const float* __restrict__ attr,
                                                          const float* __restrict__ rep, const double* __restrict__ z,
                                                          int n, double ex, double eta, double mu,
                                                          const double* __restrict__ kl, double sum_p,
                                                          double* __restrict__ kl_out) {
    __shared__ double red_a[3 * kStepWaves + 3], red_b[2 * kStepWaves + 2];
    const int tid = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += kStepBlock) {
        s[0] += z[i];
        if (kl != nullptr) {
            s[1] += kl[2 * i];
            s[2] += kl[2 * i + 1];
        }
    }
    step_sum_all<3>(s, red_a);
    const double zsum = s[0];
    if (kl != nullptr && tid == 0) kl_out[0] = s[1] - s[2] + log(zsum) * sum_p;

    double m[2] = {0.0, 0.0};
    for (int i = tid; i < n; i += kStepBlock) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int e = 2 * i + c;
            const double g = 4.0 * (ex * (double)attr[e] - (double)rep[e] / zsum);
            const float v0 = vel[e];
            float gn = gain[e];
            gn = ((g > 0.0) != (v0 > 0.f)) ? gn + 0.2f : gn * 0.8f;
            gn = fmaxf(gn, 0.01f);
            const float v1 = (float)(mu * (double)v0 - eta * (double)gn * g);
            gain[e] = gn;
            vel[e] = v1;
            m[c] += (double)y[e] + (double)v1;
        }
    }
    step_sum_all<2>(m, red_b);
    const double mean[2] = {m[0] / (double)n, m[1] / (double)n};
    for (int i = tid; i < n; i += kStepBlock) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int e = 2 * i + c;
            y[e] = (float)((double)y[e] + (double)vel[e] - mean[c]);   // vel[e]: this thread's own store above
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The chart's marks

constexpr int kMaxRadius = 64;

// thread g: offset g % side^2 of mark g / side^2, side = 2 r + 1
__global__ __launch_bounds__(kBlock) void scatter_own_kernel(const int32_t* __restrict__ xy,
                                                             const int32_t* __restrict__ colour, long long total,
                                                             int radius, int colours, int h, int w,
                                                             int32_t* __restrict__ owner) {
    const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (g >= total) return;
    const int side = 2 * radius + 1;
    const int k = (int)(g / (side * side)), o = (int)(g - (long long)k * (side * side));
    const int dy = o / side - radius, dx = o - (o / side) * side - radius;
    if (dx * dx + dy * dy > radius * radius) return;
    const int c = colour[k];
    if (c < 0 || c >= colours) return;
    const long long px = (long long)xy[2 * k] + dx, py = (long long)xy[2 * k + 1] + dy;
    if (px < 0 || px >= w || py < 0 || py >= h) return;
    atomicMax(owner + (size_t)py * w + (size_t)px, k + 1);
}

__global__ __launch_bounds__(kBlock) void scatter_paint_kernel(const int32_t* __restrict__ owner,
                                                               const int32_t* __restrict__ colour,
                                                               const uint8_t* __restrict__ palette, size_t pixels,
                                                               uint8_t* __restrict__ img) {
    const size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= pixels) return;
    const int k = owner[g];
    if (k <= 0) return;
    const uint8_t* rgb = palette + 3 * (size_t)colour[k - 1];   // an owner's colour lies inside the palette
    img[3 * g] = rgb[0];
    img[3 * g + 1] = rgb[1];
    img[3 * g + 2] = rgb[2];
}

bool aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

}  // namespace

extern "C" {

int lf_tsne_max_points(void) { return kMaxPoints; }

int lf_tsne_perplexity_f32(const float* d2, int n, double perplexity, float* p, double* beta, int32_t* evals,
                           lf_stream_t stream) {
    LF_REQUIRE(d2 && p && beta && evals, "lf_tsne_perplexity: null buffer");
    LF_REQUIRE(n >= 2 && n <= kMaxPoints, "lf_tsne_perplexity: n=%d (2..%d)", n, kMaxPoints);
    LF_REQUIRE(isfinite(perplexity) && perplexity >= 1.0, "lf_tsne_perplexity: perplexity=%g (finite, >= 1)",
               perplexity);
    static const bool lds_ok =
        hipFuncSetAttribute(reinterpret_cast<const void*>(perplexity_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)perplexity_lds(kMaxPoints)) == hipSuccess;
    LF_REQUIRE(lds_ok, "lf_tsne_perplexity: the device refused %zu bytes of LDS per workgroup",
               perplexity_lds(kMaxPoints));
    perplexity_kernel<<<(unsigned)n, kBlock, perplexity_lds(n), lf::as_stream(stream)>>>(d2, n, log(perplexity), p,
                                                                                         beta, evals);
    return lf::check_launch("lf_tsne_perplexity");
}

int lf_tsne_symmetrize_f32(float* p, int n, lf_stream_t stream) {
    LF_REQUIRE(p, "lf_tsne_symmetrize: null buffer");
    LF_REQUIRE(n >= 1 && n <= kMaxPoints, "lf_tsne_symmetrize: n=%d (1..%d)", n, kMaxPoints);
    const unsigned tiles = (unsigned)((n + kTile - 1) / kTile);
    symmetrize_kernel<<<dim3(tiles, tiles), kBlock, 0, lf::as_stream(stream)>>>(p, n, (float)(2 * n));
    return lf::check_launch("lf_tsne_symmetrize");
}

int lf_tsne_forces_f32(const float* p, const float* y, int n, float* attr, float* rep, double* z, double* kl,
                       lf_stream_t stream) {
    LF_REQUIRE(p && y && attr && rep && z, "lf_tsne_forces: null buffer");
    LF_REQUIRE(n >= 2 && n <= kMaxPoints, "lf_tsne_forces: n=%d (2..%d)", n, kMaxPoints);
    LF_REQUIRE(aligned16(p) && aligned16(y), "lf_tsne_forces: p and y must be 16-byte aligned");
    const int rows = wave_rows(n);
    const unsigned grid = (unsigned)((n + kWaves * rows - 1) / (kWaves * rows));
    hipStream_t s = lf::as_stream(stream);
    const bool vec = n % 4 == 0;
    if (kl != nullptr) {
        if (vec)
            forces_kernel<true, true><<<grid, kBlock, 0, s>>>(p, y, n, rows, attr, rep, z, kl);
        else
            forces_kernel<true, false><<<grid, kBlock, 0, s>>>(p, y, n, rows, attr, rep, z, kl);
    } else {
        if (vec)
            forces_kernel<false, true><<<grid, kBlock, 0, s>>>(p, y, n, rows, attr, rep, z, kl);
        else
            forces_kernel<false, false><<<grid, kBlock, 0, s>>>(p, y, n, rows, attr, rep, z, kl);
    }
    return lf::check_launch("lf_tsne_forces");
}

int lf_tsne_step_f32(float* y, float* vel, float* gain, const float* attr, const float* rep, const double* z, int n,
                     double exaggeration, double eta, double momentum, const double* kl, double sum_p,
                     double* kl_out, lf_stream_t stream) {
    LF_REQUIRE(y && vel && gain && attr && rep && z, "lf_tsne_step: null buffer");
    LF_REQUIRE(n >= 2 && n <= kMaxPoints, "lf_tsne_step: n=%d (2..%d)", n, kMaxPoints);
    LF_REQUIRE(isfinite(exaggeration) && isfinite(eta) && isfinite(momentum) && isfinite(sum_p),
               "lf_tsne_step: exaggeration=%g eta=%g momentum=%g sum_p=%g must be finite", exaggeration, eta,
               momentum, sum_p);
    LF_REQUIRE((kl == nullptr) == (kl_out == nullptr), "lf_tsne_step: kl and kl_out go together");
    step_kernel<<<1, kStepBlock, 0, lf::as_stream(stream)>>>(y, vel, gain, attr, rep, z, n, exaggeration, eta,
                                                             momentum, kl, sum_p, kl_out);
    return lf::check_launch("lf_tsne_step");
}

int lf_scatter_points_u8(const int32_t* xy, const int32_t* colour, int m, int radius, const uint8_t* palette,
                         int colours, uint8_t* img, int h, int w, int32_t* owner, lf_stream_t stream) {
    LF_REQUIRE(xy && colour && palette && img && owner, "lf_scatter_points: null buffer");
    LF_REQUIRE(m >= 1 && m <= (1 << 20), "lf_scatter_points: m=%d (1..%d)", m, 1 << 20);
    LF_REQUIRE(radius >= 0 && radius <= kMaxRadius, "lf_scatter_points: radius=%d (0..%d)", radius, kMaxRadius);
    LF_REQUIRE(colours >= 1 && h >= 1 && w >= 1 && (long long)h * w <= (1ll << 28),
               "lf_scatter_points: colours=%d h=%d w=%d (each >= 1, h * w <= 2^28)", colours, h, w);
    hipStream_t s = lf::as_stream(stream);
    const size_t pixels = (size_t)h * w;
    if (hipMemsetAsync(owner, 0, pixels * sizeof(int32_t), s) != hipSuccess) {
        lf::set_error("lf_scatter_points: the owner plane could not be cleared");
        return LF_ERR_LAUNCH;
    }
    const long long side = 2 * radius + 1, total = (long long)m * side * side;
    scatter_own_kernel<<<(unsigned)((total + kBlock - 1) / kBlock), kBlock, 0, s>>>(xy, colour, total, radius,
                                                                                    colours, h, w, owner);
    scatter_paint_kernel<<<(unsigned)((pixels + kBlock - 1) / kBlock), kBlock, 0, s>>>(owner, colour, palette,
                                                                                       pixels, img);
    return lf::check_launch("lf_scatter_points");
}

}  // extern "C"
