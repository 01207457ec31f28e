// libleafhip — calibration: what a set of probability rows and their labels say about a temperature
// (lf_calib_stats), and the rows at a temperature (lf_calib_apply_f32).  The rules are stated in include/leafhip.h
// and DESIGN.md ("Calibrated confidences").
//
// All per-row arithmetic is float64 and built without FMA contraction (Makefile, NO_CONTRACT), so that every
// operation rounds once, as numpy's do: tests/calib_ref.py is the same arithmetic and the tests bound the difference
// by the rounding of the additions and the 1-ulp exp and log alone.
//
// A row is never staged: z_j = ln max(p_j, FLT_MIN) is taken again from p_j in every pass over the row (one for the
// maximum, two per beta).  The rows come from the L1 after the first pass, and a launch is tens of microseconds
// beside a forward pass of milliseconds; a register or LDS copy of z would have to be sized for 64 classes per lane.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "lf_common.h"
#include "lf_wave.h"

namespace {

using lf::kHeadMaxClasses;
using lf::take_larger;
using lf::wave_sum_all;

constexpr int kWaves = 4;
constexpr int kBlock = 64 * kWaves;
constexpr int kMaxBetas = 8;
constexpr int kMaxBins = 64;
constexpr int kMaxGroups = 256;     // workgroups of a stats launch: one per CU
constexpr int kSums = 5;            // nll, g, h, brier, conf

// the inverse temperatures as a kernel argument: uniform over the launch, read through scalar registers
struct Betas {
    double b[kMaxBetas];
};

// fmaxf returns the other operand for a NaN: a NaN is read as FLT_MIN too
__device__ __forceinline__ double zlog(float p) { return log((double)fmaxf(p, FLT_MIN)); }

// The maximum of the input row and the lowest index that attains it, the same in every lane.  A row of NaNs alone
// has no maximum: index 0, so that what is returned always indexes a class.
__device__ __forceinline__ int row_argmax(const float* row, int c, int lane, float* best) {
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int j = lane; j < c; j += 64) take_larger(bv, bi, row[j], j);
    bi = lf::wave_argmax_all(bv, bi);
    *best = bv;
    return (unsigned)bi < (unsigned)c ? bi : 0;
}

// sum_j exp(beta z_j - m) over the row, m = beta ln(max p): the largest term is exp(0) = 1.  With `zsum` also
// sum_j exp(.) z_j.  The same values in every lane.
__device__ __forceinline__ double row_expsum(const float* row, int c, int lane, double beta, double m,
                                             double* zsum) {
    double s = 0.0, t = 0.0;
    for (int j = lane; j < c; j += 64) {
        const double z = zlog(row[j]);
        const double e = exp(beta * z - m);
        s += e;
        t += e * z;
    }
    if (zsum != nullptr) *zsum = wave_sum_all(t);
    return wave_sum_all(s);
}

// One wave per row at a time; wave w of the launch takes the rows w, w + waves, ...  Lane l owns the classes l,
// l + 64, ...; after the butterflies every lane holds the row's terms, and lane k adds those of beta k to the five
// sums it keeps in registers and to the wave's own bin table in LDS: one lane per beta, in row order.  The waves of
// a workgroup are then added in wave order into the workgroup's partial (ws_d, ws_i), which calib_reduce_kernel
// adds in workgroup order.  No float is ever added by an atomic.
__global__ __launch_bounds__(kBlock) void calib_stats_kernel(const float* __restrict__ probs,
                                                             const int32_t* __restrict__ labels, int n, int c,
                                                             Betas betas, int nk, int bins,
                                                             int32_t* __restrict__ pred_out, int32_t* __restrict__ cm,
                                                             double* __restrict__ ws_d, int32_t* __restrict__ ws_i) {
    __shared__ double sd[kWaves][kMaxBetas * (kSums + kMaxBins)];
    __shared__ int32_t si[kWaves][kMaxBetas * 2 * kMaxBins + 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = kSums + bins;              // doubles per beta: the five sums, then the bins' confidence sums
    const int nd = nk * per, ni = nk * 2 * bins + 2;
    double* md = sd[wave];
    int32_t* mi = si[wave];                    // per beta: bins counts, bins correct counts; then correct, skipped
    for (int e = lane; e < nd; e += 64) md[e] = 0.0;
    for (int e = lane; e < ni; e += 64) mi[e] = 0;
    __syncthreads();

    double a_nll = 0.0, a_g = 0.0, a_h = 0.0, a_brier = 0.0, a_conf = 0.0;   // lane k: those of beta k
    int correct = 0, skipped = 0;                                             // uniform over the wave
    const size_t waves = (size_t)gridDim.x * kWaves;
    for (size_t i = (size_t)blockIdx.x * kWaves + wave; i < (size_t)n; i += waves) {
        const float* row = probs + i * c;
        float pmax;
        const int pred = row_argmax(row, c, lane, &pmax);
        if (pred_out != nullptr && lane == 0) pred_out[i] = pred;
        const int y = labels[i];
        if ((unsigned)y >= (unsigned)c) {
            ++skipped;
            continue;
        }
        const int hit = pred == y;
        correct += hit;
        if (cm != nullptr && lane == 0) atomicAdd(cm + (size_t)y * c + pred, 1);
        const double zmax = zlog(pmax), zy = zlog(row[y]);
#pragma unroll 1
        for (int k = 0; k < nk; ++k) {
            const double beta = betas.b[k];
            const double m = beta * zmax;
            double t;
            const double s = row_expsum(row, c, lane, beta, m, &t);
            const double mu = t / s;
            double hh = 0.0, br = 0.0;
            for (int j = lane; j < c; j += 64) {   // the second pass: about the mean, so that h is never negative
                const double z = zlog(row[j]);
                const double q = exp(beta * z - m) / s;
                const double d = z - mu;
                const double r = q - (j == y ? 1.0 : 0.0);
                hh += q * (d * d);
                br += r * r;
            }
            hh = wave_sum_all(hh);
            br = wave_sum_all(br);
            if (lane == k) {
                const double conf = 1.0 / s;       // max_j q_j: the largest exp is 1
                a_nll += m + log(s) - beta * zy;
                a_g += mu - zy;
                a_h += hh;
                a_brier += br;
                a_conf += conf;
                const int b = min(bins - 1, max(0, (int)(conf * (double)bins)));
                md[k * per + kSums + b] += conf;
                mi[k * 2 * bins + b] += 1;
                mi[k * 2 * bins + bins + b] += hit;
            }
        }
    }
    if (lane < nk) {
        double* mine = md + lane * per;
        mine[0] = a_nll;
        mine[1] = a_g;
        mine[2] = a_h;
        mine[3] = a_brier;
        mine[4] = a_conf;
    }
    if (lane == 0) {
        mi[ni - 2] = correct;
        mi[ni - 1] = skipped;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nd; e += kBlock) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) v += sd[w][e];
        ws_d[(size_t)blockIdx.x * nd + e] = v;
    }
    for (int e = threadIdx.x; e < ni; e += kBlock) {
        int v = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) v += si[w][e];
        ws_i[(size_t)blockIdx.x * ni + e] = v;
    }
}

// one workgroup: entry e of the output is the sum of the workgroups' entries e, in workgroup order
__global__ __launch_bounds__(kBlock) void calib_reduce_kernel(const double* __restrict__ ws_d,
                                                              const int32_t* __restrict__ ws_i, int groups, int nd,
                                                              int ni, double* __restrict__ sums,
                                                              int32_t* __restrict__ counts) {
    for (int e = threadIdx.x; e < nd; e += kBlock) {
        double v = 0.0;
        for (int g = 0; g < groups; ++g) v += ws_d[(size_t)g * nd + e];
        sums[e] = v;
    }
    for (int e = threadIdx.x; e < ni; e += kBlock) {
        int v = 0;
        for (int g = 0; g < groups; ++g) v += ws_i[(size_t)g * ni + e];
        counts[e] = v;
    }
}

// One wave per row.  probs and out carry no __restrict__: out == probs is allowed.  A lane reads the elements l,
// l + 64, ... of its row and no others, and writes them in its last pass, after both reductions: nothing a lane
// writes is read by another.
__global__ __launch_bounds__(kBlock) void calib_apply_kernel(const float* probs, float* out, int n, int c,
                                                             double beta, float* __restrict__ conf,
                                                             int32_t* __restrict__ top) {
    const int lane = threadIdx.x & 63;
    const size_t i = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= (size_t)n) return;
    const float* row = probs + i * c;
    float pmax;
    const int pred = row_argmax(row, c, lane, &pmax);
    const double m = beta * zlog(pmax);
    const double s = row_expsum(row, c, lane, beta, m, nullptr);
    for (int j = lane; j < c; j += 64) out[i * c + j] = (float)(exp(beta * zlog(row[j]) - m) / s);
    if (lane == 0) {
        conf[i] = (float)(1.0 / s);
        top[i] = pred;
    }
}

int stats_groups(int n) {
    const int g = (n + kWaves - 1) / kWaves;
    return g < kMaxGroups ? g : kMaxGroups;
}

bool calib_dims_ok(int n, int c) { return n > 0 && c >= 1 && c <= kHeadMaxClasses; }

}  // namespace

extern "C" {

size_t lf_calib_stats_workspace(int n, int k, int bins) {
    if (n <= 0 || k < 1 || k > kMaxBetas || bins < 1 || bins > kMaxBins) return 0;
    const size_t nd = (size_t)k * (kSums + bins), ni = (size_t)k * 2 * bins + 2;
    return (size_t)stats_groups(n) * (nd * sizeof(double) + ni * sizeof(int32_t));
}

int lf_calib_stats(const float* probs, const int32_t* labels, int n, int c, const double* betas, int k, int bins,
                   double* sums, int32_t* counts, int32_t* pred, int32_t* cm, void* ws, size_t ws_bytes,
                   lf_stream_t stream) {
    LF_REQUIRE(probs && labels && betas && sums && counts && ws, "lf_calib_stats: null buffer");
    LF_REQUIRE(calib_dims_ok(n, c), "lf_calib_stats: bad dims n=%d c=%d (c in 1..%d)", n, c, kHeadMaxClasses);
    LF_REQUIRE(k >= 1 && k <= kMaxBetas, "lf_calib_stats: k=%d inverse temperatures (1..%d)", k, kMaxBetas);
    LF_REQUIRE(bins >= 1 && bins <= kMaxBins, "lf_calib_stats: bins=%d (1..%d)", bins, kMaxBins);
    Betas bt = {};
    for (int j = 0; j < k; ++j) {
        LF_REQUIRE(isfinite(betas[j]) && betas[j] > 0.0, "lf_calib_stats: beta %d is not finite and positive", j);
        bt.b[j] = betas[j];
    }
    LF_REQUIRE(ws_bytes >= lf_calib_stats_workspace(n, k, bins), "lf_calib_stats: workspace of %zu bytes, %zu needed",
               ws_bytes, lf_calib_stats_workspace(n, k, bins));
    LF_REQUIRE(((uintptr_t)ws & 7) == 0, "lf_calib_stats: the workspace must be 8-byte aligned");
    hipStream_t s = lf::as_stream(stream);
    if (cm != nullptr && hipMemsetAsync(cm, 0, (size_t)c * c * sizeof(int32_t), s) != hipSuccess) {
        lf::set_error("lf_calib_stats: clearing the confusion counts failed");
        return LF_ERR_LAUNCH;
    }
    const int groups = stats_groups(n);
    const int nd = k * (kSums + bins), ni = k * 2 * bins + 2;
    double* ws_d = static_cast<double*>(ws);
    int32_t* ws_i = reinterpret_cast<int32_t*>(ws_d + (size_t)groups * nd);
    calib_stats_kernel<<<(unsigned)groups, kBlock, 0, s>>>(probs, labels, n, c, bt, k, bins, pred, cm, ws_d, ws_i);
    calib_reduce_kernel<<<1, kBlock, 0, s>>>(ws_d, ws_i, groups, nd, ni, sums, counts);
    return lf::check_launch("lf_calib_stats");
}

int lf_calib_apply_f32(const float* probs, double beta, float* out, float* conf, int32_t* top, int n, int c,
                       lf_stream_t stream) {
    LF_REQUIRE(probs && out && conf && top, "lf_calib_apply: null buffer");
    LF_REQUIRE(calib_dims_ok(n, c), "lf_calib_apply: bad dims n=%d c=%d (c in 1..%d)", n, c, kHeadMaxClasses);
    LF_REQUIRE(isfinite(beta) && beta > 0.0, "lf_calib_apply: beta is not finite and positive");
    const uintptr_t a = (uintptr_t)probs, b = (uintptr_t)out, bytes = (uintptr_t)n * c * sizeof(float);
    LF_REQUIRE(a == b || a + bytes <= b || b + bytes <= a,
               "lf_calib_apply: out overlaps probs without being probs (in place means out == probs)");
    const unsigned grid = (unsigned)(((size_t)n + kWaves - 1) / kWaves);
    calib_apply_kernel<<<grid, kBlock, 0, lf::as_stream(stream)>>>(probs, out, n, c, beta, conf, top);
    return lf::check_launch("lf_calib_apply");
}

}  // extern "C"
