// libleafhip — split conformal prediction: the conformity score of each row's true label (lf_conformal_scores) and
// the prediction sets at given thresholds, with their coverage counters (lf_conformal_sets).  The rule is stated in
// include/leafhip.h ("Conformal") and DESIGN.md ("Prediction sets").
//
// Every score is float64, every operation rounded on its own (built without FMA contraction: Makefile, NO_CONTRACT),
// and the cumulative mass is added in rank order, one class after the other: tests/conformal_ref.py does the same
// operations in the same order, so the two agree in every bit and `score <= qhat` never falls on the other side.
//
// One wave per row, c <= 256: lane l owns the classes l, l + 64, l + 128, l + 192.  The row goes to the wave's LDS
// once (a NaN as 0); every lane counts the classes that stand before each of its own (the rank: c broadcast reads),
// scatters its values to their ranks, and then walks the sorted row from the top, adding as it goes and keeping the
// sum at the ranks of its own classes.  The walk is a chain of c dependent additions: that is the rule, not an
// oversight (a tree would round differently).
#include <math.h>

#include "lf_common.h"
#include "lf_wave.h"

namespace {

using lf::wave_sum_all;

constexpr int kWaves = 4;
constexpr int kBlock = 64 * kWaves;
constexpr int kMaxClasses = 256;               // nn.CONFORMAL_MAX_CLASSES
constexpr int kSlots = kMaxClasses / 64;       // classes per lane
constexpr int kMaxGroups = 2048;               // workgroups of a launch: 8,192 waves (nn.CONFORMAL_WAVES)
constexpr int kGlobals = 4;                    // rows, skipped, covered, size_sum
constexpr int kPerClass = 3;                   // rows, covered, size_sum

typedef unsigned long long u64;

struct Rule {
    int kind;       // LF_CONFORMAL_LAC / _APS / _RAPS
    double lambda;
    int kreg;
};

// One row in a wave's registers: slot t of lane l is class l + 64 t (valid while < c).
struct Row {
    float p[kSlots];
    int r[kSlots];
    double m[kSlots];
};

// k stands before j
__device__ __forceinline__ bool before(float pk, int k, float pj, int j) { return pk > pj || (pk == pj && k < j); }

// Reads row `src` (null: the wave has no row in this round; it still meets the barriers), fills p and r, and walks
// the ranks below limit(row), a count that is the same in every lane (limit sees p and r): m of every class of such
// a rank is filled, and the mass past the last of them is returned.  raw / sorted: the wave's own LDS.  Every wave
// of the workgroup calls this the same number of times: the two barriers are workgroup barriers.
template <typename Limit>
__device__ __forceinline__ double rank_row(const float* src, int c, int lane, float* raw, float* sorted, Row& row,
                                           Limit limit) {
#pragma unroll
    for (int t = 0; t < kSlots; ++t) {
        const int j = lane + 64 * t;
        float v = 0.f;
        if (src != nullptr && j < c) v = src[j];
        row.p[t] = v != v ? 0.f : v;           // a NaN reads as 0
        row.r[t] = 0;
        row.m[t] = 0.0;
        if (j < c) raw[j] = row.p[t];
    }
    __syncthreads();
    for (int k = 0; k < c; ++k) {
        const float pk = raw[k];
#pragma unroll
        for (int t = 0; t < kSlots; ++t) row.r[t] += before(pk, k, row.p[t], lane + 64 * t) ? 1 : 0;
    }
#pragma unroll
    for (int t = 0; t < kSlots; ++t)
        if (lane + 64 * t < c) sorted[row.r[t]] = row.p[t];    // a total order: the ranks are 0 .. c - 1, once each
    __syncthreads();
    const int stop = limit(row);
    double acc = 0.0;
    for (int r = 0; r < stop; ++r) {
#pragma unroll
        for (int t = 0; t < kSlots; ++t)
            if (row.r[t] == r) row.m[t] = acc;
        acc += (double)sorted[r];
    }
    return acc;
}

// the score of a class with probability p at rank r, m the mass before it
__device__ __forceinline__ double score_of(float p32, double m, int r, double u, const Rule& rule) {
    const double p = (double)p32;
    if (rule.kind == LF_CONFORMAL_LAC) return 1.0 - p;
    double s = m + u * p;
    if (rule.kind == LF_CONFORMAL_RAPS) {
        const int over = r + 1 - rule.kreg;
        s = s + rule.lambda * (double)(over > 0 ? over : 0);
    }
    return s;
}

__global__ __launch_bounds__(kBlock) void conformal_scores_kernel(const float* __restrict__ probs,
                                                                  const int32_t* __restrict__ labels,
                                                                  const float* __restrict__ u, int n, int c, Rule rule,
                                                                  double* __restrict__ score,
                                                                  int32_t* __restrict__ rank) {
    __shared__ float raw[kWaves][kMaxClasses];
    __shared__ float sorted[kWaves][kMaxClasses];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t step = (size_t)gridDim.x * kWaves;
    for (size_t base = (size_t)blockIdx.x * kWaves; base < (size_t)n; base += step) {   // uniform over the workgroup
        const size_t i = base + wave;
        const bool live = i < (size_t)n;
        const int y = live ? labels[i] : -1;                     // the same in every lane of the wave
        const bool known = (unsigned)y < (unsigned)c;
        Row row;
        int ry = 0;
        // the label's rank is the sum of its owner's count (the other lanes add 0); the walk ends there, so what it
        // returns is the mass before the label.  LAC needs no walk.
        const double my = rank_row(live ? probs + i * c : nullptr, c, lane, raw[wave], sorted[wave], row,
                                   [&](const Row& rw) {
                                       int mine = 0;
#pragma unroll
                                       for (int t = 0; t < kSlots; ++t)
                                           if (known && lane + 64 * t == y) mine = rw.r[t];
                                       ry = wave_sum_all(mine);
                                       return known && rule.kind != LF_CONFORMAL_LAC ? ry : 0;
                                   });
        if (!live || lane != 0) continue;
        if (known) {
            score[i] = score_of(raw[wave][y], my, ry, u != nullptr ? (double)u[i] : 1.0, rule);
            rank[i] = ry;
        } else {
            score[i] = (double)NAN;
            rank[i] = -1;
        }
    }
}

// tab: {rows, skipped, covered, size_sum}, size_hist[c + 1], per class {rows, covered, size_sum}: counted in the
// workgroup's LDS by lane 0 of each wave, then added to `stats` with one integer atomic per entry that is not zero.
__global__ __launch_bounds__(kBlock) void conformal_sets_kernel(const float* __restrict__ probs,
                                                                const float* __restrict__ u,
                                                                const double* __restrict__ qhat, int n, int c,
                                                                Rule rule, int force_top,
                                                                const int32_t* __restrict__ labels,
                                                                uint8_t* __restrict__ member,
                                                                int32_t* __restrict__ size, u64* __restrict__ stats) {
    __shared__ float raw[kWaves][kMaxClasses];
    __shared__ float sorted[kWaves][kMaxClasses];
    __shared__ u64 tab[kGlobals + kMaxClasses + 1 + kPerClass * kMaxClasses];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int entries = kGlobals + c + 1 + kPerClass * c;
    if (stats != nullptr) {
        for (int e = threadIdx.x; e < entries; e += kBlock) tab[e] = 0;   // rank_row's first barrier follows
    }
    double q[kSlots];
#pragma unroll
    for (int t = 0; t < kSlots; ++t) q[t] = lane + 64 * t < c ? qhat[lane + 64 * t] : 0.0;
    const size_t step = (size_t)gridDim.x * kWaves;
    for (size_t base = (size_t)blockIdx.x * kWaves; base < (size_t)n; base += step) {   // uniform over the workgroup
        const size_t i = base + wave;
        const bool live = i < (size_t)n;
        Row row;
        rank_row(live ? probs + i * c : nullptr, c, lane, raw[wave], sorted[wave], row,
                 [&](const Row&) { return rule.kind != LF_CONFORMAL_LAC ? c : 0; });
        if (!live) continue;
        const double ui = u != nullptr ? (double)u[i] : 1.0;
        const int y = labels != nullptr ? labels[i] : -1;
        int count = 0, hit = 0;
#pragma unroll
        for (int t = 0; t < kSlots; ++t) {
            const int j = lane + 64 * t;
            if (j < c) {
                const bool in =
                    score_of(row.p[t], row.m[t], row.r[t], ui, rule) <= q[t] || (force_top && row.r[t] == 0);
                member[i * c + j] = in ? 1 : 0;
                count += in;
                hit += in && j == y;
            }
        }
        count = wave_sum_all(count);
        hit = wave_sum_all(hit);
        if (lane == 0) {
            size[i] = count;
            if (stats != nullptr) {
                if ((unsigned)y < (unsigned)c) {
                    u64* cls = tab + kGlobals + c + 1 + kPerClass * y;
                    atomicAdd(tab + 0, (u64)1);
                    atomicAdd(tab + 2, (u64)hit);
                    atomicAdd(tab + 3, (u64)count);
                    atomicAdd(tab + kGlobals + count, (u64)1);
                    atomicAdd(cls + 0, (u64)1);
                    atomicAdd(cls + 1, (u64)hit);
                    atomicAdd(cls + 2, (u64)count);
                } else {
                    atomicAdd(tab + 1, (u64)1);
                }
            }
        }
    }
    if (stats != nullptr) {
        __syncthreads();
        for (int e = threadIdx.x; e < entries; e += kBlock)
            if (tab[e] != 0) atomicAdd(stats + e, tab[e]);
    }
}

unsigned conformal_groups(int n) {
    const int g = (n + kWaves - 1) / kWaves;
    return (unsigned)(g < kMaxGroups ? g : kMaxGroups);
}

// what both calls ask of their shared arguments; says what is wrong
bool rule_ok(const char* who, int n, int c, int kind, double lambda, int kreg) {
    if (!(n > 0 && c >= 1 && c <= kMaxClasses))
        lf::set_error("%s: bad dims n=%d c=%d (c in 1..%d)", who, n, c, kMaxClasses);
    else if (kind != LF_CONFORMAL_LAC && kind != LF_CONFORMAL_APS && kind != LF_CONFORMAL_RAPS)
        lf::set_error("%s: kind=%d is none of lac (0), aps (1), raps (2)", who, kind);
    else if (!(isfinite(lambda) && lambda >= 0.0))
        lf::set_error("%s: lambda is not finite and >= 0", who);
    else if (kreg < 0)
        lf::set_error("%s: kreg=%d is negative", who, kreg);
    else
        return true;
    return false;
}

}  // namespace

extern "C" {

int lf_conformal_scores(const float* probs, const int32_t* labels, const float* u, int n, int c, int kind,
                        double lambda, int kreg, double* score, int32_t* rank, lf_stream_t stream) {
    LF_REQUIRE(probs && labels && score && rank, "lf_conformal_scores: null buffer");
    if (!rule_ok("lf_conformal_scores", n, c, kind, lambda, kreg)) return LF_ERR_INVALID;
    const Rule rule = {kind, lambda, kreg};
    conformal_scores_kernel<<<conformal_groups(n), kBlock, 0, lf::as_stream(stream)>>>(probs, labels, u, n, c, rule,
                                                                                      score, rank);
    return lf::check_launch("lf_conformal_scores");
}

int lf_conformal_sets(const float* probs, const float* u, const double* qhat, int n, int c, int kind, double lambda,
                      int kreg, int force_top, const int32_t* labels, uint8_t* member, int32_t* size,
                      long long* stats, lf_stream_t stream) {
    LF_REQUIRE(probs && qhat && member && size, "lf_conformal_sets: null buffer");
    if (!rule_ok("lf_conformal_sets", n, c, kind, lambda, kreg)) return LF_ERR_INVALID;
    LF_REQUIRE(stats == nullptr || labels != nullptr, "lf_conformal_sets: stats without labels");
    LF_REQUIRE(((uintptr_t)stats & 7) == 0 && ((uintptr_t)qhat & 7) == 0,
               "lf_conformal_sets: qhat and stats must be 8-byte aligned");
    hipStream_t s = lf::as_stream(stream);
    const size_t entries = (size_t)kGlobals + c + 1 + (size_t)kPerClass * c;
    if (stats != nullptr && hipMemsetAsync(stats, 0, entries * sizeof(long long), s) != hipSuccess) {
        lf::set_error("lf_conformal_sets: clearing the counters failed");
        return LF_ERR_LAUNCH;
    }
    const Rule rule = {kind, lambda, kreg};
    conformal_sets_kernel<<<conformal_groups(n), kBlock, 0, s>>>(probs, u, qhat, n, c, rule, force_top != 0, labels,
                                                                member, size, reinterpret_cast<u64*>(stats));
    return lf::check_launch("lf_conformal_sets");
}

}  // extern "C"
