// libleafhip — novelty score: the float64 sums a Mahalanobis fit needs from pooled feature rows (lf_feat_moments),
// and the squared distance of feature rows to the nearest whitened class mean (lf_maha_score_f32).  The rules are
// stated in include/leafhip.h and DESIGN.md ("Novelty score").
//
// No float goes through an atomic: every output element has one owner, which adds the rows in row order, so the same
// calls give the same bits.  A product of two f32 values is exact in f64 (48 bits), so only additions round in
// lf_feat_moments and FMA contraction cannot change a bit of it; lf_maha_score_f32 states each fmaf itself.
#include <limits.h>
#include <math.h>

#include "lf_common.h"
#include "lf_wave.h"

namespace {

using lf::f32x16;
using lf::f32x4;
using lf::kHeadMaxClasses;
using lf::take_smaller;

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxDim = 256;
constexpr int kDimStep = 16;
constexpr int kBlock = 256;

// ---- lf_feat_moments ---------------------------------------------------------------------------------------------

// One wave per upper 16x16 tile (ti <= tj) of the Gram matrix, four rows of feat to a v_mfma_f64_16x16x4_f64:
//   A[i][k] = f[r0 + k][16 ti + i]  in lane 16 k + i,   B[k][j] = f[r0 + k][16 tj + j]  in lane 16 k + j
// (the operand maps of the f32 16x16x4 form), so D[i][j] += sum_k A[i][k] B[k][j] walks the rows in row order.  A
// row past n, or one whose label lies outside [0, c), enters as zeros.  The f64 C/D map is NOT the f32 one: register
// `reg` of lane l holds D[row = (l >> 4) + 4 reg][col = l & 15].  The tile is added to gram and, off the diagonal,
// its transpose to the mirrored tile: every element of gram has one owner.
__global__ __launch_bounds__(64) void gram_kernel(const float* __restrict__ feat, const int32_t* __restrict__ labels,
                                                  int n, int d, int c, double* __restrict__ gram) {
    const int tiles = d / 16;
    int ti = 0, rest = blockIdx.x;   // upper tiles in row-major order: row ti holds tiles - ti of them
    while (rest >= tiles - ti) {
        rest -= tiles - ti;
        ++ti;
    }
    const int tj = ti + rest;
    const int lane = threadIdx.x, k = lane >> 4, e = lane & 15;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    constexpr int kAhead = 4;   // instructions whose operands are loaded together: the loads overlap, the order stays
    for (int r0 = 0; r0 < n; r0 += 4 * kAhead) {
        double a[kAhead], b[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int r = r0 + 4 * u + k;
            a[u] = b[u] = 0.0;
            if (r < n && (unsigned)labels[r] < (unsigned)c) {
                const float* row = feat + (size_t)r * d;
                a[u] = (double)row[16 * ti + e];
                b[u] = (double)row[16 * tj + e];
            }
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int i = 16 * ti + k + 4 * reg, j = 16 * tj + e;
        gram[(size_t)i * d + j] += acc[reg];
        if (ti != tj) gram[(size_t)j * d + i] += acc[reg];
    }
}

// Workgroup `cls` < c: thread j < d owns sum[cls][j] and adds the rows of that class in row order; thread 0 counts
// them.  Workgroup c counts the rows whose label lies outside [0, c) (integers: any order gives the same count).
__global__ __launch_bounds__(kBlock) void class_sums_kernel(const float* __restrict__ feat,
                                                            const int32_t* __restrict__ labels, int n, int d, int c,
                                                            long long* __restrict__ count,
                                                            long long* __restrict__ skipped,
                                                            double* __restrict__ sum) {
    const int cls = blockIdx.x, j = threadIdx.x;
    if (cls == c) {
        long long bad = 0;
        for (int r = j; r < n; r += kBlock) bad += (unsigned)labels[r] >= (unsigned)c;
        bad = lf::wave_sum(bad);
        if ((j & 63) == 0 && bad != 0)
            atomicAdd(reinterpret_cast<unsigned long long*>(skipped), (unsigned long long)bad);
        return;
    }
    double s = 0.0;
    long long rows = 0;
    for (int r = 0; r < n; ++r) {
        if (labels[r] != cls) continue;   // uniform over the workgroup
        ++rows;
        if (j < d) s += (double)feat[(size_t)r * d + j];
    }
    if (rows == 0) return;
    if (j < d) sum[(size_t)cls * d + j] += s;
    if (j == 0) count[cls] += rows;
}

// ---- lf_maha_score_f32 -------------------------------------------------------------------------------------------

constexpr int kRows = 32;             // rows of feat to a workgroup
constexpr int kGroups = kBlock / kRows;   // threads to a row in the distance pass: thread t takes classes t / 32 + 8 m
constexpr int kPitchPad = 1;          // an odd LDS pitch: the 32 rows of a column lie in 32 banks

// One workgroup per 32 rows of feat, three passes over one LDS tile t[32][d + 1]:
//  1. t[i][j] = feat[r0 + i][j] - mu0[j]  (one f32 subtraction; rows past n are zeros).
//  2. z = t W^T on v_mfma_f32_32x32x2_f32, wave w taking the 32-column tiles w, w + 4 of z.  Lane l (i = l & 31,
//     h = l >> 5) holds A[i][h] = t[i][h d/2 + s] and B[h][q] = W[32 tile + q][h d/2 + s] in step s < d/2 (q = l & 31),
//     so a lane reads its row of W contiguously, 16 bytes at a time.  The MFMA is an f32 fmaf chain in k order: z[i][q]
//     adds its d products in the order j = 0, d/2, 1, d/2 + 1, ...  A column of z past d (d = 48: half of the last
//     tile) takes zeros for B and is not kept.  C/D: register reg of lane l holds row (reg & 3) + 8 (reg >> 2) + 4 h,
//     column q.  After a barrier (every wave has read t) z replaces t.
//  3. thread t (row i = t & 31, group t >> 5) owns the pairs (i, cls = t / 32 + 8 m): d2 = fmaf chain over k = 0 ..
//     d - 1 of (z[i][k] - M[cls][k])^2 from 0; a non-finite d2 is +inf.  The smaller of (d2, cls) pairs, the lower
//     class on a tie, first over the thread's classes, then over the row's 8 groups in LDS.
__global__ __launch_bounds__(kBlock) void maha_score_kernel(const float* __restrict__ feat,
                                                            const float* __restrict__ mu0,
                                                            const float* __restrict__ w, const float* __restrict__ m,
                                                            int n, int d, int c, float* __restrict__ d2,
                                                            float* __restrict__ score, int32_t* __restrict__ nearest) {
    __shared__ float tile[kRows * (kMaxDim + kPitchPad)];
    __shared__ float red_v[kGroups][kRows];
    __shared__ int red_i[kGroups][kRows];
    const int pitch = d + kPitchPad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r0 = (size_t)blockIdx.x * kRows;

    for (int e = tid; e < kRows * d; e += kBlock) {
        const int i = e / d, j = e - i * d;
        tile[i * pitch + j] = r0 + i < (size_t)n ? feat[(r0 + i) * d + j] - mu0[j] : 0.f;
    }
    __syncthreads();

    const int q = lane & 31, h = lane >> 5, half = d / 2;
    const int col_tiles = (d + 31) / 32;
    f32x16 acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int ct = wave + 4 * u;
        acc[u] = f32x16{};
        if (ct >= col_tiles) continue;   // uniform over the wave
        const int col = 32 * ct + q;
        const bool live = col < d;
        const float* wrow = w + (size_t)(live ? col : 0) * d + h * half;
        const float* trow = tile + q * pitch + h * half;
        for (int s = 0; s < half; s += 4) {   // half is a multiple of 8
            f32x4 b = *reinterpret_cast<const f32x4*>(wrow + s);
            if (!live) b = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int x = 0; x < 4; ++x)
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(trow[s + x], b[x], acc[u], 0, 0, 0);
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int col = 32 * (wave + 4 * u) + q;
        if (col >= d) continue;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) tile[((reg & 3) + 8 * (reg >> 2) + 4 * h) * pitch + col] = acc[u][reg];
    }
    __syncthreads();

    const int i = tid & 31, grp = tid >> 5;
    const bool row_ok = r0 + i < (size_t)n;
    const float* zrow = tile + i * pitch;
    float bv = INFINITY;
    int bi = INT_MAX;
    for (int cls = grp; cls < c; cls += kGroups) {
        const float* mrow = m + (size_t)cls * d;
        float v = 0.f;
        for (int k = 0; k < d; ++k) {
            const float t = zrow[k] - mrow[k];
            v = fmaf(t, t, v);
        }
        if (!isfinite(v)) v = INFINITY;
        if (d2 != nullptr && row_ok) d2[(r0 + i) * c + cls] = v;
        take_smaller(bv, bi, v, cls);
    }
    red_v[grp][i] = bv;
    red_i[grp][i] = bi;
    __syncthreads();
    if (tid < kRows && row_ok) {
        for (int g = 1; g < kGroups; ++g) take_smaller(bv, bi, red_v[g][i], red_i[g][i]);
        score[r0 + i] = bv;
        nearest[r0 + i] = (unsigned)bi < (unsigned)c ? bi : 0;
    }
}

bool novelty_dims_ok(int n, int d, int c) {
    return n > 0 && d >= kDimStep && d <= kMaxDim && d % kDimStep == 0 && c >= 1 && c <= kHeadMaxClasses;
}

}  // namespace

extern "C" {

int lf_feat_moments(const float* feat, const int32_t* labels, int n, int d, int c, long long* count,
                    long long* skipped, double* sum, double* gram, lf_stream_t stream) {
    LF_REQUIRE(feat && labels && count && skipped && sum && gram, "lf_feat_moments: null buffer");
    LF_REQUIRE(novelty_dims_ok(n, d, c),
               "lf_feat_moments: bad dims n=%d d=%d c=%d (n > 0, d a multiple of %d in %d..%d, c in 1..%d)", n, d, c,
               kDimStep, kDimStep, kMaxDim, kHeadMaxClasses);
    LF_REQUIRE((((uintptr_t)count | (uintptr_t)skipped | (uintptr_t)sum | (uintptr_t)gram) & 7) == 0,
               "lf_feat_moments: the accumulators must be 8-byte aligned");
    hipStream_t s = lf::as_stream(stream);
    const int tiles = d / 16;
    gram_kernel<<<(unsigned)(tiles * (tiles + 1) / 2), 64, 0, s>>>(feat, labels, n, d, c, gram);
    class_sums_kernel<<<(unsigned)(c + 1), kBlock, 0, s>>>(feat, labels, n, d, c, count, skipped, sum);
    return lf::check_launch("lf_feat_moments");
}

int lf_maha_score_f32(const float* feat, const float* mu0, const float* w, const float* m, int n, int d, int c,
                      float* d2, float* score, int32_t* nearest, lf_stream_t stream) {
    LF_REQUIRE(feat && mu0 && w && m && score && nearest, "lf_maha_score: null buffer");
    LF_REQUIRE(novelty_dims_ok(n, d, c),
               "lf_maha_score: bad dims n=%d d=%d c=%d (n > 0, d a multiple of %d in %d..%d, c in 1..%d)", n, d, c,
               kDimStep, kDimStep, kMaxDim, kHeadMaxClasses);
    LF_REQUIRE(((uintptr_t)w & 15) == 0, "lf_maha_score: w must be 16-byte aligned");
    const unsigned grid = (unsigned)(((size_t)n + kRows - 1) / kRows);
    maha_score_kernel<<<grid, kBlock, 0, lf::as_stream(stream)>>>(feat, mu0, w, m, n, d, c, d2, score, nearest);
    return lf::check_launch("lf_maha_score");
}

}  // extern "C"
