// libleafhip — exact k-nearest-neighbour search over feature rows (lf_knn_topk_f32): all squared distances between a
// batch of queries and a gallery on the f32 matrix cores, reduced to the k smallest per query without ever writing
// the distance matrix.  The rule is stated in include/leafhip.h and DESIGN.md ("Nearest neighbours").
//
// A candidate is the pair (d2, j).  d2 is never negative and never NaN, so its f32 bits order as an unsigned
// integer, and the pair is held as one 64-bit key: d2's bits above, j below.  Comparing keys IS the total order of
// the rule (smaller d2 first, lower j on equal d2); the fill pair (+inf, -1) is the largest key a pair can have,
// because -1 reads as 0xffffffff.  Every list below is sorted by key, and the sorted list of the k smallest keys of a
// set does not depend on the order in which the set was met: tiling, waves and segments cannot change a bit.  No
// atomics.
#include <math.h>

#include "lf_common.h"

namespace {

using lf::f32x16;
using lf::f32x4;

typedef unsigned long long u64;

constexpr int kMaxDim = 256;
constexpr int kDimStep = 16;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kQueryTile = 64;              // queries to a workgroup: two 32-row A tiles
constexpr int kWaveRows = 64;               // gallery rows to a wave and step: two 32-column B tiles
constexpr int kStepRows = kWaves * kWaveRows;
constexpr int kMaxK = 32;                   // a list is the 32 lanes of a wave half
constexpr int kMaxSegments = 64;            // the merge kernel gives every segment a lane
constexpr int kPitchPad = 1;                // an odd LDS pitch: the 32 query rows of a column lie in 32 banks
constexpr int kFillCUs = 256;               // workgroups wanted before the gallery is cut into segments
constexpr u64 kFill = 0x7F800000FFFFFFFFull;   // (+inf, -1)
constexpr int kDeadRow = -2;
constexpr u64 kSpent = ~0ull;               // above every key: the head of a list that has been read to its end

__device__ __forceinline__ u64 pair_key(float dot, float qn, float gn, int j) {
    float v = fmaf(-2.f, dot, qn + gn);
    v = isfinite(v) ? (v > 0.f ? v : 0.f) : INFINITY;   // -0 becomes +0: the bits order as integers
    return ((u64)__float_as_uint(v) << 32) | (unsigned)j;
}

__device__ __forceinline__ u64 lane_value(u64 v, int src /* uniform */) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

template <int CTRL>
__device__ __forceinline__ u64 dpp_u64(u64 v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xf, 0xf, true);
    return ((u64)hi << 32) | lo;
}
constexpr int kDppWaveShr1 = 0x138;    // lane l reads lane l - 1 of the whole wave
constexpr int kDppQuadXor1 = 0xB1;     // quad_perm [1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;     // quad_perm [2,3,0,1]

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int off) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off, 64);
    return ((u64)hi << 32) | lo;
}

// The two lists a register holds (lane half h: slot c of the list of that half's query row) take the keys of their
// own half that are smaller than their last key, slot k - 1.  Per turn each half takes its lowest passing lane's key:
// every slot keeps its key, takes the candidate, or takes its left neighbour's key (one DPP shift), by two
// comparisons.  The rest are then tested against the new last keys, so a turn is spent only on a key that enters.
__device__ __forceinline__ void insert_passing(u64& slot, u64 key, int k, int c, int h) {
    u64 last = h ? lane_value(slot, 32 + k - 1) : lane_value(slot, k - 1);
    u64 pass = __ballot(key < last);
    while (pass != 0) {
        const unsigned plo = (unsigned)pass, phi = (unsigned)(pass >> 32);
        const int slo = plo != 0 ? __builtin_ctz(plo) : 0, shi = 32 + (phi != 0 ? __builtin_ctz(phi) : 0);
        const u64 cand = h ? lane_value(key, shi) : lane_value(key, slo);
        const bool on = h ? phi != 0 : plo != 0;
        const u64 own = slot;
        u64 left = dpp_u64<kDppWaveShr1>(own);
        if (c == 0) left = 0;
        if (on && c < k) slot = cand < left ? left : (cand < own ? cand : own);
        const u64 taken = (plo != 0 ? 1ull << slo : 0ull) | (phi != 0 ? 1ull << shi : 0ull);
        last = h ? lane_value(slot, 32 + k - 1) : lane_value(slot, k - 1);
        pass = __ballot(key < last) & pass & ~taken;
    }
}

// gn[j] = the fmaf chain over the squares of gallery row j in the order 0 .. d - 1, one thread to a row.
__global__ __launch_bounds__(kBlock) void knn_norms_kernel(const float* __restrict__ g, int ng, int d,
                                                           float* __restrict__ gn) {
    const size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= (size_t)ng) return;
    const f32x4* row = reinterpret_cast<const f32x4*>(g + j * d);
    float s = 0.f;
    for (int c = 0; c < d / 4; ++c) {
        const f32x4 v = row[c];
        s = fmaf(v.x, v.x, s);
        s = fmaf(v.y, v.y, s);
        s = fmaf(v.z, v.z, s);
        s = fmaf(v.w, v.w, s);
    }
    gn[j] = s;
}

// Workgroup (x, y): queries 64 x .. 64 x + 63 against gallery segment y = rows [y seg_rows, (y + 1) seg_rows) below ng.
//  1. The query tile goes to LDS once, t[64][d + 1] (rows past nq are zeros); qn[i] is the fmaf chain over the squares
//     of row i in the order 0 .. d - 1.
//  2. Wave w walks the segment in steps of 256 rows and takes rows j0 + 64 w .. + 63 of each step as two B tiles,
//     against both A tiles (the second only when the workgroup has more than 32 queries): four independent
//     accumulators.  v_mfma_f32_32x32x2_f32, lane l (c = l & 31, h = l >> 5) holding A[c][h] = t[32 u + c][f] and
//     B[h][c] = g[row c of the B tile][f], f = 8 m + 4 h + x in step (m, x), m < d/8, x < 4: the two halves of a wave
//     read the two 16-byte halves of the same 32 bytes of a gallery row, and dot_ij is the fmaf chain over the products
//     in the order 0, 4, 1, 5, 2, 6, 3, 7, then 8, 12, 9, 13, ... (each run of 8 features in that order, the runs
//     ascending).  A lane whose row lies past the segment reads the segment's last row instead and its results are
//     dropped.
//  3. C/D: register reg of lane l holds query row (reg & 3) + 8 (reg >> 2) + 4 h of the A tile, gallery row c of the
//     B tile.  The wave keeps its own sorted list of k keys per query row IN REGISTERS, laid out like the accumulators:
//     list[u][reg] of lane l is slot c of that same query row (slots k .. 31 stay fill keys).  So the list of the row
//     a register belongs to is always register list[u][reg] of the 32 lanes of the lane's own half, with static
//     indices.  The lane forms its key (a row past the segment, past nq or excluded gives the fill key) and
//     insert_passing takes in those that are smaller than the list's last key.  Passing becomes rare after the first
//     steps.  No LDS and no memory is touched.
//  4. After a barrier the lists go to LDS over the query tile, [wave][query][k]; after another, the 64 lanes of wave
//     w are the 4 lists of each of the query rows 16 w .. 16 w + 15 and pick, k times, the smallest of the 4 heads
//     (two DPP steps): the row's k smallest keys in order, written to d2 / idx when the grid has one segment, else as
//     keys to part[query][segment][k].
// Two waves per SIMD (189 VGPRs, no scratch): two workgroups to a CU, one's MFMAs under the other's selection.
__global__ __launch_bounds__(kBlock, 2) void knn_kernel(const float* __restrict__ q, const float* __restrict__ g,
                                                        const float* __restrict__ gn,
                                                        const int32_t* __restrict__ exclude, int nq, int ng, int d,
                                                        int k, int seg_rows, float* __restrict__ out_d2,
                                                        int32_t* __restrict__ out_idx, u64* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int pitch = d + kPitchPad;
    float* qn = reinterpret_cast<float*>(smem);
    int* excl = reinterpret_cast<int*>(qn + kQueryTile);
    float* tile = reinterpret_cast<float*>(excl + kQueryTile);
    u64* lists = reinterpret_cast<u64*>(tile);   // after the walk; 512 bytes in: a multiple of 8

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t q0 = (size_t)blockIdx.x * kQueryTile;
    const int rows_here = (int)((size_t)nq - q0 < (size_t)kQueryTile ? (size_t)nq - q0 : (size_t)kQueryTile);
    const bool two = rows_here > 32;
    const int seg = blockIdx.y, segments = gridDim.y;
    const long long seg_lo = (long long)seg * seg_rows;
    const int seg_begin = (int)(seg_lo < ng ? seg_lo : ng);
    const int seg_end = (int)(seg_lo + seg_rows < ng ? seg_lo + seg_rows : ng);

    for (int e = tid; e < kQueryTile * d; e += kBlock) {
        const int i = e / d, j = e - i * d;
        tile[i * pitch + j] = i < rows_here ? q[(q0 + i) * d + j] : 0.f;
    }
    __syncthreads();
    if (tid < kQueryTile) {
        const float* row = tile + tid * pitch;
        float s = 0.f;
        for (int j = 0; j < d; ++j) s = fmaf(row[j], row[j], s);
        qn[tid] = s;
        // -1: no row excluded (any negative value given means that); kDeadRow: a row past nq takes no candidate
        int ex = -1;
        if (exclude != nullptr && tid < rows_here) ex = max(exclude[q0 + tid], -1);
        excl[tid] = tid < rows_here ? ex : kDeadRow;
    }
    __syncthreads();

    const int c = lane & 31, h = lane >> 5;
    const float* a0 = tile + c * pitch + 4 * h;
    const float* a1 = a0 + 32 * pitch;
    u64 list[2][16];   // the lane's slot of the lists of its 32 query rows, in the accumulators' layout
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) list[u][reg] = kFill;

    for (long long j0 = (long long)seg_begin + wave * kWaveRows; j0 < seg_end; j0 += kStepRows) {
        int jr[2];
        bool live[2];
        const float* brow[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long long j = j0 + 32 * t + c;
            live[t] = j < seg_end;
            jr[t] = (int)(live[t] ? j : seg_end - 1);
            brow[t] = g + (size_t)jr[t] * d + 4 * h;
        }
        f32x16 acc[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[u][t] = f32x16{};
        for (int s = 0; s < d; s += 16) {   // d is a multiple of 16: four loads in flight
            f32x4 b[2][2];
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int t = 0; t < 2; ++t) b[y][t] = *reinterpret_cast<const f32x4*>(brow[t] + s + 8 * y);
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const float av0 = a0[s + 8 * y + x];
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, b[y][0][x], acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, b[y][1][x], acc[0][1], 0, 0, 0);
                    if (two) {   // uniform over the workgroup
                        const float av1 = a1[s + 8 * y + x];
                        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, b[y][0][x], acc[1][0], 0, 0, 0);
                        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, b[y][1][x], acc[1][1], 0, 0, 0);
                    }
                }
        }
        const float gnv[2] = {gn[jr[0]], gn[jr[1]]};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u == 1 && !two) continue;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int i = 32 * u + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                    const int ex = excl[i];
                    u64 key = kFill;
                    if (live[t] && ex != kDeadRow && jr[t] != ex) key = pair_key(acc[u][t][reg], qn[i], gnv[t], jr[t]);
                    insert_passing(list[u][reg], key, k, c, h);
                }
        }
    }
    __syncthreads();   // every wave has read the query tile for the last time: the lists take its place

#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int i = 32 * u + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            if (c < k) lists[(wave * kQueryTile + i) * k + c] = list[u][reg];
        }
    __syncthreads();

    const int i = 16 * wave + (lane >> 2), w = lane & 3;
    const u64* mine = lists + (w * kQueryTile + i) * k;
    int taken = 0;
    u64 head = mine[0];
    for (int t = 0; t < k; ++t) {
        u64 best = head;
        u64 other = dpp_u64<kDppQuadXor1>(best);
        best = other < best ? other : best;
        other = dpp_u64<kDppQuadXor2>(best);
        best = other < best ? other : best;
        if (head == best) {   // real keys are distinct; several lists may hold the fill key, which only fills
            ++taken;
            head = taken < k ? mine[taken] : kSpent;
        }
        if (w == 0 && i < rows_here) {
            if (part != nullptr) {
                part[((q0 + i) * segments + seg) * k + t] = best;
            } else {
                out_d2[(q0 + i) * k + t] = __uint_as_float((unsigned)(best >> 32));
                out_idx[(q0 + i) * k + t] = (int)(unsigned)best;
            }
        }
    }
}

// One wave per query: lane s holds the head of segment s's list part[query][s][k] (staged in LDS) and the wave picks,
// k times, the smallest head: the k smallest keys of all segments in order.
__global__ __launch_bounds__(64) void knn_merge_kernel(const u64* __restrict__ part, int segments, int k,
                                                       float* __restrict__ out_d2, int32_t* __restrict__ out_idx) {
    __shared__ u64 all[kMaxSegments * kMaxK];
    const int lane = threadIdx.x;
    const size_t qi = blockIdx.x;
    const u64* rows = part + qi * segments * k;
    for (int e = lane; e < segments * k; e += 64) all[e] = rows[e];
    __syncthreads();
    int span = 1;
    while (span < segments) span <<= 1;
    int taken = 0;
    u64 head = lane < segments ? all[lane * k] : kSpent;
    u64 kept = kFill;
    for (int t = 0; t < k; ++t) {
        u64 best = head;
        for (int off = span >> 1; off > 0; off >>= 1) {
            const u64 other = shfl_xor_u64(best, off);
            best = other < best ? other : best;
        }
        best = lane_value(best, 0);   // lanes span .. 63 took no part
        if (head == best) {
            ++taken;
            head = taken < k ? all[lane * k + taken] : kSpent;
        }
        if (lane == t) kept = best;
    }
    if (lane < k) {
        out_d2[qi * k + lane] = __uint_as_float((unsigned)(kept >> 32));
        out_idx[qi * k + lane] = (int)(unsigned)kept;
    }
}

bool knn_dims_ok(int nq, int ng, int d, int k) {
    return nq >= 1 && ng >= 1 && d >= kDimStep && d <= kMaxDim && d % kDimStep == 0 && k >= 1 && k <= kMaxK;
}

size_t norms_bytes(int ng) { return ((size_t)ng * sizeof(float) + 15) & ~(size_t)15; }

// qn and excl, then the query tile and, after the walk, the waves' lists in its place
size_t lds_bytes(int d, int k) {
    const size_t tile = (size_t)kQueryTile * (d + kPitchPad) * sizeof(float);
    const size_t lists = (size_t)kWaves * kQueryTile * k * sizeof(u64);
    return 2 * kQueryTile * 4 + (tile > lists ? tile : lists);
}

}  // namespace

extern "C" {

int lf_knn_query_tile(void) { return kQueryTile; }
int lf_knn_max_k(void) { return kMaxK; }

int lf_knn_segments(int nq, int ng) {
    if (nq < 1 || ng < 1) return 0;
    const long long tiles = ((long long)nq + kQueryTile - 1) / kQueryTile;
    const long long steps = ((long long)ng + kStepRows - 1) / kStepRows;   // a segment holds at least one step
    long long s = kFillCUs / tiles;
    if (s > kMaxSegments) s = kMaxSegments;
    if (s > steps) s = steps;
    return s < 1 ? 1 : (int)s;
}

size_t lf_knn_topk_workspace(int nq, int ng, int k, int segments) {
    if (nq < 1 || ng < 1 || k < 1 || k > kMaxK || segments < 1 || segments > kMaxSegments) return 0;
    return norms_bytes(ng) + (segments > 1 ? (size_t)nq * segments * k * sizeof(u64) : 0);
}

int lf_knn_topk_f32(const float* q, const float* g, int nq, int ng, int d, int k, const int32_t* exclude,
                    int segments, float* d2, int32_t* idx, void* ws, size_t ws_bytes, lf_stream_t stream) {
    LF_REQUIRE(q && g && d2 && idx && ws, "lf_knn_topk: null buffer");
    LF_REQUIRE(knn_dims_ok(nq, ng, d, k),
               "lf_knn_topk: bad dims nq=%d ng=%d d=%d k=%d (nq, ng >= 1, d a multiple of %d in %d..%d, k in 1..%d)", nq,
               ng, d, k, kDimStep, kDimStep, kMaxDim, kMaxK);
    LF_REQUIRE(segments >= 1 && segments <= kMaxSegments, "lf_knn_topk: segments=%d (1..%d)", segments, kMaxSegments);
    LF_REQUIRE(((uintptr_t)g & 15) == 0, "lf_knn_topk: the gallery must be 16-byte aligned");
    LF_REQUIRE(((uintptr_t)ws & 15) == 0, "lf_knn_topk: the workspace must be 16-byte aligned");
    LF_REQUIRE(ws_bytes >= lf_knn_topk_workspace(nq, ng, k, segments), "lf_knn_topk: workspace too small (%zu < %zu)",
               ws_bytes, lf_knn_topk_workspace(nq, ng, k, segments));
    static const bool lds_ok =
        hipFuncSetAttribute(reinterpret_cast<const void*>(knn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_bytes(kMaxDim, kMaxK)) == hipSuccess;
    LF_REQUIRE(lds_ok, "lf_knn_topk: the device refused %zu bytes of LDS per workgroup", lds_bytes(kMaxDim, kMaxK));
    hipStream_t s = lf::as_stream(stream);
    float* gn = static_cast<float*>(ws);
    u64* part = segments > 1 ? reinterpret_cast<u64*>(static_cast<unsigned char*>(ws) + norms_bytes(ng)) : nullptr;
    const int seg_rows = (int)(((long long)ng + segments - 1) / segments);
    const unsigned tiles = (unsigned)(((size_t)nq + kQueryTile - 1) / kQueryTile);
    knn_norms_kernel<<<(unsigned)(((size_t)ng + kBlock - 1) / kBlock), kBlock, 0, s>>>(g, ng, d, gn);
    knn_kernel<<<dim3(tiles, (unsigned)segments), kBlock, lds_bytes(d, k), s>>>(q, g, gn, exclude, nq, ng, d, k,
                                                                                seg_rows, d2, idx, part);
    if (segments > 1) knn_merge_kernel<<<(unsigned)nq, 64, 0, s>>>(part, segments, k, d2, idx);
    return lf::check_launch("lf_knn_topk");
}

}  // extern "C"
