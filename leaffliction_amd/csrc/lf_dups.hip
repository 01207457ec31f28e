// libleafhip — near-duplicate search: a 128-bit difference hash of every image of a batch with up to eight flipped /
// turned variants (lf_dhash128_u8), and the all-pairs Hamming search over such signatures as count -> scan -> fill
// (lf_hamming_pairs_count / lf_hamming_pairs_fill).  The rules are stated in include/leafhip.h and DESIGN.md.
//
// Everything here is integer and exact; no float appears.  Width of the cell comparison: a luma value is at most
// 255 * 256 = 65,280, a cell of a 4096 x 4096 image holds at most 456 * 456 = 207,936 pixels, so a cell sum stays
// below 1.36e10 and a cross product sum_a * cnt_b below 2.83e15 < 2^63: 64-bit arithmetic never wraps.
#include "lf_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kGrid = 9;        // cells per side
constexpr int kUnit = 16;       // pixels a thread takes at a time: 48 bytes, three 16-byte loads
constexpr int kMinSide = 9, kMaxSide = 4096;

__host__ __device__ __forceinline__ int cell_bound(int c, int extent) { return (c * extent + 4) / kGrid; }

// 48 bytes of pixels from flat pixel p on, as twelve dwords: three 16-byte loads where the image lies on a 16-byte
// boundary and the unit is whole, else byte by byte and only the bytes that exist
template <bool ALIGNED>
__device__ __forceinline__ void load_unit(const uint8_t* __restrict__ img, size_t p, int npx, unsigned (&d)[12]) {
    const uint8_t* src = img + p * 3;
    if (ALIGNED && npx == kUnit) {
        const lf::u32x4* q = reinterpret_cast<const lf::u32x4*>(src);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const lf::u32x4 v = q[k];
            d[4 * k] = v.x;
            d[4 * k + 1] = v.y;
            d[4 * k + 2] = v.z;
            d[4 * k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * k + b < 3 * npx) v |= (unsigned)src[4 * k + b] << (8 * b);
            d[k] = v;
        }
    }
}
// the luma weights of the four bytes of dword k of a unit, k % 3 = phase: byte j of it is channel (4k + j) % 3
__device__ __forceinline__ constexpr unsigned luma_weights(int phase) {
    constexpr unsigned wt[3] = {77u, 150u, 29u};
    unsigned v = 0;
    for (int j = 0; j < 4; ++j) v |= wt[(4 * phase + j) % 3] << (8 * j);
    return v;
}
__device__ __forceinline__ unsigned byte_of(const unsigned (&d)[12], int i) { return (d[i >> 2] >> (8 * (i & 3))) & 255u; }

// One unit of `npx` pixels from flat pixel p on, held in `cur`, added to the cell sums it falls into.
__device__ __forceinline__ void sum_unit(unsigned long long* cell, const unsigned (&cur)[12], unsigned p, int npx,
                                         int h, int w) {
    int y = (int)(p / (unsigned)w), x = (int)(p - (unsigned)y * (unsigned)w);   // hw <= 2^24
    int r = min(kGrid - 1, y * kGrid / h), c = min(kGrid - 1, x * kGrid / w);
    // (the guesses are off by at most one either way: settle them on the bounds themselves)
    while (y < cell_bound(r, h)) --r;
    while (y >= cell_bound(r + 1, h)) ++r;
    while (x < cell_bound(c, w)) --c;
    while (x >= cell_bound(c + 1, w)) ++c;
    int x_next = cell_bound(c + 1, w), y_next = cell_bound(r + 1, h);
    const int second = c + 2 <= kGrid ? cell_bound(c + 2, w) : w + kUnit;
    if (npx == kUnit && x + kUnit <= w && second - x >= kUnit) {
        // the usual unit: whole, in one image row, at most one cell border inside.  Twelve byte dot products give
        // its luma sum (prefix[k] = the sum of the bytes before dword k); the part left of a border after `left`
        // pixels is the prefix at the dword the border falls in plus that dword's bytes before it.
        unsigned prefix[13];
        prefix[0] = 0;
#pragma unroll
        for (int k = 0; k < 12; ++k) prefix[k + 1] = __builtin_amdgcn_udot4(cur[k], luma_weights(k % 3), prefix[k], false);
        const int left = x_next - x;
        if (left >= kUnit) {
            atomicAdd(&cell[r * kGrid + c], (unsigned long long)prefix[12]);
        } else {
            const int cut = 3 * left, kb = cut >> 2;   // 3 <= cut <= 45
            unsigned before = 0, word = 0, wts = 0;
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                before = k == kb ? prefix[k] : before;
                word = k == kb ? cur[k] : word;
                wts = k == kb ? luma_weights(k % 3) : wts;
            }
            const unsigned mask = (1u << (8 * (cut & 3))) - 1u;
            const unsigned lsum = __builtin_amdgcn_udot4(word & mask, wts, before, false);
            atomicAdd(&cell[r * kGrid + c], (unsigned long long)lsum);
            atomicAdd(&cell[r * kGrid + c + 1], (unsigned long long)(prefix[12] - lsum));
        }
    } else {
        unsigned acc = 0;   // at most 16 * 65,280
#pragma unroll
        for (int i = 0; i < kUnit; ++i) {
            if (i < npx) {
                acc += 77u * byte_of(cur, 3 * i) + 150u * byte_of(cur, 3 * i + 1) + 29u * byte_of(cur, 3 * i + 2);
                if (++x == x_next || i == npx - 1) {
                    atomicAdd(&cell[r * kGrid + c], (unsigned long long)acc);
                    acc = 0;
                    if (x == w) {
                        x = 0;
                        c = 0;
                        if (++y == y_next) y_next = cell_bound(++r + 1, h);
                    } else if (x == x_next) {
                        ++c;
                    }
                    x_next = cell_bound(c + 1, w);
                }
            }
        }
    }
}

// One workgroup = one image, read once.  The image is walked as a flat run of pixels in units of 16 (48 contiguous
// bytes per lane, 3 KiB per wave and step); the next unit is asked for before the current one is summed (two register buffers taking turns).  A lane
// sums the luma of its unit per cell and adds each part to the cell's 64-bit sum in LDS (a cell is at least w/9
// pixels wide, so that is once or twice per unit) — LDS atomics on integers: the sums do not depend on the order.
// The usual unit is summed with byte dot products, twelve for its 48 bytes; a ragged one (the image's last, one that
// runs over a row end or over two cell borders, which takes w < 144 or w % 16 != 0) pixel by pixel.  Cell pixel
// counts are the products of the cell's extents and are not counted.  Then thread k of every 128 forms bit k of one
// variant and a wave ballot packs 64 bits at a time.
template <bool ALIGNED>
__global__ __launch_bounds__(kBlock) void dhash128_kernel(const uint8_t* __restrict__ in, int32_t* __restrict__ sig,
                                                          int h, int w, int variants) {
    __shared__ unsigned long long cell[kGrid * kGrid];
    const unsigned hw = (unsigned)h * (unsigned)w;   // at most 2^24
    const uint8_t* img = in + (size_t)blockIdx.x * hw * 3;
    for (int k = threadIdx.x; k < kGrid * kGrid; k += kBlock) cell[k] = 0;
    __syncthreads();

    const unsigned units = (hw + kUnit - 1) / kUnit;
    const auto pixels = [&](unsigned u) { return (int)min((unsigned)kUnit, hw - u * kUnit); };
    unsigned even[12], odd[12];
    unsigned u = threadIdx.x;
    if (u < units) load_unit<ALIGNED>(img, (size_t)u * kUnit, pixels(u), even);
    while (u < units) {
        if (u + kBlock < units) load_unit<ALIGNED>(img, (size_t)(u + kBlock) * kUnit, pixels(u + kBlock), odd);
        sum_unit(cell, even, u * kUnit, pixels(u), h, w);
        u += kBlock;
        if (u >= units) break;
        if (u + kBlock < units) load_unit<ALIGNED>(img, (size_t)(u + kBlock) * kUnit, pixels(u + kBlock), even);
        sum_unit(cell, odd, u * kUnit, pixels(u), h, w);
        u += kBlock;
    }
    __syncthreads();

    // bit k of variant s: k < 64 compares a cell with its right neighbour, else with the one below
    for (int k = threadIdx.x; k < variants * 128; k += kBlock) {   // (a multiple of 64: whole waves)
        const int s = k >> 7, bit = k & 127;
        const int rr = (bit >> 3) & 7, cc = bit & 7;
        const bool down = bit >= 64;
        int ra[2] = {rr, down ? rr + 1 : rr}, ca[2] = {cc, down ? cc : cc + 1};
        unsigned long long sum[2], cnt[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int r0 = (s & 4) ? ca[e] : ra[e], c0 = (s & 4) ? ra[e] : ca[e];
            const int r1 = (s & 2) ? kGrid - 1 - r0 : r0, c1 = (s & 1) ? kGrid - 1 - c0 : c0;
            sum[e] = cell[r1 * kGrid + c1];
            cnt[e] = (unsigned long long)((cell_bound(r1 + 1, h) - cell_bound(r1, h)) *
                                          (cell_bound(c1 + 1, w) - cell_bound(c1, w)));
        }
        const unsigned long long m = __ballot(sum[0] * cnt[1] < sum[1] * cnt[0]);
        if ((threadIdx.x & 63) == 0) {
            int32_t* dst = sig + ((size_t)blockIdx.x * variants + s) * 4 + (bit >> 5);
            dst[0] = (int32_t)(unsigned)m;
            dst[1] = (int32_t)(unsigned)(m >> 32);
        }
    }
}

// ---- pair search
constexpr int kTile = 128;        // columns of b staged at a time: kTile * V signatures, at most 16 KiB
constexpr int kWantBlocks = 2048; // workgroups that fill the chip a few times over

// the columns are cut into `chunks` runs of whole tiles over gridDim.y, so that few rows of `a` still fill the chip
inline int pair_chunks(int na, int nb) {
    const int row_blocks = (na + kBlock - 1) / kBlock, tiles = (nb + kTile - 1) / kTile;
    int want = (kWantBlocks + row_blocks - 1) / row_blocks;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    const int tiles_per = (tiles + want - 1) / want;
    return (tiles + tiles_per - 1) / tiles_per;
}
inline int pair_chunk_cols(int nb, int chunks) {
    const int tiles = (nb + kTile - 1) / kTile;
    return (tiles + chunks - 1) / chunks * kTile;
}

__device__ __forceinline__ int dist128(const lf::u32x4& a, const lf::u32x4& b) {
    return __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w);
}

// One thread = one row i of `a`, held in registers; workgroup (x, y) walks the columns of chunk y tile by tile: a
// tile's kTile * V signatures are staged in LDS with 16-byte loads and read back at one address per step by the whole
// wave (a broadcast).  FILL = false counts the matches of (i, chunk); FILL = true repeats the walk and stores row
// {i, j, distance, s} number k of (i, chunk) at offsets[i * chunks + chunk] + k, which is ascending in j: with the
// offsets an exclusive scan over (i major, chunk minor) the rows come out in ascending (i, j) order.  In self mode a
// tile whose columns all lie at or left of the workgroup's first row is skipped by all its threads together.
template <int V, bool FILL>
__global__ __launch_bounds__(kBlock) void hamming_pairs_kernel(const int32_t* __restrict__ a, long long a_stride,
                                                               int na, const lf::u32x4* __restrict__ b, int nb,
                                                               int threshold, int self, int chunk_cols,
                                                               int32_t* __restrict__ counts,
                                                               const long long* __restrict__ offsets,
                                                               int32_t* __restrict__ out) {
    __shared__ lf::u32x4 tile[kTile * V];
    const int i0 = (int)blockIdx.x * kBlock, i = i0 + (int)threadIdx.x;
    const bool live = i < na;
    lf::u32x4 mine = {0u, 0u, 0u, 0u};
    if (live) {
        const int32_t* row = a + (size_t)i * a_stride;
        mine.x = (unsigned)row[0];
        mine.y = (unsigned)row[1];
        mine.z = (unsigned)row[2];
        mine.w = (unsigned)row[3];
    }
    const int col0 = (int)blockIdx.y * chunk_cols, col1 = min(nb, col0 + chunk_cols);
    const size_t slot = (size_t)i * gridDim.y + blockIdx.y;
    int found = 0;
    int32_t* dst = nullptr;
    if (FILL && live) dst = out + (size_t)offsets[slot] * 4;
    for (int j0 = col0; j0 < col1; j0 += kTile) {
        const int jn = min(kTile, col1 - j0);
        if (self && j0 + jn - 1 <= i0) continue;   // uniform over the workgroup
        __syncthreads();
        for (int k = threadIdx.x; k < jn * V; k += kBlock) tile[k] = b[(size_t)j0 * V + k];
        __syncthreads();
        if (!live) continue;
        for (int jj = 0; jj < jn; ++jj) {
            int best = dist128(mine, tile[jj * V]), at = 0;
#pragma unroll
            for (int s = 1; s < V; ++s) {
                const int d = dist128(mine, tile[jj * V + s]);
                if (d < best) {
                    best = d;
                    at = s;
                }
            }
            const int j = j0 + jj;
            if (best <= threshold && (!self || j > i)) {
                if (FILL) {
                    const lf::u32x4 rowv = {(unsigned)i, (unsigned)j, (unsigned)best, (unsigned)at};
                    *reinterpret_cast<lf::u32x4*>(dst + (size_t)found * 4) = rowv;
                }
                ++found;
            }
        }
    }
    if (!FILL && live) counts[slot] = found;
}

template <bool FILL>
int launch_pairs(const int32_t* a, long long a_stride, int na, const int32_t* b, int nb, int variants, int threshold,
                 int self, int chunks, int32_t* counts, const long long* offsets, int32_t* out, hipStream_t s) {
    const dim3 grid((unsigned)((na + kBlock - 1) / kBlock), (unsigned)chunks);
    const int cols = pair_chunk_cols(nb, chunks);
    const lf::u32x4* bv = reinterpret_cast<const lf::u32x4*>(b);
#define LF_PAIRS(VV)                                                                                               \
    hamming_pairs_kernel<VV, FILL><<<grid, kBlock, 0, s>>>(a, a_stride, na, bv, nb, threshold, self, cols, counts, \
                                                           offsets, out)
    switch (variants) {
        case 1: LF_PAIRS(1); break;
        case 2: LF_PAIRS(2); break;
        case 4: LF_PAIRS(4); break;
        default: LF_PAIRS(8); break;
    }
#undef LF_PAIRS
    return lf::check_launch(FILL ? "lf_hamming_pairs_fill" : "lf_hamming_pairs_count");
}

bool variants_ok(int v) { return v == 1 || v == 2 || v == 4 || v == 8; }

int pairs_checks(const char* who, const int32_t* a, long long a_stride, int na, const int32_t* b, int nb, int variants,
                 int threshold, int self, int chunks) {
    LF_REQUIRE(a && b, "%s: null buffer", who);
    LF_REQUIRE(na > 0 && nb > 0, "%s: bad dims na=%d nb=%d", who, na, nb);
    LF_REQUIRE(variants_ok(variants), "%s: variants=%d (1, 2, 4 or 8)", who, variants);
    LF_REQUIRE(threshold >= 0 && threshold <= 128, "%s: threshold=%d (0..128)", who, threshold);
    LF_REQUIRE(a_stride >= 4, "%s: a_stride=%lld (at least 4 int32)", who, a_stride);
    LF_REQUIRE(((uintptr_t)b & 15) == 0 && ((uintptr_t)a & 3) == 0, "%s: b must lie on a 16-byte boundary", who);
    LF_REQUIRE(!self || na == nb, "%s: self mode needs na == nb, got %d and %d", who, na, nb);
    LF_REQUIRE(chunks == pair_chunks(na, nb), "%s: chunks=%d, lf_hamming_pairs_chunks(%d, %d) = %d", who, chunks, na,
               nb, pair_chunks(na, nb));
    return LF_OK;
}

}  // namespace

extern "C" {

int lf_dhash128_u8(const uint8_t* in, int32_t* sig, int n, int h, int w, int variants, lf_stream_t stream) {
    LF_REQUIRE(in && sig, "lf_dhash128: null buffer");
    LF_REQUIRE(n > 0, "lf_dhash128: bad dims n=%d", n);
    LF_REQUIRE(h >= kMinSide && h <= kMaxSide && w >= kMinSide && w <= kMaxSide,
               "lf_dhash128: h=%d w=%d (each %d..%d)", h, w, kMinSide, kMaxSide);
    LF_REQUIRE(variants_ok(variants), "lf_dhash128: variants=%d (1, 2, 4 or 8)", variants);
    const bool aligned = ((uintptr_t)in & 15) == 0 && ((size_t)h * w * 3) % 16 == 0;
    auto kern = aligned ? dhash128_kernel<true> : dhash128_kernel<false>;
    kern<<<(unsigned)n, kBlock, 0, lf::as_stream(stream)>>>(in, sig, h, w, variants);
    return lf::check_launch("lf_dhash128");
}

int lf_hamming_pairs_tile(void) { return kTile; }
int lf_hamming_pairs_rows(void) { return kBlock; }

int lf_hamming_pairs_chunks(int na, int nb) {
    if (na <= 0 || nb <= 0) {
        lf::set_error("lf_hamming_pairs_chunks: bad dims na=%d nb=%d", na, nb);
        return 0;
    }
    return pair_chunks(na, nb);
}

int lf_hamming_pairs_count(const int32_t* a, long long a_stride, int na, const int32_t* b, int nb, int variants,
                           int threshold, int self, int32_t* counts, int chunks, lf_stream_t stream) {
    const int rc = pairs_checks("lf_hamming_pairs_count", a, a_stride, na, b, nb, variants, threshold, self, chunks);
    if (rc != LF_OK) return rc;
    LF_REQUIRE(counts, "lf_hamming_pairs_count: null buffer");
    return launch_pairs<false>(a, a_stride, na, b, nb, variants, threshold, self, chunks, counts, nullptr, nullptr,
                               lf::as_stream(stream));
}

int lf_hamming_pairs_fill(const int32_t* a, long long a_stride, int na, const int32_t* b, int nb, int variants,
                          int threshold, int self, const long long* offsets, int chunks, int32_t* out,
                          lf_stream_t stream) {
    const int rc = pairs_checks("lf_hamming_pairs_fill", a, a_stride, na, b, nb, variants, threshold, self, chunks);
    if (rc != LF_OK) return rc;
    LF_REQUIRE(offsets && out, "lf_hamming_pairs_fill: null buffer");
    LF_REQUIRE(((uintptr_t)out & 15) == 0, "lf_hamming_pairs_fill: out must lie on a 16-byte boundary");
    return launch_pairs<true>(a, a_stride, na, b, nb, variants, threshold, self, chunks, nullptr, offsets, out,
                              lf::as_stream(stream));
}

}  // extern "C"
