// nm_segments.hip - nm_segment_table: one row of descriptors per segment of a labelled cloud (gfx950, wave64).
// the contract (columns, degenerate segments, arithmetic, summation order) is in include/nimrud_hip.h.
//
// stages, all on the caller's stream, scratch from the caller:
//   1. k_seg_keys + a stable radix sort of (label, row) pairs: the rows of every segment, ascending.  rows of no
//      segment get the key n_segments and end up behind the last segment.  k_seg_starts: where each segment begins.
//   2. k_seg_short: a group of 8 lanes per segment.  a segment of at most SEG_SHORT rows is finished here, one row
//      to a lane; a longer one gets its number of chunks noted.
//      an exclusive scan of the chunk counts is the flat chunk list: chunk t belongs to the last segment whose
//      first chunk is <= t (a binary search per wave).  work is dealt out by chunks from here on.
//   3. k_seg_box: a wave per chunk; n, the row count and the box of the chunk (the box through an order-preserving
//      map of fp64 onto uint64), one partial of 8 words per chunk.  k_seg_box_join: the wave of a segment's first
//      chunk joins its partials - integer sums, minima and maxima: exact, whatever the order.  (integer atomics
//      into one accumulator per segment were measured first: the 5 685 chunks of the benchmark scene's ground
//      cluster queue up on eight addresses, 0.53 ms against 0.02 ms this way.)
//   4. k_seg_moments: a wave per chunk; d = p - box minimum, w d and w d (x) d summed in the chunk tree, one partial
//      of 9 doubles per chunk.
//   5. k_seg_finish: the wave of a segment's first chunk adds its partials in the second tree and writes the row.
// no atomics of any kind, no raw moments of p.
//
// the two trees (NM_SEGMENT_CHUNK = 256 = 64 slots x 4):
//   chunk tree:   slot j of 64 adds rows j, j + 64, j + 128, j + 192 of the chunk left to right; then slots are
//                 added pairwise, neighbours first: j += j + 1 (j even), j += j + 2 (j % 4 == 0), ... j += j + 32.
//                 an absent row is +0, which changes no sum - so the 8-lane group of k_seg_short (slots 0..7, the
//                 first three pairwise steps) forms the same bits as a whole wave would.
//   segment tree: slot j of 64 adds chunk partials j, j + 64, j + 128, ... left to right; then the same pairwise steps.
#include "nm_common.h"
#include "nm_eigen.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

static_assert(NM_SEGMENT_CHUNK == 256, "the chunk tree below is written for 64 slots of 4 rows");
static_assert(NM_SEGMENT_COLUMNS == 25, "the row layout below has 25 columns");

constexpr int SEG_SHORT = 8;             // a segment up to here is one 8-lane group's work, start to finish
constexpr int SEG_SLOT_ROWS = NM_SEGMENT_CHUNK / 64;
constexpr int SEG_BOX_WORDS = 8;         // per segment: n, rows, min xyz, max xyz (uint64 each)
constexpr int SEG_MAX_BLOCKS = 4096;     // chunk kernels: 4 waves to a block, the waves share the chunks out

struct SegPlan {
    int64_t max_chunks;
    size_t sort_bytes, scan_bytes;
    size_t off_key_in, off_key_out, off_row_in, off_row_out, off_start, off_first, off_box, off_chunk_box, off_partial,
        off_sort, off_scan, bytes;
};

static size_t seg_pad(size_t b) { return (b + 255) / 256 * 256; }

// temporary storage of the two library primitives: asked with null pointers, nothing is launched
static size_t seg_sort_bytes(int64_t n)
{
    size_t temp = 0;
    (void)rocprim::radix_sort_pairs(nullptr, temp, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                    (uint32_t*)nullptr, (size_t)n, 0, 32, (hipStream_t)0);
    return temp;
}
static size_t seg_scan_bytes(int64_t c)
{
    size_t temp = 0;
    (void)rocprim::exclusive_scan(nullptr, temp, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)c,
                                  rocprim::plus<uint32_t>(), (hipStream_t)0);
    return temp;
}

static SegPlan seg_plan(int64_t n, int64_t c)
{
    SegPlan P;
    // a long segment of len rows has at most len / K + 1 chunks, and there are at most n / (SEG_SHORT + 1) of them
    const int64_t longs = n / (SEG_SHORT + 1) < c ? n / (SEG_SHORT + 1) : c;
    P.max_chunks = n / NM_SEGMENT_CHUNK + longs;
    // the primitives' needs are not promised to grow with the size (they change algorithm on the way): take the
    // largest over the sizes they switch at, so that the whole is monotone
    P.sort_bytes = P.scan_bytes = 0;
    for (int64_t m = 1; m / 2 <= n; m *= 2) {
        const size_t b = seg_sort_bytes(m < n ? m : n);
        if (b > P.sort_bytes) P.sort_bytes = b;
    }
    for (int64_t m = 1; m / 2 <= c + 1; m *= 2) {
        const size_t b = seg_scan_bytes(m < c + 1 ? m : c + 1);
        if (b > P.scan_bytes) P.scan_bytes = b;
    }
    size_t off = 0;
    auto take = [&off](size_t b) {
        const size_t at = off;
        off += seg_pad(b);
        return at;
    };
    P.off_key_in = take((size_t)n * 4);
    P.off_key_out = take((size_t)n * 4);
    P.off_row_in = take((size_t)n * 4);
    P.off_row_out = take((size_t)n * 4);
    P.off_start = take((size_t)(c + 1) * 4);
    P.off_first = take((size_t)(c + 1) * 4);
    P.off_box = take((size_t)c * SEG_BOX_WORDS * 8);
    P.off_chunk_box = take((size_t)P.max_chunks * SEG_BOX_WORDS * 8);
    P.off_partial = take((size_t)P.max_chunks * 9 * 8);
    P.off_sort = take(P.sort_bytes);
    P.off_scan = take(P.scan_bytes);
    P.bytes = off + 256;
    return P;
}

// ---- fp64 <-> uint64, order preserving (the box is joined as integers) ----------------------------------------------------
__device__ __forceinline__ unsigned long long seg_enc(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double seg_dec(unsigned long long e)
{
    const unsigned long long b = (e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e;
    return __longlong_as_double((long long)b);
}

// ---- the row -----------------------------------------------------------------------------------------------------------
// n = sum of weights, r = rows of positive weight, box, S[0..2] = sum w d, S[3..8] = sum w d (x) d (xx xy xz yy yz zz),
// d = p - mn
__device__ __forceinline__ void seg_write_row(int64_t n, uint32_t r, const double* mn, const double* mx, const double* S,
                                              double* __restrict__ out)
{
    double row[NM_SEGMENT_COLUMNS];
#pragma unroll
    for (int c = 0; c < NM_SEGMENT_COLUMNS; ++c) row[c] = 0.0;
    if (n > 0) {
        const double dn = (double)n;
        row[0] = dn;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            row[1 + a] = mn[a] + S[a] / dn;
            row[4 + a] = mn[a];
            row[7 + a] = mx[a];
        }
        if (n >= 2) {
            const double f = dn - 1.0;
            const double cxx = (S[3] - S[0] * S[0] / dn) / f, cxy = (S[4] - S[0] * S[1] / dn) / f,
                         cxz = (S[5] - S[0] * S[2] / dn) / f, cyy = (S[6] - S[1] * S[1] / dn) / f,
                         cyz = (S[7] - S[1] * S[2] / dn) / f, czz = (S[8] - S[2] * S[2] / dn) / f;
            row[10] = cxx; row[11] = cxy; row[12] = cxz; row[13] = cyy; row[14] = cyz; row[15] = czz;
            const double tr = cxx + cyy + czz;
            if (tr > 0.0) {
                // the solve and both vectors on the matrix scaled to unit trace
                const double inv = 1.0 / tr;
                const double a00 = cxx * inv, a01 = cxy * inv, a02 = cxz * inv, a11 = cyy * inv, a12 = cyz * inv,
                             a22 = czz * inv;
                double l0, l1, l2;
                nm_eig3(a00, a01, a02, a11, a12, a22, l0, l1, l2);
                row[16] = l0 * tr; row[17] = l1 * tr; row[18] = l2 * tr;
                if (r >= 3) {
                    nm_unit_eigenvector(a00, a01, a02, a11, a12, a22, l2, 1.0, 1.0, 1.0, row + 19);
                    nm_unit_eigenvector(a00, a01, a02, a11, a12, a22, l0, 1.0, 1.0, 1.0, row + 22);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NM_SEGMENT_COLUMNS; ++c) out[c] = row[c];
}

// the nine terms of one row into the running sums of a slot
__device__ __forceinline__ void seg_add_row(double* S, double w, double dx, double dy, double dz)
{
    const double wx = w * dx, wy = w * dy, wz = w * dz;
    S[0] += wx; S[1] += wy; S[2] += wz;
    S[3] += wx * dx; S[4] += wx * dy; S[5] += wx * dz;
    S[6] += wy * dy; S[7] += wy * dz; S[8] += wz * dz;
}

// pairwise steps over `width` neighbouring slots (a power of two up to 64): the sum ends in the first of them
template <int WIDTH>
__device__ __forceinline__ void seg_tree(double* S)
{
#pragma unroll
    for (int s = 1; s < WIDTH; s <<= 1)
#pragma unroll
        for (int c = 0; c < 9; ++c) S[c] += __shfl_down(S[c], s, 64);
}

// ---- stage 1 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_seg_keys(const int64_t* __restrict__ label, int64_t n, int64_t c,
                                                  uint32_t* __restrict__ key, uint32_t* __restrict__ row)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t l = label[i];
    key[i] = (l >= 0 && l < c) ? (uint32_t)l : (uint32_t)c;
    row[i] = (uint32_t)i;
}

// start[s] = number of sorted keys below s, s = 0 .. c
__global__ __launch_bounds__(256) void k_seg_starts(const uint32_t* __restrict__ key, int64_t n, int64_t c,
                                                    uint32_t* __restrict__ start)
{
    const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (s > c) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)key[mid] < s) lo = mid + 1;
        else hi = mid;
    }
    start[s] = (uint32_t)lo;
}

// ---- stage 2 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_seg_short(const double* __restrict__ xyz, int64_t stride,
                                                   const int64_t* __restrict__ weight,
                                                   const uint32_t* __restrict__ rows,
                                                   const uint32_t* __restrict__ start, int64_t c,
                                                   uint32_t* __restrict__ n_chunks, double* __restrict__ table,
                                                   int64_t tstride)
{
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t seg = t / SEG_SHORT;
    const int lane = (int)(t % SEG_SHORT);
    // (the grid is whole groups; a group past the end still takes part in the shuffles below, with no rows)
    const bool real = seg < c;
    const uint32_t s = real ? start[seg] : 0u;
    const uint32_t len = real ? start[seg + 1] - s : 0u;
    const bool here = len <= (uint32_t)SEG_SHORT;
    if (real && lane == 0)
        n_chunks[seg] = here ? 0u : (len + (uint32_t)NM_SEGMENT_CHUNK - 1u) / (uint32_t)NM_SEGMENT_CHUNK;
    if (seg == c && lane == 0) n_chunks[c] = 0u;       // (the scan's last entry: the number of chunks)
    double p[3] = {0.0, 0.0, 0.0};
    int64_t w = 0;
    if (here && (uint32_t)lane < len) {
        const int64_t r = (int64_t)rows[s + (uint32_t)lane];
        const double* q = xyz + r * stride;
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
        w = weight ? weight[r] : 1;
    }
    const bool counts = w > 0;
    int64_t n = w;
    uint32_t r = counts ? 1u : 0u;
    double mn[3], mx[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mn[a] = counts ? p[a] : INFINITY;
        mx[a] = counts ? p[a] : -INFINITY;
    }
#pragma unroll
    for (int m = 1; m < SEG_SHORT; m <<= 1) {
        n += __shfl_xor(n, m, 64);
        r += __shfl_xor(r, m, 64);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = fmin(mn[a], __shfl_xor(mn[a], m, 64));
            mx[a] = fmax(mx[a], __shfl_xor(mx[a], m, 64));
        }
    }
    double S[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = 0.0;
    if (counts) seg_add_row(S, (double)w, p[0] - mn[0], p[1] - mn[1], p[2] - mn[2]);
    seg_tree<SEG_SHORT>(S);
    if (real && here && lane == 0) seg_write_row(n, r, mn, mx, S, table + seg * tstride);
}

// the segment of chunk t: the last one whose first chunk is <= t
__device__ __forceinline__ int64_t seg_of_chunk(const uint32_t* __restrict__ first, int64_t c, uint32_t t)
{
    int64_t lo = 0, hi = c;        // first[lo] <= t < first[hi] (first[c] = all chunks)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (first[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- stage 3 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_seg_box(const double* __restrict__ xyz, int64_t stride,
                                                 const int64_t* __restrict__ weight,
                                                 const uint32_t* __restrict__ rows,
                                                 const uint32_t* __restrict__ start,
                                                 const uint32_t* __restrict__ first, int64_t c,
                                                 unsigned long long* __restrict__ chunk_box)
{
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6), total = first[c];
    for (uint32_t t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < total; t += waves) {
        const int64_t seg = seg_of_chunk(first, c, t);
        const uint32_t s = start[seg], len = start[seg + 1] - s;
        const uint32_t at = (t - first[seg]) * (uint32_t)NM_SEGMENT_CHUNK;
        const uint32_t cnt = len - at < (uint32_t)NM_SEGMENT_CHUNK ? len - at : (uint32_t)NM_SEGMENT_CHUNK;
        int64_t n = 0;
        uint32_t r = 0;
        double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int k = 0; k < SEG_SLOT_ROWS; ++k) {
            const uint32_t i = (uint32_t)lane + 64u * k;
            if (i < cnt) {
                const int64_t row = (int64_t)rows[s + at + i];
                const int64_t w = weight ? weight[row] : 1;
                if (w > 0) {
                    const double* q = xyz + row * stride;
                    n += w;
                    ++r;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const double v = q[a];
                        mn[a] = fmin(mn[a], v);
                        mx[a] = fmax(mx[a], v);
                    }
                }
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            n += __shfl_xor(n, m, 64);
            r += __shfl_xor(r, m, 64);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                mn[a] = fmin(mn[a], __shfl_xor(mn[a], m, 64));
                mx[a] = fmax(mx[a], __shfl_xor(mx[a], m, 64));
            }
        }
        if (lane == 0) {
            // (a chunk without a row of positive weight: +inf and -inf, which change no minimum and no maximum)
            unsigned long long* b = chunk_box + (int64_t)t * SEG_BOX_WORDS;
            b[0] = (unsigned long long)n;
            b[1] = (unsigned long long)r;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                b[2 + a] = seg_enc(mn[a]);
                b[5 + a] = seg_enc(mx[a]);
            }
        }
    }
}

// the wave of a segment's first chunk joins the chunk boxes of the segment
__global__ __launch_bounds__(256) void k_seg_box_join(const uint32_t* __restrict__ first, int64_t c,
                                                      const unsigned long long* __restrict__ chunk_box,
                                                      unsigned long long* __restrict__ box)
{
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6), total = first[c];
    for (uint32_t t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < total; t += waves) {
        const int64_t seg = seg_of_chunk(first, c, t);
        if (first[seg] != t) continue;
        const uint32_t nch = first[seg + 1] - t;
        unsigned long long v[SEG_BOX_WORDS] = {0ull, 0ull, ~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
        for (uint32_t i = (uint32_t)lane; i < nch; i += 64u) {
            const unsigned long long* b = chunk_box + (int64_t)(t + i) * SEG_BOX_WORDS;
            v[0] += b[0];
            v[1] += b[1];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                v[2 + a] = b[2 + a] < v[2 + a] ? b[2 + a] : v[2 + a];
                v[5 + a] = b[5 + a] > v[5 + a] ? b[5 + a] : v[5 + a];
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            v[0] += __shfl_xor(v[0], m, 64);
            v[1] += __shfl_xor(v[1], m, 64);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const unsigned long long lo = __shfl_xor(v[2 + a], m, 64), hi = __shfl_xor(v[5 + a], m, 64);
                v[2 + a] = lo < v[2 + a] ? lo : v[2 + a];
                v[5 + a] = hi > v[5 + a] ? hi : v[5 + a];
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < SEG_BOX_WORDS; ++k) box[seg * SEG_BOX_WORDS + k] = v[k];
        }
    }
}

// ---- stage 4 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_seg_moments(const double* __restrict__ xyz, int64_t stride,
                                                     const int64_t* __restrict__ weight,
                                                     const uint32_t* __restrict__ rows,
                                                     const uint32_t* __restrict__ start,
                                                     const uint32_t* __restrict__ first, int64_t c,
                                                     const unsigned long long* __restrict__ box,
                                                     double* __restrict__ partial)
{
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6), total = first[c];
    for (uint32_t t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < total; t += waves) {
        const int64_t seg = seg_of_chunk(first, c, t);
        const uint32_t s = start[seg], len = start[seg + 1] - s;
        const uint32_t at = (t - first[seg]) * (uint32_t)NM_SEGMENT_CHUNK;
        const uint32_t cnt = len - at < (uint32_t)NM_SEGMENT_CHUNK ? len - at : (uint32_t)NM_SEGMENT_CHUNK;
        const unsigned long long* b = box + seg * SEG_BOX_WORDS;
        const double px = seg_dec(b[2]), py = seg_dec(b[3]), pz = seg_dec(b[4]);
        // the gathers first, all in flight together; then the sums in their order
        double q[SEG_SLOT_ROWS][3], w[SEG_SLOT_ROWS];
#pragma unroll
        for (int k = 0; k < SEG_SLOT_ROWS; ++k) {
            const uint32_t i = (uint32_t)lane + 64u * k;
            q[k][0] = px; q[k][1] = py; q[k][2] = pz;
            w[k] = 0.0;
            if (i < cnt) {
                const int64_t row = (int64_t)rows[s + at + i];
                const double* p = xyz + row * stride;
                q[k][0] = p[0]; q[k][1] = p[1]; q[k][2] = p[2];
                w[k] = weight ? (double)weight[row] : 1.0;
            }
        }
        double S[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = 0.0;
#pragma unroll
        for (int k = 0; k < SEG_SLOT_ROWS; ++k) seg_add_row(S, w[k], q[k][0] - px, q[k][1] - py, q[k][2] - pz);
        seg_tree<64>(S);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) partial[(int64_t)t * 9 + k] = S[k];
        }
    }
}

// ---- stage 5 -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_seg_finish(const uint32_t* __restrict__ first, int64_t c,
                                                    const unsigned long long* __restrict__ box,
                                                    const double* __restrict__ partial, double* __restrict__ table,
                                                    int64_t tstride)
{
    const int lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * (blockDim.x >> 6), total = first[c];
    for (uint32_t t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < total; t += waves) {
        const int64_t seg = seg_of_chunk(first, c, t);
        if (first[seg] != t) continue;          // the wave of the segment's first chunk does the segment
        const uint32_t nch = first[seg + 1] - t;
        double S[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = 0.0;
        // four partials of a slot in flight at a time; they are added in their order (an absent one is +0)
        for (uint32_t i = (uint32_t)lane; i < nch; i += 256u) {
            double v[4][9];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t at = i + 64u * u;
                const double* p = partial + (int64_t)(t + (at < nch ? at : i)) * 9;
#pragma unroll
                for (int k = 0; k < 9; ++k) v[u][k] = p[k];
                if (at >= nch) {
#pragma unroll
                    for (int k = 0; k < 9; ++k) v[u][k] = 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < 9; ++k) S[k] += v[u][k];
        }
        seg_tree<64>(S);
        if (lane == 0) {
            const unsigned long long* b = box + seg * SEG_BOX_WORDS;
            const int64_t n = (int64_t)b[0];
            const uint32_t r = (uint32_t)b[1];
            double mn[3], mx[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                mn[a] = seg_dec(b[2 + a]);
                mx[a] = seg_dec(b[5 + a]);
            }
            seg_write_row(n, r, mn, mx, S, table + seg * tstride);
        }
    }
}

__global__ __launch_bounds__(256) void k_seg_zero(double* __restrict__ table, int64_t c, int64_t tstride)
{
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= c * NM_SEGMENT_COLUMNS) return;
    const int64_t seg = t / NM_SEGMENT_COLUMNS;
    table[seg * tstride + (t - seg * NM_SEGMENT_COLUMNS)] = 0.0;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------
static bool seg_size_ok(int64_t v) { return v >= 0 && v < (int64_t)1 << 31; }

extern "C" size_t nm_segment_table_workspace_bytes(int64_t n, int64_t n_segments)
{
    if (!seg_size_ok(n) || !seg_size_ok(n_segments)) return 0;
    return seg_plan(n, n_segments).bytes;
}

extern "C" int nm_segment_table(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride, const int64_t* d_label,
                                int64_t n_segments, const int64_t* d_weight, double* d_table, int64_t table_stride,
                                void* d_tmp, size_t tmp_bytes, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    const int64_t c = n_segments;
    if (!seg_size_ok(n) || !seg_size_ok(c) || stride < 3 || table_stride < NM_SEGMENT_COLUMNS ||
        (n > 0 && (!d_xyz || !d_label)) || (c > 0 && !d_table))
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_segment_table: bad arguments");
    if (c == 0) return NM_OK;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        k_seg_zero<<<(unsigned)((c * NM_SEGMENT_COLUMNS + 255) / 256), 256, 0, s>>>(d_table, c, table_stride);
        NM_HIP(ctx, hipGetLastError());
        return NM_OK;
    }
    const SegPlan P = seg_plan(n, c);
    if (!d_tmp || tmp_bytes < P.bytes) NM_FAIL(ctx, NM_ERR_WORKSPACE, "nm_segment_table: workspace too small");
    // (256-byte aligned pieces whatever the caller's pointer: P.bytes has the room)
    char* w = (char*)(((uintptr_t)d_tmp + 255) / 256 * 256);
    uint32_t* key_in = (uint32_t*)(w + P.off_key_in);
    uint32_t* key_out = (uint32_t*)(w + P.off_key_out);
    uint32_t* row_in = (uint32_t*)(w + P.off_row_in);
    uint32_t* row_out = (uint32_t*)(w + P.off_row_out);
    uint32_t* start = (uint32_t*)(w + P.off_start);
    uint32_t* first = (uint32_t*)(w + P.off_first);
    unsigned long long* box = (unsigned long long*)(w + P.off_box);
    unsigned long long* chunk_box = (unsigned long long*)(w + P.off_chunk_box);
    double* partial = (double*)(w + P.off_partial);

    unsigned bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) <= c) ++bits;        // keys are 0 .. c
    k_seg_keys<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_label, n, c, key_in, row_in);
    size_t sort_bytes = P.sort_bytes;
    NM_HIP(ctx, rocprim::radix_sort_pairs(w + P.off_sort, sort_bytes, key_in, key_out, row_in, row_out, (size_t)n, 0,
                                          bits, s));
    k_seg_starts<<<(unsigned)((c + 1 + 255) / 256), 256, 0, s>>>(key_out, n, c, start);
    // whole 8-lane groups for segments 0 .. c (the last one only ends the chunk counts)
    k_seg_short<<<(unsigned)(((c + 1) * SEG_SHORT + 255) / 256), 256, 0, s>>>(
        d_xyz, stride, d_weight, row_out, start, c, first, d_table, table_stride);
    size_t scan_bytes = P.scan_bytes;
    NM_HIP(ctx, rocprim::exclusive_scan(w + P.off_scan, scan_bytes, first, first, 0u, (size_t)(c + 1),
                                        rocprim::plus<uint32_t>(), s));
    if (P.max_chunks > 0) {
        const int64_t want = (P.max_chunks + 3) / 4;
        const unsigned blocks = (unsigned)(want < SEG_MAX_BLOCKS ? want : SEG_MAX_BLOCKS);
        k_seg_box<<<blocks, 256, 0, s>>>(d_xyz, stride, d_weight, row_out, start, first, c, chunk_box);
        k_seg_box_join<<<blocks, 256, 0, s>>>(first, c, chunk_box, box);
        k_seg_moments<<<blocks, 256, 0, s>>>(d_xyz, stride, d_weight, row_out, start, first, c, box, partial);
        k_seg_finish<<<blocks, 256, 0, s>>>(first, c, box, partial, d_table, table_stride);
    }
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}
