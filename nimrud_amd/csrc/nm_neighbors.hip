// nm_neighbors.hip - neighbor lists from a dense occupancy index with a voxel-rank table.
//
// the reference names a search voxel by its position in np.unique of the addresses (geometry.py:148-150) and
// gathers by it (multiscale.py:103).  a leaf row-word holds 32 consecutive addresses (x is the low address field),
// so that position is  rank[row-word] + popc(word & bits below)  once rank[] holds, per row-word, the number of
// occupied cells with a smaller address.  the index is built ONCE per (search cloud, lattice) and then queried
// for any number of query clouds and radii: no sort, no address array, no search.
// on the same index, attributes: the voxel of a point (np.unique's inverse), the rows of every voxel, per-voxel
// reductions of per-point columns, and per-neighborhood count / mean / min / max of a voxel table without a list.
// and the graph itself: the connected components of the voxels under "within r", by a lock-free union-find, and its
// density-based clusters (DBSCAN): a density walk, the same union-find on the core voxels, a border walk.
// and the graph of a labelling's segments: which of them touch, over how many edges, at which saddle (adjacency).
// and path length over the graph: the shortest way from a set of seeds to every voxel, by relaxation sweeps (geodesic).
//
// workspace (nm_neighbor_index_workspace_bytes), S = superblocks of the lattice (at most 2^NM_DENSE_LOG2):
//   header  256 B      [0] M, written by the scan
//   leaves  S * 256 B  the dense index: 64 row-words per superblock, leaf number = nm_sb_key
//   totals  NT * 4 B   occupied cells per piece of a lattice row, in ADDRESS order; scanned in place
//   partial 8 KB       the scan's per-block sums
//   rank    S * 256 B  one word per row-word, same layout as the leaves
#include "nm_common.h"

namespace {

constexpr int NBR_CHUNK_LOG2 = 4;                 // leaves of one (sbz, sby) strip a wave walks: 16
constexpr int NBR_CHUNK = 1 << NBR_CHUNK_LOG2;
constexpr int NBR_SCAN_THREADS = 256;
constexpr int NBR_SCAN_ITEMS = 16;
constexpr int NBR_SCAN_TILE = NBR_SCAN_THREADS * NBR_SCAN_ITEMS;      // 4096 totals
constexpr int NBR_SCAN_MAX_BLOCKS = 2048;
constexpr size_t NBR_HEADER_BYTES = 256;

// address order is (gz, gy, gx) = (sbz, lz, sby, ly, sbx, lx); leaf order is (sbz, sbx, sby) and a leaf's words
// run (lz, ly).  a lattice row (gz, gy) crosses 2^bx leaves; it is cut into pieces of NBR_CHUNK leaves so that
// a long thin lattice still has work for every wave.  totals[] has one entry per piece, in address order:
// index = (gz * rows_y + gy) * pieces + piece.
struct NbrPlan {
    uint64_t superblocks;
    int32_t chunk_log2;      // leaves per piece: min(bx, NBR_CHUNK_LOG2) bits
    int32_t piece_bits;      // bx - chunk_log2
    int64_t units;           // (sbz, sby, piece) triples: one wave each
    int64_t totals;          // entries of totals[]
    int64_t totals_padded;   // rounded up to whole scan tiles (the pad stays zero)
    int32_t scan_blocks;
    int32_t tiles_per_block;
    size_t off_leaf, off_totals, off_partial, off_rank, bytes;
};

inline bool nbr_in_range(const LatticeDev& L) { return L.bx + L.by + L.bz <= NM_DENSE_LOG2; }

NbrPlan nbr_plan(const LatticeDev& L)
{
    NbrPlan P;
    P.superblocks = 1ull << (L.bx + L.by + L.bz);
    P.chunk_log2 = L.bx < NBR_CHUNK_LOG2 ? L.bx : NBR_CHUNK_LOG2;
    P.piece_bits = L.bx - P.chunk_log2;
    P.units = (int64_t)1 << (L.bz + L.by + P.piece_bits);
    P.totals = P.units * NM_LEAF_WORDS;
    const int64_t tiles = (P.totals + NBR_SCAN_TILE - 1) / NBR_SCAN_TILE;
    P.totals_padded = tiles * NBR_SCAN_TILE;
    P.scan_blocks = (int32_t)(tiles < NBR_SCAN_MAX_BLOCKS ? tiles : NBR_SCAN_MAX_BLOCKS);
    P.tiles_per_block = (int32_t)((tiles + P.scan_blocks - 1) / P.scan_blocks);
    const size_t leaf_bytes = (size_t)P.superblocks * NM_LEAF_WORDS * 4;
    P.off_leaf = NBR_HEADER_BYTES;
    P.off_totals = P.off_leaf + leaf_bytes;
    P.off_partial = P.off_totals + (size_t)P.totals_padded * 4;
    P.off_rank = P.off_partial + (size_t)NBR_SCAN_MAX_BLOCKS * 4;
    P.bytes = P.off_rank + leaf_bytes;
    return P;
}

// candidates per axis for a radius / edge ratio: nm_features.hip's candidate_width, restated here because that
// translation unit keeps it to itself.  a superset is harmless: every candidate is tested exactly.
int nbr_candidate_width(double radius, double edge, int32_t* dmin)
{
    double rho = radius / edge;
    double m = floor(rho + 0.5 + 1e-9);
    if (!(m >= 0.0) || m > 1000.0) return -1;
    *dmin = -(int32_t)m;
    return 2 * (int32_t)m + 1;
}

// ---- build: the cell of every search point, one atomicOr into its row-word --------------------------------------
__global__ __launch_bounds__(256) void k_nbr_build(const double* __restrict__ xyz, int64_t n, int64_t stride,
                                                   LatticeDev L, uint32_t* __restrict__ leaf,
                                                   int64_t* __restrict__ oob_count)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    bool oob = false;
    if (i < n) {
        const double* p = xyz + i * stride;
        const double fx = nm_cell_f(p[0], L.min_x, L.edge);
        const double fy = nm_cell_f(p[1], L.min_y, L.edge);
        const double fz = nm_cell_f(p[2], L.min_z, L.edge);
        // the contract of nm_voxelize's d_count[1] (k_addresses); NaN coordinates fail every comparison: outside
        const bool in = fx >= 0.0 && fy >= 0.0 && fz >= 0.0 && fx < (double)(1u << L.wx) &&
                        fy < (double)(1u << L.wy) && fz < (double)(1u << L.wz);
        oob = !in;
        if (in) {
            const uint32_t cx = (uint32_t)fx, cy = (uint32_t)fy, cz = (uint32_t)fz;
            const uint64_t sb = nm_sb_key(cx >> NM_SBX_BITS, cy >> NM_SBY_BITS, cz >> NM_SBZ_BITS, L);
            atomicOr(&leaf[sb * NM_LEAF_WORDS + (((cz & 7u) << 3) | (cy & 7u))], 1u << (cx & 31u));
        }
    }
    const unsigned long long m = __ballot(oob);
    if (m && (threadIdx.x & 63) == 0)
        atomicAdd((unsigned long long*)oob_count, (unsigned long long)__popcll(m));
}

// ---- rank table ---------------------------------------------------------------------------------------------------
// one wave per (sbz, sby, piece): lane w = lz*8 + ly holds row-word w of every leaf it walks, so each leaf is one
// 256-byte read of the wave.  the walk's loads are issued together (the leaves are a fixed stride apart).
// first_leaf: the leaf of the piece's first superblock; total_at: where this lane's piece of a row sits in totals[]
__device__ __forceinline__ bool nbr_unit(const LatticeDev& L, int32_t chunk_log2, int32_t piece_bits, int64_t units,
                                         int lane, uint64_t* first_leaf, int64_t* total_at)
{
    const int64_t u = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (u >= units) return false;
    const uint32_t piece = (uint32_t)(u & (((int64_t)1 << piece_bits) - 1));
    const uint32_t sby = (uint32_t)((u >> piece_bits) & ((1u << L.by) - 1u));
    const uint32_t sbz = (uint32_t)(u >> (piece_bits + L.by));
    *first_leaf = nm_sb_key(piece << chunk_log2, sby, sbz, L);
    const int64_t gz = ((int64_t)sbz << 3) | (lane >> 3), gy = ((int64_t)sby << 3) | (lane & 7);
    *total_at = (((gz << (L.by + 3)) | gy) << piece_bits) | piece;
    return true;
}

__global__ __launch_bounds__(256) void k_nbr_row_totals(const uint32_t* __restrict__ leaf, LatticeDev L,
                                                        int32_t chunk_log2, int32_t piece_bits, int64_t units,
                                                        uint32_t* __restrict__ totals)
{
    const int lane = threadIdx.x & 63;
    uint64_t first;
    int64_t at;
    if (!nbr_unit(L, chunk_log2, piece_bits, units, lane, &first, &at)) return;
    const int32_t leaves = 1 << chunk_log2;
    const uint64_t step = (uint64_t)NM_LEAF_WORDS << L.by;        // the next superblock along x
    const uint32_t* p = leaf + first * NM_LEAF_WORDS + lane;
    uint32_t v[NBR_CHUNK];
#pragma unroll
    for (int i = 0; i < NBR_CHUNK; ++i) v[i] = i < leaves ? p[(uint64_t)i * step] : 0u;
    uint32_t t = 0;
#pragma unroll
    for (int i = 0; i < NBR_CHUNK; ++i) t += (uint32_t)__popc(v[i]);
    totals[at] = t;
}

__global__ __launch_bounds__(256) void k_nbr_rank(const uint32_t* __restrict__ leaf, LatticeDev L,
                                                  int32_t chunk_log2, int32_t piece_bits, int64_t units,
                                                  const uint32_t* __restrict__ totals, uint32_t* __restrict__ rank)
{
    const int lane = threadIdx.x & 63;
    uint64_t first;
    int64_t at;
    if (!nbr_unit(L, chunk_log2, piece_bits, units, lane, &first, &at)) return;
    const int32_t leaves = 1 << chunk_log2;
    const uint64_t step = (uint64_t)NM_LEAF_WORDS << L.by;
    const uint64_t base = first * NM_LEAF_WORDS + lane;
    uint32_t v[NBR_CHUNK];
#pragma unroll
    for (int i = 0; i < NBR_CHUNK; ++i) v[i] = i < leaves ? leaf[base + (uint64_t)i * step] : 0u;
    uint32_t run = totals[at];       // (scanned: occupied cells before this piece of the row)
#pragma unroll
    for (int i = 0; i < NBR_CHUNK; ++i)
        if (i < leaves) {
            rank[base + (uint64_t)i * step] = run;
            run += (uint32_t)__popc(v[i]);
        }
}

// ---- flat exclusive scan of totals[], two launches (the shape of nm_order.hip's k_scan_reduce / k_scan_apply) ----
__device__ __forceinline__ uint32_t nbr_block_sum(uint32_t v, uint32_t* wsum)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
    for (int w = 0; w < NBR_SCAN_THREADS / 64; ++w) t += wsum[w];
    return t;
}

__global__ __launch_bounds__(NBR_SCAN_THREADS) void k_nbr_scan_reduce(const uint32_t* __restrict__ totals,
                                                                      int32_t tiles_per_block,
                                                                      int64_t len, uint32_t* __restrict__ partial)
{
    __shared__ uint32_t wsum[NBR_SCAN_THREADS / 64];
    uint32_t s = 0;
    for (int32_t t = 0; t < tiles_per_block; ++t) {
        const int64_t at = ((int64_t)blockIdx.x * tiles_per_block + t) * NBR_SCAN_TILE +
                           (int64_t)threadIdx.x * NBR_SCAN_ITEMS;
        if (at >= len) break;        // len is a multiple of the tile
        const uint4* p = (const uint4*)(totals + at);
#pragma unroll
        for (int q = 0; q < NBR_SCAN_ITEMS / 4; ++q) {
            const uint4 v = p[q];
            s += v.x + v.y + v.z + v.w;
        }
    }
    const uint32_t sum = nbr_block_sum(s, wsum);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(NBR_SCAN_THREADS) void k_nbr_scan_apply(uint32_t* __restrict__ totals,
                                                                     int32_t tiles_per_block, int64_t len,
                                                                     const uint32_t* __restrict__ partial,
                                                                     uint32_t* __restrict__ header,
                                                                     int64_t* __restrict__ d_count)
{
    __shared__ uint32_t wsum[NBR_SCAN_THREADS / 64];
    __shared__ uint32_t wpre[NBR_SCAN_THREADS / 64];
    // everything before this block's tiles; block 0 also adds up the rest: M
    uint32_t before = 0, rest = 0;
    const int nb = (int)gridDim.x;
    for (int b = threadIdx.x; b < nb; b += NBR_SCAN_THREADS) {
        const uint32_t v = (b < (int)blockIdx.x || blockIdx.x == 0) ? partial[b] : 0u;
        if (b < (int)blockIdx.x) before += v;
        else rest += v;
    }
    before = nbr_block_sum(before, wsum);
    if (blockIdx.x == 0) {
        rest = nbr_block_sum(rest, wsum);
        if (threadIdx.x == 0) {
            header[0] = rest;
            d_count[0] = (int64_t)rest;
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int32_t t = 0; t < tiles_per_block; ++t) {
        const int64_t at = ((int64_t)blockIdx.x * tiles_per_block + t) * NBR_SCAN_TILE +
                           (int64_t)threadIdx.x * NBR_SCAN_ITEMS;
        if (at >= len) break;        // (the same for every thread of the block: len is a multiple of the tile)
        uint32_t v[NBR_SCAN_ITEMS];
        uint32_t s = 0;
        uint4* p = (uint4*)(totals + at);
#pragma unroll
        for (int q = 0; q < NBR_SCAN_ITEMS / 4; ++q) {
            const uint4 x = p[q];
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
            s += x.x + x.y + x.z + x.w;
        }
        uint32_t incl = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        __syncthreads();       // the readers of wsum / wpre of the round before are done
        if (lane == 63) wpre[w] = incl;
        __syncthreads();
        uint32_t run = before + incl - s;
        uint32_t tile_sum = 0;
        for (int ww = 0; ww < NBR_SCAN_THREADS / 64; ++ww) {
            if (ww < w) run += wpre[ww];
            tile_sum += wpre[ww];
        }
#pragma unroll
        for (int q = 0; q < NBR_SCAN_ITEMS / 4; ++q) {
            uint4 x;
            x.x = run; run += v[4 * q];
            x.y = run; run += v[4 * q + 1];
            x.z = run; run += v[4 * q + 2];
            x.w = run; run += v[4 * q + 3];
            p[q] = x;
        }
        before += tile_sum;
    }
}

// ---- addresses: every set bit writes its address at its rank ----------------------------------------------------------
__global__ __launch_bounds__(256) void k_nbr_addresses(const uint32_t* __restrict__ leaf,
                                                       const uint32_t* __restrict__ rank,
                                                       const uint32_t* __restrict__ header, LatticeDev L,
                                                       uint64_t words, int64_t* __restrict__ out, uint32_t room)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= words) return;
    uint32_t word = leaf[i];
    if (!word) return;
    const uint32_t m = min(header[0], room);       // (room: entries `out` has; the caller's promise, or a scratch's size)
    const uint64_t sb = i >> (NM_SBY_BITS + NM_SBZ_BITS);
    const uint32_t w = (uint32_t)i & (NM_LEAF_WORDS - 1);
    const int64_t sby = (int64_t)(sb & ((1ull << L.by) - 1ull));
    const int64_t sbx = (int64_t)((sb >> L.by) & ((1ull << L.bx) - 1ull));
    const int64_t sbz = (int64_t)(sb >> (L.bx + L.by));
    const int64_t gy = (sby << 3) | (w & 7u), gz = (sbz << 3) | (w >> 3);
    const int64_t a0 = (sbx << NM_SBX_BITS) + (gy << L.s0) + (gz << L.s1);
    uint32_t pos = rank[i];
    while (word) {
        const int bit = __ffs((int)word) - 1;
        word &= word - 1u;
        if (pos < m) out[pos] = a0 + bit;      // (always, for a workspace built for this lattice)
        ++pos;
    }
}

// ---- the window walk: one lane per query ---------------------------------------------------------------------------
// z outer, y inner, x inside the word: ascending address = ascending rank, so hit(voxel) is called in ascending
// voxel order.  shared by the lists and the neighborhood statistics: same clamped home cell, same clipping, same
// row skip, same unfused test.  nbr_walk_d2 hands hit(voxel, d2) the squared distance it tested as well; nbr_walk is
// the same walk for a callback that has no use for it
template <typename F>
__device__ __forceinline__ void nbr_walk_d2(double qx, double qy, double qz, const uint32_t* __restrict__ leaf,
                                            const uint32_t* __restrict__ rank, const LatticeDev& L, double r2,
                                            int32_t dmin, int32_t W, F&& hit)
{
    const int32_t hx = nm_clamp_cell(nm_cell_f(qx, L.min_x, L.edge));
    const int32_t hy = nm_clamp_cell(nm_cell_f(qy, L.min_y, L.edge));
    const int32_t hz = nm_clamp_cell(nm_cell_f(qz, L.min_z, L.edge));
    // the window clipped to the lattice (home cells are clamped to +-2^30 and |dmin| <= 1000: no overflow)
    const int32_t x0 = max(hx + dmin, 0), x1 = min(hx + dmin + W - 1, (1 << L.wx) - 1);
    const int32_t y0 = max(hy + dmin, 0), y1 = min(hy + dmin + W - 1, (1 << L.wy) - 1);
    const int32_t z0 = max(hz + dmin, 0), z1 = min(hz + dmin + W - 1, (1 << L.wz) - 1);
    if (x0 > x1) return;
    for (int32_t gz = z0; gz <= z1; ++gz) {
        double d = qz - nm_centre(gz, L.min_z, L.edge, L.half_edge);
        const double dz2 = d * d;
        for (int32_t gy = y0; gy <= y1; ++gy) {
            d = qy - nm_centre(gy, L.min_y, L.edge, L.half_edge);
            const double dy2 = d * d;
            // dx*dx >= 0 and rounding is monotonic: ((dx*dx + dy2) + dz2) >= fl(dy2 + dz2), so a row this
            // far away holds no neighbor whatever its words say
            if (!(dy2 + dz2 <= r2)) continue;
            const uint32_t wrow = (((uint32_t)gz & 7u) << 3) | ((uint32_t)gy & 7u);
            for (int32_t sbx = x0 >> NM_SBX_BITS; sbx <= (x1 >> NM_SBX_BITS); ++sbx) {
                const uint64_t at = nm_sb_key((uint32_t)sbx, (uint32_t)gy >> NM_SBY_BITS,
                                              (uint32_t)gz >> NM_SBZ_BITS, L) * NM_LEAF_WORDS + wrow;
                const uint32_t all = leaf[at];
                // mask to the x-window
                const int32_t base = sbx << NM_SBX_BITS;
                const int32_t lo = max(x0 - base, 0), hi = min(x1 - base, 31);
                uint32_t word = all & (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo);
                if (!word) continue;
                const uint32_t r0 = rank[at];
                while (word) {
                    const int bit = __ffs((int)word) - 1;
                    word &= word - 1u;
                    d = qx - nm_centre(base + bit, L.min_x, L.edge, L.half_edge);
                    const double s = (d * d + dy2) + dz2;
                    if (!(s <= r2)) continue;
                    hit(r0 + (uint32_t)__popc(all & ((1u << bit) - 1u)), s);
                }
            }
        }
    }
}

template <typename F>
__device__ __forceinline__ void nbr_walk(double qx, double qy, double qz, const uint32_t* __restrict__ leaf,
                                         const uint32_t* __restrict__ rank, const LatticeDev& L, double r2,
                                         int32_t dmin, int32_t W, F&& hit)
{
    nbr_walk_d2(qx, qy, qz, leaf, rank, L, r2, dmin, W, [&](uint32_t voxel, double) { hit(voxel); });
}

// ---- lists: the voxels the walk finds, counted or written at the query's offset ---------------------------------
__global__ __launch_bounds__(256) void k_nbr_lists(const double* __restrict__ query, int64_t nq, int64_t qstride,
                                                   const uint32_t* __restrict__ leaf,
                                                   const uint32_t* __restrict__ rank, LatticeDev L, double r2,
                                                   int32_t dmin, int32_t W, int32_t* __restrict__ count,
                                                   const int64_t* __restrict__ offsets,
                                                   int64_t* __restrict__ index)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const double* p = query + q * qstride;
    int32_t n = 0;
    int64_t* out = index ? index + offsets[q] : nullptr;
    nbr_walk(p[0], p[1], p[2], leaf, rank, L, r2, dmin, W, [&](uint32_t voxel) {
        if (out) out[n] = (int64_t)voxel;
        ++n;
    });
    if (count) count[q] = n;
}

// ---- point -> voxel: the np.unique inverse -------------------------------------------------------------------------
// one lane per point: its cell by the reference's own division (as k_nbr_build), the row-word and its rank.
// -1 outside the lattice on any axis (NaN coordinates fail every comparison) and in a cell nobody occupies
__global__ __launch_bounds__(256) void k_nbr_voxel_of(const double* __restrict__ xyz, int64_t n, int64_t stride,
                                                      LatticeDev L, const uint32_t* __restrict__ leaf,
                                                      const uint32_t* __restrict__ rank,
                                                      int64_t* __restrict__ voxel)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* p = xyz + i * stride;
    const double fx = nm_cell_f(p[0], L.min_x, L.edge);
    const double fy = nm_cell_f(p[1], L.min_y, L.edge);
    const double fz = nm_cell_f(p[2], L.min_z, L.edge);
    const bool in = fx >= 0.0 && fy >= 0.0 && fz >= 0.0 && fx < (double)(1u << L.wx) &&
                    fy < (double)(1u << L.wy) && fz < (double)(1u << L.wz);
    int64_t v = -1;
    if (in) {
        const uint32_t cx = (uint32_t)fx, cy = (uint32_t)fy, cz = (uint32_t)fz;
        const uint64_t at = nm_sb_key(cx >> NM_SBX_BITS, cy >> NM_SBY_BITS, cz >> NM_SBZ_BITS, L) * NM_LEAF_WORDS +
                            (((cz & 7u) << 3) | (cy & 7u));
        const uint32_t word = leaf[at], bit = cx & 31u;
        if ((word >> bit) & 1u) v = (int64_t)(rank[at] + (uint32_t)__popc(word & ((1u << bit) - 1u)));
    }
    voxel[i] = v;
}

// ---- grouping: the rows of every voxel, ascending ----------------------------------------------------------------
// tmp (nm_neighbor_index_group_workspace_bytes), n rows into m voxels:
//   header  256 B                  word 0: the scan's total; bytes 16..23: the same as int64 (the scan writes both);
//                                  word 8: number of long segments
//   partial 8 KB                   the scan's per-block sums
//   longs   (n / 64 + 1) * 4 B     the voxels with more than GRP_SHORT rows (there are at most n / 65)
//   cursor  pad4096(m) * 4 B       per voxel: its count, then (scanned in place) its start, then its fill cursor
constexpr int GRP_SHORT = 64;           // a segment up to here is ordered by one thread, in place
constexpr int GRP_LDS_ROWS = 8192;      // a longer one by a block: in LDS up to here (32 KB), else in memory
constexpr int GRP_LONG_BLOCKS = 1024;
constexpr int GRP_HEAD_LONGS = 8;

struct GrpPlan {
    int64_t cursor_len;          // m rounded up to whole scan tiles
    int32_t scan_blocks, tiles_per_block;
    size_t off_partial, off_longs, off_cursor, bytes;
};

GrpPlan grp_plan(int64_t n, int64_t m)
{
    GrpPlan G;
    const int64_t tiles = m > 0 ? (m + NBR_SCAN_TILE - 1) / NBR_SCAN_TILE : 1;
    G.cursor_len = tiles * NBR_SCAN_TILE;
    G.scan_blocks = (int32_t)(tiles < NBR_SCAN_MAX_BLOCKS ? tiles : NBR_SCAN_MAX_BLOCKS);
    G.tiles_per_block = (int32_t)((tiles + G.scan_blocks - 1) / G.scan_blocks);
    G.off_partial = NBR_HEADER_BYTES;
    G.off_longs = G.off_partial + (size_t)NBR_SCAN_MAX_BLOCKS * 4;
    G.off_cursor = G.off_longs + ((size_t)(n / 64 + 1) * 4 + 15) / 16 * 16;     // (16-byte loads of the scan)
    G.bytes = G.off_cursor + (size_t)G.cursor_len * 4;
    return G;
}

__global__ __launch_bounds__(256) void k_grp_zero(uint32_t* __restrict__ header, uint32_t* __restrict__ cursor,
                                                  int64_t len)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < (int64_t)(NBR_HEADER_BYTES / 4)) header[i] = 0u;
    if (i < len) cursor[i] = 0u;
}

// integer atomics on the voxel number: exact, whatever the order.  rows of no voxel (-1, or a number past m)
// are in no segment
__global__ __launch_bounds__(256) void k_grp_count(const int64_t* __restrict__ voxel, int64_t n, int64_t m,
                                                   uint32_t* __restrict__ cursor)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t v = voxel[i];
    if (v >= 0 && v < m) atomicAdd(&cursor[v], 1u);
}

__global__ __launch_bounds__(256) void k_grp_put_counts(const uint32_t* __restrict__ cursor, int64_t m,
                                                        int64_t* __restrict__ counts)
{
    const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (v < m) counts[v] = (int64_t)cursor[v];
}

__global__ __launch_bounds__(256) void k_grp_put_start(const uint32_t* __restrict__ cursor,
                                                       const uint32_t* __restrict__ header, int64_t m,
                                                       int64_t* __restrict__ start)
{
    const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (v < m) start[v] = (int64_t)cursor[v];
    if (v == m) start[m] = (int64_t)header[0];
}

// every row takes the next place of its voxel's segment: whichever comes first.  the order is put right below
__global__ __launch_bounds__(256) void k_grp_fill(const int64_t* __restrict__ voxel, int64_t n, int64_t m,
                                                  uint32_t* __restrict__ cursor, int64_t* __restrict__ rows)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t v = voxel[i];
    if (v >= 0 && v < m) rows[atomicAdd(&cursor[v], 1u)] = i;
}

// one thread per voxel: a short segment by insertion, in place; a long one is put on the list
__global__ __launch_bounds__(256) void k_grp_order_short(const int64_t* __restrict__ start, int64_t m,
                                                         int64_t* __restrict__ rows,
                                                         uint32_t* __restrict__ header,
                                                         uint32_t* __restrict__ longs)
{
    const int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (v >= m) return;
    const int64_t s = start[v];
    const int32_t len = (int32_t)(start[v + 1] - s);
    if (len > GRP_SHORT) {
        longs[atomicAdd(&header[GRP_HEAD_LONGS], 1u)] = (uint32_t)v;
        return;
    }
    int64_t* a = rows + s;
    for (int32_t i = 1; i < len; ++i) {
        const int64_t x = a[i];
        int32_t j = i;
        while (j > 0 && a[j - 1] > x) {
            a[j] = a[j - 1];
            --j;
        }
        a[j] = x;
    }
}

// bitonic network of a block over a[0 .. len), every comparator leaves the smaller value at the smaller place
// (the merges start with a flip), so the places from len up to the next power of two act as +infinity without
// existing: a comparator that reaches one does nothing.  len * log2(len)^2 / 4 comparators in all, a 256th of
// them per thread - whatever the values are
template <typename T>
__device__ __forceinline__ void grp_bitonic(T* a, uint32_t len)
{
    uint32_t p = 1;
    while (p < len) p <<= 1;
    const uint32_t half = p >> 1;
    for (uint32_t k = 2; k <= p; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const bool flip = j == (k >> 1);
            for (uint32_t i = threadIdx.x; i < half; i += blockDim.x) {
                const uint32_t lo = ((i / j) * (j << 1)) + (i % j);
                const uint32_t hi = flip ? (lo - (i % j)) + (k - 1u) - (i % j) : lo + j;
                if (hi < len) {
                    const T x = a[lo], y = a[hi];
                    if (x > y) {
                        a[lo] = y;
                        a[hi] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// one block per long segment (the blocks share the list out)
__global__ __launch_bounds__(256) void k_grp_order_long(const int64_t* __restrict__ start, int64_t* __restrict__ rows,
                                                        const uint32_t* __restrict__ header,
                                                        const uint32_t* __restrict__ longs)
{
    __shared__ uint32_t tile[GRP_LDS_ROWS];
    const uint32_t n_long = header[GRP_HEAD_LONGS];
    for (uint32_t at = blockIdx.x; at < n_long; at += gridDim.x) {
        const uint32_t v = longs[at];
        const int64_t s = start[v];
        const uint32_t len = (uint32_t)(start[v + 1] - s);
        int64_t* a = rows + s;
        if (len <= GRP_LDS_ROWS) {
            for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) tile[i] = (uint32_t)a[i];     // rows < 2^31
            __syncthreads();
            grp_bitonic(tile, len);
            for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) a[i] = (int64_t)tile[i];
        } else {
            __syncthreads();       // (the fill's stores are another kernel's; this orders the rounds of the loop)
            grp_bitonic(a, len);
        }
        __syncthreads();
    }
}

// ---- voxel table: one thread per (voxel, column), the segment left to right ----------------------------------------
enum { GRP_MEAN = NM_REDUCE_MEAN, GRP_SUM = NM_REDUCE_SUM, GRP_MIN = NM_REDUCE_MIN, GRP_MAX = NM_REDUCE_MAX };

// sum: ((0 + a[r0]) + a[r1]) + ... in ascending row order - np.bincount(inverse, weights=column); mean: that sum,
// divided once by the count.  a voxel without rows gives 0
template <int OP>
__global__ __launch_bounds__(256) void k_nbr_voxel_reduce(const int64_t* __restrict__ start,
                                                          const int64_t* __restrict__ rows, int64_t m,
                                                          const double* __restrict__ attr, int64_t astride,
                                                          int32_t dims, double* __restrict__ out)
{
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= m * dims) return;
    const int64_t v = t / dims;
    const int32_t c = (int32_t)(t - v * dims);
    const int64_t s = start[v], e = start[v + 1];
    double acc = 0.0;
    if (OP == GRP_MEAN || OP == GRP_SUM) {
        for (int64_t i = s; i < e; ++i) acc += attr[rows[i] * astride + c];
        if (OP == GRP_MEAN && e > s) acc = acc / (double)(e - s);
    } else if (e > s) {
        acc = attr[rows[s] * astride + c];
        for (int64_t i = s + 1; i < e; ++i) {
            const double x = attr[rows[i] * astride + c];
            if (OP == GRP_MIN ? x < acc : x > acc) acc = x;
        }
    }
    out[t] = acc;
}

// ---- neighborhood statistics: the lists' walk, nothing list-shaped written ---------------------------------------------
// per included voxel the D values of its table row: count, sum left to right in ascending voxel order, running
// minimum and maximum, all in registers (DB = the compile-time bucket dims falls in)
template <int DB>
__global__ __launch_bounds__(256) void k_nbr_stats(const double* __restrict__ query, int64_t nq, int64_t qstride,
                                                   const uint32_t* __restrict__ leaf,
                                                   const uint32_t* __restrict__ rank, LatticeDev L, double r2,
                                                   int32_t dmin, int32_t W, const double* __restrict__ values,
                                                   int64_t vstride, int32_t dims, int32_t* __restrict__ count,
                                                   double* __restrict__ mean, double* __restrict__ vmin,
                                                   double* __restrict__ vmax, int64_t ostride)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const double* p = query + q * qstride;
    double sum[DB], lo[DB], hi[DB];
#pragma unroll
    for (int c = 0; c < DB; ++c) sum[c] = lo[c] = hi[c] = 0.0;
    int32_t n = 0;
    nbr_walk(p[0], p[1], p[2], leaf, rank, L, r2, dmin, W, [&](uint32_t voxel) {
        const double* val = values + (int64_t)voxel * vstride;
        const bool first = n == 0;
#pragma unroll
        for (int c = 0; c < DB; ++c)
            if (c < dims) {
                const double x = val[c];
                sum[c] += x;
                lo[c] = (first || x < lo[c]) ? x : lo[c];
                hi[c] = (first || x > hi[c]) ? x : hi[c];
            }
        ++n;
    });
    if (count) count[q] = n;
    const double k = (double)n;
#pragma unroll
    for (int c = 0; c < DB; ++c)
        if (c < dims) {
            // no voxel in reach: zeros in all three tables
            if (mean) mean[q * ostride + c] = n ? sum[c] / k : 0.0;
            if (vmin) vmin[q * ostride + c] = lo[c];
            if (vmax) vmax[q * ostride + c] = hi[c];
        }
}

// ---- nearest: the k nearest occupied voxels of any point --------------------------------------------------------------
// one lane per query.  candidates are all M occupied voxels; a voxel's d2 is nbr_walk's ((dx*dx + dy*dy) + dz*dz)
// on nm_centre, voxels are ordered by (d2, voxel index) and a voxel qualifies when d2 <= r2 (NaN fails).
//
// the search examines cubes of growing half-width S around the clamped home cell h, shell by shell (the cells of
// cube S1 that are not in cube S0), and keeps the k best of everything it has examined.  after the cube of
// half-width S has been examined completely the list is FINAL when one of these holds:
//   (a) it holds k voxels and the k-th d2 is <= ((S + 1/2 - 1e-6) * e)^2.  the query lies in its home cell, so a
//       cell whose offset from h exceeds S on some axis has its centre more than (S + 1/2) * e away on that axis:
//       every cell outside the cube is strictly farther than the k-th voxel and cannot enter the list, not even
//       through the tie rule.  the 1e-6 margin (far above the rounding of the cell division and the centres)
//       keeps the comparison strict.  a query outside the lattice has its home cell clamped towards the lattice;
//       the cells beyond the cube then lie on the inner side only, where the query is at least as far from them
//       as a point of the clamped home cell would be.  (the bound k_knn_fallback uses.)
//   (b) S has reached the candidate window of the limit, nbr_candidate_width(max_distance, e): no cell outside
//       it holds a voxel within the limit - the window lists() walks.
//   (c) the cube covers the lattice: there is no cell outside.
// which S values are stepped through, and which kernel answers, changes the work and never the answer: the k
// smallest of a total order over a set that provably contains them.
//
// best list: K slots in registers (K = the compile-time bucket k falls in), sorted ascending, the fallback's
// branch-free insertion.  k < K uses the LAST k slots: the first K - k hold -infinity, which no candidate
// precedes, so the k-th best is always bd[K - 1] - no search for slot k - 1.  the tie key is the voxel index
// itself (rank[word] + popc(word below the bit)): it is the output, it is 32 bits whatever the cube's width (a
// cell-offset code needs 64 beyond +-511 cells, and the wide stage goes far beyond), and it does not depend on
// the home cell.  its rank word is loaded only for a word with a candidate that can enter the list.
//
// stages: k_nn_near takes every query up to cubes of half-width NN_NEAR_CAP.  a query that is not final by then
// is appended to a list in the caller's scratch (one atomic per wave) with the half-width it needs next, and
// k_nn_wide - one lane per LISTED query, so no finished lane waits - starts it again from that cube.  the wide
// stage skips empty space through the scanned totals[]: the occupied cells of any run of consecutive pieces (a
// piece = 2^chunk_log2 leaves of one lattice row) is the difference of two entries, M closing the last; it asks
// that per z-layer of the cube (all rows of the layer in the y-range, a superset), per row and per piece before
// it reads a leaf word.
constexpr int NN_NEAR_CAP = 8;
constexpr size_t NN_HEADER_BYTES = 256;          // word 0: number of listed queries

struct NnArgs {
    const double* query;
    int64_t nq, qstride;
    const uint32_t* leaf;
    const uint32_t* rank;
    const uint32_t* totals;      // scanned
    const uint32_t* header;      // [0] M
    LatticeDev L;
    int32_t chunk_log2, piece_bits;
    int64_t n_totals;
    int32_t k;
    int32_t s_limit;             // half-width of the limit's window, -1: no limit
    double r2;
    double* dist2;
    int64_t* index;
    int64_t ostride;
    int32_t* found;
    uint32_t* pend_count;
    uint2* pend;                 // {query, half-width to start from}
};

// occupied cells before piece i of the address order
__device__ __forceinline__ uint32_t nn_before(const NnArgs& A, uint32_t m, int64_t i)
{
    return i < A.n_totals ? A.totals[i] : m;
}

// searches query q from a full cube of half-width s_first on.  true: final, the row is written.  false: the
// next cube would be wider than `cap`; *hint is its half-width and nothing is written
template <int K, bool WIDE>
__device__ __forceinline__ bool nn_search(const NnArgs& A, int64_t q, int64_t s_first, int64_t cap, uint32_t* hint)
{
    const LatticeDev& L = A.L;
    const double* p = A.query + q * A.qstride;
    const double qx = p[0], qy = p[1], qz = p[2];
    const int32_t hx = nm_clamp_cell(nm_cell_f(qx, L.min_x, L.edge));
    const int32_t hy = nm_clamp_cell(nm_cell_f(qy, L.min_y, L.edge));
    const int32_t hz = nm_clamp_cell(nm_cell_f(qz, L.min_z, L.edge));
    const int32_t nx = (1 << L.wx) - 1, ny = (1 << L.wy) - 1, nz = (1 << L.wz) - 1;      // last cells
    // (c): the half-width at which the cube covers the lattice; (b): the limit's window
    int64_t s_end = max(max((int64_t)hx, (int64_t)nx - hx), max((int64_t)hy, (int64_t)ny - hy));
    s_end = max(s_end, max((int64_t)hz, (int64_t)nz - hz));
    if (A.s_limit >= 0 && A.s_limit < s_end) s_end = A.s_limit;
    const uint32_t m = WIDE ? A.header[0] : 0u;
    const int32_t pshift = NM_SBX_BITS + A.chunk_log2;

    double bd[K];
    uint32_t bi[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const bool real = t >= K - A.k;
        bd[t] = real ? INFINITY : -INFINITY;
        bi[t] = real ? 0xFFFFFFFFu : 0u;
    }
    double cut = A.r2;       // min(r2, k-th best): a candidate beyond it neither qualifies nor enters the list
    int64_t S0 = -1, S1 = min(s_first, s_end);
    for (;;) {
        // the shell: cube S1 clipped to the lattice, without cube S0 (S0 = -1: nothing was examined yet)
        const int32_t X0 = (int32_t)max((int64_t)hx - S1, (int64_t)0), X1 = (int32_t)min((int64_t)hx + S1, (int64_t)nx);
        const int32_t Y0 = (int32_t)max((int64_t)hy - S1, (int64_t)0), Y1 = (int32_t)min((int64_t)hy + S1, (int64_t)ny);
        const int32_t Z0 = (int32_t)max((int64_t)hz - S1, (int64_t)0), Z1 = (int32_t)min((int64_t)hz + S1, (int64_t)nz);
        if (X0 <= X1 && Y0 <= Y1) {
            for (int32_t gz = Z0; gz <= Z1; ++gz) {
                double d = qz - nm_centre(gz, L.min_z, L.edge, L.half_edge);
                const double dz2 = d * d;
                // as nbr_walk's row skip: d2 >= fl(dy2 + dz2) >= dz2 by monotonic rounding
                if (!(dz2 <= cut)) continue;
                const bool inz = (int64_t)gz >= hz - S0 && (int64_t)gz <= hz + S0;
                const int64_t layer = (int64_t)gz << (L.by + NM_SBY_BITS);
                if (WIDE) {
                    const int64_t a = (layer | Y0) << A.piece_bits, b = ((layer | Y1) + 1) << A.piece_bits;
                    if (nn_before(A, m, b) == nn_before(A, m, a)) continue;
                }
                for (int32_t gy = Y0; gy <= Y1; ++gy) {
                    d = qy - nm_centre(gy, L.min_y, L.edge, L.half_edge);
                    const double dy2 = d * d;
                    if (!(dy2 + dz2 <= cut)) continue;
                    const bool inner = inz && (int64_t)gy >= hy - S0 && (int64_t)gy <= hy + S0;
                    const uint32_t wrow = (((uint32_t)gz & 7u) << 3) | ((uint32_t)gy & 7u);
                    const int64_t row = (layer | gy) << A.piece_bits;
                    // a row that crosses the examined cube has a piece on either side of it
                    for (int seg = 0; seg < (inner ? 2 : 1); ++seg) {
                        int32_t xa = X0, xb = X1;
                        if (inner) {
                            if (seg == 0) xb = (int32_t)min((int64_t)X1, (int64_t)hx - S0 - 1);
                            else xa = (int32_t)max((int64_t)X0, (int64_t)hx + S0 + 1);
                        }
                        if (xa > xb) continue;
                        int32_t piece_seen = -1;
                        if (WIDE) {
                            const int32_t pa = xa >> pshift, pb = xb >> pshift;
                            if (nn_before(A, m, row + pb + 1) == nn_before(A, m, row + pa)) continue;
                            if (pa == pb) piece_seen = pa;
                        }
                        for (int32_t sbx = xa >> NM_SBX_BITS; sbx <= (xb >> NM_SBX_BITS); ++sbx) {
                            if (WIDE) {
                                const int32_t pc = sbx >> A.chunk_log2;
                                if (pc != piece_seen) {
                                    piece_seen = pc;
                                    if (nn_before(A, m, row + pc + 1) == nn_before(A, m, row + pc)) {
                                        sbx = ((pc + 1) << A.chunk_log2) - 1;
                                        continue;
                                    }
                                }
                            }
                            const uint64_t at = nm_sb_key((uint32_t)sbx, (uint32_t)gy >> NM_SBY_BITS,
                                                          (uint32_t)gz >> NM_SBZ_BITS, L) * NM_LEAF_WORDS + wrow;
                            const uint32_t all = A.leaf[at];
                            const int32_t base = sbx << NM_SBX_BITS;
                            const int32_t lo = max(xa - base, 0), hi = min(xb - base, 31);
                            uint32_t word = all & (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo);
                            uint32_t r0 = 0;
                            bool have_rank = false;
                            while (word) {
                                const int bit = __ffs((int)word) - 1;
                                word &= word - 1u;
                                d = qx - nm_centre(base + bit, L.min_x, L.edge, L.half_edge);
                                double cd = (d * d + dy2) + dz2;
                                if (!(cd <= cut)) continue;
                                if (!have_rank) {
                                    r0 = A.rank[at];
                                    have_rank = true;
                                }
                                uint32_t ci = r0 + (uint32_t)__popc(all & ((1u << bit) - 1u));
#pragma unroll
                                for (int t = 0; t < K; ++t) {
                                    const bool before = cd < bd[t] || (cd == bd[t] && ci < bi[t]);
                                    const double td = before ? bd[t] : cd;
                                    const uint32_t ti = before ? bi[t] : ci;
                                    bd[t] = before ? cd : bd[t];
                                    bi[t] = before ? ci : bi[t];
                                    cd = td;
                                    ci = ti;
                                }
                                cut = bd[K - 1] < A.r2 ? bd[K - 1] : A.r2;
                            }
                        }
                    }
                }
            }
        }
        const double kth = bd[K - 1];
        if (S1 >= s_end) break;                                   // (b), (c)
        const double reach = ((double)S1 + 0.5 - 1e-6) * L.edge;
        if (kth <= reach * reach) break;                          // (a)
        // the next cube: with k voxels in hand the smallest whose bound (a) covers the k-th (it can only come
        // closer, so that cube is the last); else twice as wide.  only the test above decides what is final
        int64_t next = 2 * S1 > 0 ? 2 * S1 : 1;
        if (kth < INFINITY) {
            next = (int64_t)ceil(sqrt(kth) / L.edge - 0.5 + 1e-6);
            if (next <= S1) next = S1 + 1;
        }
        if (next > s_end) next = s_end;
        if (next > cap) {
            *hint = (uint32_t)next;
            return false;
        }
        S0 = S1;
        S1 = next;
    }
    int32_t n = 0;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const int j = t - (K - A.k);
        if (j >= 0) {
            const bool real = bi[t] != 0xFFFFFFFFu;
            n += real;
            if (A.dist2) A.dist2[q * A.ostride + j] = bd[t];          // (+infinity where no voxel is)
            if (A.index) A.index[q * A.ostride + j] = real ? (int64_t)bi[t] : (int64_t)-1;
        }
    }
    if (A.found) A.found[q] = n;
    return true;
}

// the first cube holds at least k cells: 27 at half-width 1, 125 at 2 (k <= NM_NEAREST_MAX_K = 32)
__device__ __forceinline__ int64_t nn_first_cube(int32_t k) { return k <= 27 ? 1 : 2; }

template <int K>
__global__ __launch_bounds__(256) void k_nn_near(NnArgs A)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool pending = false;
    uint32_t hint = 0;
    if (q < A.nq) pending = !nn_search<K, false>(A, q, nn_first_cube(A.k), NN_NEAR_CAP, &hint);
    // the wave's unfinished queries take consecutive places of the list (their order in it decides nothing)
    const unsigned long long mask = __ballot(pending);
    if (!mask) return;
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(A.pend_count, (uint32_t)__popcll(mask));
    base = __shfl(base, __ffsll((long long)mask) - 1);
    if (pending) A.pend[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = make_uint2((uint32_t)q, hint);
}

// one wave per block: the listed queries are spread over the device; the blocks beyond the list leave at once
template <int K>
__global__ __launch_bounds__(64) void k_nn_wide(NnArgs A)
{
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= (int64_t)*A.pend_count) return;
    const uint2 e = A.pend[at];
    uint32_t hint = 0;
    nn_search<K, true>(A, (int64_t)e.x, (int64_t)e.y, INT64_MAX, &hint);
}

// ---- components: the connected components of the voxel graph ------------------------------------------------------------
// vertices: the M occupied voxels by position; u ~ v iff v is in lists(voxels(), r)[u] (or the other way round:
// for a voxel centre as query the home cell is the voxel's own cell, the window is symmetric about it, and
// ((dx*dx + dy2) + dz2) has the same value from either end, so the relation is symmetric as computed) and both carry
// the same class >= 0.  no list is written: every voxel walks the FORWARD half of its window - the cells of a larger
// address, i.e. the voxels of a larger position - so every edge is seen once, from its smaller end, and is handed to
// a lock-free union-find.
//
// union-find: parent[x] <= x always (only a root is ever hooked, under a smaller node, by compare-and-swap on its
// own word; path halving replaces a parent by the parent's parent, smaller still), so walks strictly descend, end,
// and the root of a finished tree is the smallest position of its component - whatever order the lanes ran in.
// nobody waits: a failed compare-and-swap returns the word another lane wrote, and the loop goes on from THAT node,
// strictly below the one it tried; there is no value a lane polls for.  parent[] is read and written with relaxed
// device-scope atomics while lanes race (link, flatten); a stale read is an older parent, still in the same tree.
//
// tmp (nm_neighbor_index_components_workspace_bytes), room = the voxel count rounded up to whole scan tiles:
//   header  256 B      word 0: components kept (the scan's total)
//   partial 8 KB       the scan's per-block sums
//   addr    room * 8   the address of every voxel (k_nbr_addresses): the lane of voxel v finds its cell there
//   size    room * 8   per ROOT the sum of its component's weights (integer atomics: exact in any order)
//   parent  room * 4   the forest; CC_NONE for a voxel that is not in the graph
//   keep    room * 4   1 for the root of a kept component, then (scanned in place) its number
constexpr uint32_t CC_NONE = 0xFFFFFFFFu;

struct CcPlan {
    int64_t room;
    int32_t scan_blocks, tiles_per_block;
    size_t off_partial, off_addr, off_size, off_parent, off_keep, bytes;
};

CcPlan cc_plan_tiles(int64_t tiles)
{
    CcPlan C;
    C.room = tiles * NBR_SCAN_TILE;
    C.scan_blocks = (int32_t)(tiles < NBR_SCAN_MAX_BLOCKS ? tiles : NBR_SCAN_MAX_BLOCKS);
    C.tiles_per_block = (int32_t)((tiles + C.scan_blocks - 1) / C.scan_blocks);
    C.off_partial = NBR_HEADER_BYTES;
    C.off_addr = C.off_partial + (size_t)NBR_SCAN_MAX_BLOCKS * 4;
    C.off_size = C.off_addr + (size_t)C.room * 8;
    C.off_parent = C.off_size + (size_t)C.room * 8;
    C.off_keep = C.off_parent + (size_t)C.room * 4;
    C.bytes = C.off_keep + (size_t)C.room * 4;
    return C;
}

CcPlan cc_plan(int64_t n) { return cc_plan_tiles(n > 0 ? (n + NBR_SCAN_TILE - 1) / NBR_SCAN_TILE : 1); }

// the plan a scratch of `bytes` has room for (at least cc_plan(0).bytes; M itself is known on the device only)
CcPlan cc_plan_of(size_t bytes)
{
    const size_t fixed = cc_plan(0).bytes - (size_t)NBR_SCAN_TILE * 24;
    int64_t tiles = (int64_t)((bytes - fixed) / ((size_t)NBR_SCAN_TILE * 24));
    const int64_t most = ((int64_t)1 << 31) / NBR_SCAN_TILE;          // positions are 32 bits, M < 2^31
    return cc_plan_tiles(tiles < most ? tiles : most);
}

// M as the kernels take it: nothing at all where the scratch has no room for it (k_cc_label reports that)
__device__ __forceinline__ uint32_t cc_voxels(const uint32_t* __restrict__ index_header, uint32_t room)
{
    const uint32_t m = index_header[0];
    return m <= room ? m : 0u;
}

__device__ __forceinline__ uint32_t cc_load(uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void cc_store(uint32_t* p, uint32_t x)
{
    __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x's tree as of some moment of the walk, halving the path on the way.  x strictly descends
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t x)
{
    uint32_t p = cc_load(parent + x);
    while (p != x) {
        const uint32_t g = cc_load(parent + p);
        if (g == p) return p;
        cc_store(parent + x, g);       // x is no root and never will be again: no compare-and-swap can want this word
        x = g;
        p = cc_load(parent + x);
    }
    return x;
}

// the root of x's tree once nobody links any more, nothing written: in k_cc_flatten only the lane of voxel v stores
// parent[v], and what it stores is final (a halving store of another lane could land behind it and undo it)
__device__ __forceinline__ uint32_t cc_root(uint32_t* parent, uint32_t x)
{
    uint32_t p = cc_load(parent + x);
    while (p != x) {
        x = p;
        p = cc_load(parent + x);
    }
    return x;
}

// joins u's tree to the tree `mine` is in (mine: the root of the lane's own tree when the lane last looked); returns
// a node of the joined tree no larger than either root found.  the walk up from u stops as soon as it meets `mine`:
// u hangs below it, the trees are one, and the root's word - the one word every lane of a large component would
// otherwise load twice per edge - is not touched.  a + b strictly falls with every failed compare-and-swap, so the
// loop ends whatever the other lanes do
__device__ __forceinline__ uint32_t cc_join(uint32_t* parent, uint32_t mine, uint32_t u)
{
    uint32_t b = u;
    uint32_t p = cc_load(parent + b);
    while (p != b) {
        if (p == mine) return mine;
        const uint32_t g = cc_load(parent + p);
        if (g == p) {
            b = p;
            break;
        }
        cc_store(parent + b, g);       // (halving, as cc_find)
        if (g == mine) return mine;
        b = g;
        p = cc_load(parent + b);
    }
    uint32_t a = cc_find(parent, mine);
    while (a != b) {
        const uint32_t hi = max(a, b), lo = min(a, b);
        const uint32_t seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return lo;     // hooked (lo may have stopped being a root meanwhile: still smaller, same tree)
        a = cc_find(parent, seen);     // someone else hooked hi, under seen < hi
        b = lo;
    }
    return a;
}

// nbr_walk's sibling for a voxel (ox, oy, oz) as its own query: the same centre, home cell, clipped window, row
// skip and unfused test, over the cells of a LARGER address only - bits above its own in its row, rows of a larger
// gy in its layer, every row of a larger gz.  hit(voxel) in ascending voxel order, every one > the voxel's own
template <typename F>
__device__ __forceinline__ void nbr_walk_forward(int32_t ox, int32_t oy, int32_t oz,
                                                 const uint32_t* __restrict__ leaf,
                                                 const uint32_t* __restrict__ rank, const LatticeDev& L, double r2,
                                                 int32_t dmin, int32_t W, F&& hit)
{
    const double qx = nm_centre(ox, L.min_x, L.edge, L.half_edge);
    const double qy = nm_centre(oy, L.min_y, L.edge, L.half_edge);
    const double qz = nm_centre(oz, L.min_z, L.edge, L.half_edge);
    const int32_t hx = nm_clamp_cell(nm_cell_f(qx, L.min_x, L.edge));
    const int32_t hy = nm_clamp_cell(nm_cell_f(qy, L.min_y, L.edge));
    const int32_t hz = nm_clamp_cell(nm_cell_f(qz, L.min_z, L.edge));
    const int32_t x0 = max(hx + dmin, 0), x1 = min(hx + dmin + W - 1, (1 << L.wx) - 1);
    const int32_t y0 = max(hy + dmin, 0), y1 = min(hy + dmin + W - 1, (1 << L.wy) - 1);
    const int32_t z0 = max(hz + dmin, 0), z1 = min(hz + dmin + W - 1, (1 << L.wz) - 1);
    if (x0 > x1) return;
    for (int32_t gz = max(z0, oz); gz <= z1; ++gz) {
        double d = qz - nm_centre(gz, L.min_z, L.edge, L.half_edge);
        const double dz2 = d * d;
        for (int32_t gy = gz == oz ? max(y0, oy) : y0; gy <= y1; ++gy) {
            d = qy - nm_centre(gy, L.min_y, L.edge, L.half_edge);
            const double dy2 = d * d;
            if (!(dy2 + dz2 <= r2)) continue;
            const int32_t xs = (gz == oz && gy == oy) ? max(x0, ox + 1) : x0;      // the own row: above the own bit
            if (xs > x1) continue;
            const uint32_t wrow = (((uint32_t)gz & 7u) << 3) | ((uint32_t)gy & 7u);
            for (int32_t sbx = xs >> NM_SBX_BITS; sbx <= (x1 >> NM_SBX_BITS); ++sbx) {
                const uint64_t at = nm_sb_key((uint32_t)sbx, (uint32_t)gy >> NM_SBY_BITS,
                                              (uint32_t)gz >> NM_SBZ_BITS, L) * NM_LEAF_WORDS + wrow;
                const uint32_t all = leaf[at];
                const int32_t base = sbx << NM_SBX_BITS;
                const int32_t lo = max(xs - base, 0), hi = min(x1 - base, 31);
                uint32_t word = all & (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo);
                if (!word) continue;
                const uint32_t r0 = rank[at];
                while (word) {
                    const int bit = __ffs((int)word) - 1;
                    word &= word - 1u;
                    d = qx - nm_centre(base + bit, L.min_x, L.edge, L.half_edge);
                    const double s = (d * d + dy2) + dz2;
                    if (!(s <= r2)) continue;
                    hit(r0 + (uint32_t)__popc(all & ((1u << bit) - 1u)));
                }
            }
        }
    }
}

// init: every voxel of the graph its own tree, the others CC_NONE (the pad of the scratch too); sizes and marks zero
__global__ __launch_bounds__(256) void k_cc_init(const uint32_t* __restrict__ index_header, uint32_t room,
                                                 const int64_t* __restrict__ cls, uint32_t* __restrict__ parent,
                                                 uint32_t* __restrict__ keep, int64_t* __restrict__ size,
                                                 int64_t* __restrict__ d_count)
{
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;       // (room <= 2^31)
    if (v >= room) return;
    parent[v] = (v < m && !(cls && cls[v] < 0)) ? v : CC_NONE;
    keep[v] = 0u;
    size[v] = 0;
    if (v == 0) d_count[1] = 0;
}

// link: one lane per voxel, every forward neighbor of its class joined to it
__global__ __launch_bounds__(256) void k_cc_link(const int64_t* __restrict__ addr,
                                                 const uint32_t* __restrict__ index_header, uint32_t room,
                                                 const uint32_t* __restrict__ leaf,
                                                 const uint32_t* __restrict__ rank, LatticeDev L, double r2,
                                                 int32_t dmin, int32_t W, const int64_t* __restrict__ cls,
                                                 uint32_t* parent)
{
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= m) return;
    const int64_t c = cls ? cls[v] : 0;
    if (c < 0) return;
    const int64_t a = addr[v];
    const int32_t ox = (int32_t)(a & (((int64_t)1 << L.wx) - 1));
    const int32_t oy = (int32_t)((a >> L.s0) & (((int64_t)1 << L.wy) - 1));
    const int32_t oz = (int32_t)(a >> L.s1);
    uint32_t mine = v;       // a node of v's tree, as near its root as this lane has seen
    nbr_walk_forward(ox, oy, oz, leaf, rank, L, r2, dmin, W, [&](uint32_t u) {
        if (cls && cls[u] != c) return;
        mine = cc_join(parent, mine, u);
    });
}

// flatten: parent[v] = the root, and the root's size += the voxel's weight.  a cloud that is one component would send
// M adds to one word: a wave adds once per DISTINCT root among its lanes, and the first of them - in a large
// component the only one - goes through LDS, where the block's waves that share it make one add of it
constexpr int CC_FLAT_THREADS = 1024;
__global__ __launch_bounds__(CC_FLAT_THREADS) void k_cc_flatten(const uint32_t* __restrict__ index_header,
                                                                uint32_t room, const int64_t* __restrict__ weight,
                                                                uint32_t* parent, int64_t* __restrict__ size)
{
    constexpr int WAVES = CC_FLAT_THREADS / 64;
    __shared__ uint32_t first_root[WAVES];
    __shared__ long long first_sum[WAVES];
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t root = CC_NONE;
    long long w = 0;
    if (v < m) {
        const uint32_t p = cc_load(parent + v);
        if (p != CC_NONE) {
            root = cc_root(parent, p);
            if (root != p) cc_store(parent + v, root);
            w = weight ? (long long)weight[v] : 1;
        }
    }
    // (no lane has left: the shuffles below see all 64)
    if (lane == 0) first_root[wave] = CC_NONE;
    unsigned long long pending = __ballot(root != CC_NONE);
    bool first = true;
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const uint32_t r0 = __shfl(root, leader);
        const bool same = root == r0;
        long long s = same ? w : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == leader) {
            if (first) {
                first_root[wave] = r0;
                first_sum[wave] = s;
            } else {
                atomicAdd((unsigned long long*)&size[r0], (unsigned long long)s);
            }
        }
        first = false;
        pending &= ~__ballot(same);
    }
    __syncthreads();
    if (threadIdx.x < WAVES) {
        // thread t speaks for wave t's first root unless an earlier wave has the same one
        const uint32_t r = first_root[threadIdx.x];
        long long s = r != CC_NONE ? first_sum[threadIdx.x] : 0;
        bool speaks = r != CC_NONE;
        for (int j = 0; j < WAVES; ++j) {
            const bool match = j != (int)threadIdx.x && first_root[j] == r;
            if (match && j < (int)threadIdx.x) speaks = false;
            if (match && j > (int)threadIdx.x && r != CC_NONE) s += first_sum[j];
        }
        if (speaks) atomicAdd((unsigned long long*)&size[r], (unsigned long long)s);
    }
}

// number, before the scan: the roots of the components that stay; all roots are counted
__global__ __launch_bounds__(256) void k_cc_mark(const uint32_t* __restrict__ index_header, uint32_t room,
                                                 const uint32_t* __restrict__ parent,
                                                 const int64_t* __restrict__ size, int64_t min_size,
                                                 uint32_t* __restrict__ keep, int64_t* __restrict__ d_count)
{
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const bool is_root = v < m && parent[v] == v;
    if (is_root && size[v] >= min_size) keep[v] = 1u;
    const unsigned long long roots = __ballot(is_root);
    if (roots && (threadIdx.x & 63) == 0)
        atomicAdd((unsigned long long*)(d_count + 1), (unsigned long long)__popcll(roots));
}

// number, behind the scan: id[] = keep[] scanned, so a kept root's entry is its component's number - roots in
// ascending position, which is ascending smallest member
__global__ __launch_bounds__(256) void k_cc_label(const uint32_t* __restrict__ index_header, uint32_t room,
                                                  const uint32_t* __restrict__ parent,
                                                  const int64_t* __restrict__ size, int64_t min_size,
                                                  const uint32_t* __restrict__ id, int64_t* __restrict__ label,
                                                  int64_t* __restrict__ sizes, int64_t* __restrict__ d_count)
{
    const uint32_t m = index_header[0];
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (m > room) {          // the scratch was made for fewer voxels than the index holds: nothing was labelled
        if (v == 0) d_count[0] = d_count[1] = -1;
        return;
    }
    if (v >= m) return;
    const uint32_t r = parent[v];
    int64_t out = -1;
    if (r != CC_NONE) {
        const int64_t s = size[r];
        if (s >= min_size) {
            out = (int64_t)id[r];
            if (r == v) sizes[out] = s;
        }
    }
    label[v] = out;
}

// ---- dbscan: density-based clusters of the same graph -----------------------------------------------------------------
// density[v] = the sum of the weights of v and of its neighbors of v's class (the FULL window: every voxel sees all
// of its edges, nothing is shared between lanes); core[v] = density[v] >= min_weight.  the clusters are the components
// of the graph restricted to core voxels: k_cc_init and k_cc_link as they are, on the EFFECTIVE class array eff[] =
// the class of a core voxel and -1 for every other.  a voxel of the graph that is not core joins the cluster of its
// nearest core neighbor by (d2, position) - border - or stays CC_NONE - noise; flatten, mark, scan and label then do
// what they do for components: a border voxel adds its weight to its root, every root is a core voxel, and roots in
// ascending position are clusters in ascending smallest CORE member.
//
// tmp (nm_neighbor_index_dbscan_workspace_bytes): the components layout for `room` voxels, then
//   eff     room * 8   the effective class of every voxel
struct DbPlan {
    CcPlan C;
    size_t off_eff, bytes;
};

DbPlan db_plan_tiles(int64_t tiles)
{
    DbPlan D;
    D.C = cc_plan_tiles(tiles);
    D.off_eff = D.C.bytes;
    D.bytes = D.off_eff + (size_t)D.C.room * 8;
    return D;
}

DbPlan db_plan(int64_t n) { return db_plan_tiles(n > 0 ? (n + NBR_SCAN_TILE - 1) / NBR_SCAN_TILE : 1); }

// the plan a scratch of `bytes` has room for (at least db_plan(0).bytes), as cc_plan_of
DbPlan db_plan_of(size_t bytes)
{
    const size_t fixed = db_plan(0).bytes - (size_t)NBR_SCAN_TILE * 32;
    int64_t tiles = (int64_t)((bytes - fixed) / ((size_t)NBR_SCAN_TILE * 32));
    const int64_t most = ((int64_t)1 << 31) / NBR_SCAN_TILE;
    return db_plan_tiles(tiles < most ? tiles : most);
}

// the cell of voxel v from its address (as k_cc_link)
__device__ __forceinline__ void db_cell(int64_t a, const LatticeDev& L, int32_t* ox, int32_t* oy, int32_t* oz)
{
    *ox = (int32_t)(a & (((int64_t)1 << L.wx) - 1));
    *oy = (int32_t)((a >> L.s0) & (((int64_t)1 << L.wy) - 1));
    *oz = (int32_t)(a >> L.s1);
}

// density: one lane per voxel, the lists' walk from the voxel's own centre (which finds the voxel itself, at d2 = 0),
// an int64 sum in registers.  no atomics: every word written here is the lane's own
__global__ __launch_bounds__(256) void k_db_density(const int64_t* __restrict__ addr,
                                                    const uint32_t* __restrict__ index_header, uint32_t room,
                                                    const uint32_t* __restrict__ leaf,
                                                    const uint32_t* __restrict__ rank, LatticeDev L, double r2,
                                                    int32_t dmin, int32_t W, const int64_t* __restrict__ cls,
                                                    const int64_t* __restrict__ weight, int64_t min_weight,
                                                    int64_t* __restrict__ density, uint8_t* __restrict__ core,
                                                    int64_t* __restrict__ eff, int64_t* __restrict__ d_count)
{
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0) d_count[2] = 0;          // (the core voxels are counted by k_db_border)
    if (v >= m) return;
    const int64_t c = cls ? cls[v] : 0;
    int64_t sum = 0;
    if (c >= 0) {
        int32_t ox, oy, oz;
        db_cell(addr[v], L, &ox, &oy, &oz);
        nbr_walk(nm_centre(ox, L.min_x, L.edge, L.half_edge), nm_centre(oy, L.min_y, L.edge, L.half_edge),
                 nm_centre(oz, L.min_z, L.edge, L.half_edge), leaf, rank, L, r2, dmin, W, [&](uint32_t u) {
                     if (cls && cls[u] != c) return;
                     sum += weight ? weight[u] : 1;
                 });
    }
    const bool is_core = c >= 0 && sum >= min_weight;
    if (density) density[v] = sum;
    core[v] = is_core ? 1 : 0;
    eff[v] = is_core ? c : -1;
}

// border: runs when k_cc_link has finished.  a voxel of the graph that is not core walks its window again and keeps
// the smallest (d2, position) among the core voxels of its class; the walk is in ascending position, so "strictly
// smaller replaces" breaks equal distances towards the smaller position.  it then hangs itself under the ROOT of that
// voxel's tree.  race-free without an atomic read-modify-write: only the lane of voxel v stores parent[v], and only
// where v is not core; the words cc_root reads are those of core voxels (a tree of the link kernel holds core voxels
// only, and no lane here walks up from a border voxel), which nobody writes in this kernel.  so every read sees the
// finished forest and the result is a function of the arguments.  also counts the core voxels, once per wave
__global__ __launch_bounds__(256) void k_db_border(const int64_t* __restrict__ addr,
                                                   const uint32_t* __restrict__ index_header, uint32_t room,
                                                   const uint32_t* __restrict__ leaf,
                                                   const uint32_t* __restrict__ rank, LatticeDev L, double r2,
                                                   int32_t dmin, int32_t W, const int64_t* __restrict__ cls,
                                                   const int64_t* __restrict__ eff, uint32_t* parent,
                                                   int64_t* __restrict__ d_count)
{
    const uint32_t m = index_header[0];
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (m > room) {          // (as k_cc_label: the scratch was made for fewer voxels than the index holds)
        if (v == 0) d_count[2] = -1;
        return;
    }
    bool is_core = false;
    if (v < m) {
        is_core = eff[v] >= 0;
        const int64_t c = cls ? cls[v] : 0;
        if (!is_core && c >= 0) {
            int32_t ox, oy, oz;
            db_cell(addr[v], L, &ox, &oy, &oz);
            double best_d2 = INFINITY;
            uint32_t best = CC_NONE;
            nbr_walk_d2(nm_centre(ox, L.min_x, L.edge, L.half_edge), nm_centre(oy, L.min_y, L.edge, L.half_edge),
                        nm_centre(oz, L.min_z, L.edge, L.half_edge), leaf, rank, L, r2, dmin, W,
                        [&](uint32_t u, double d2) {
                            if (eff[u] != c) return;         // core, and of this voxel's class
                            if (d2 < best_d2) {
                                best_d2 = d2;
                                best = u;
                            }
                        });
            if (best != CC_NONE) cc_store(parent + v, cc_root(parent, best));
        }
    }
    // (no lane has left)
    const unsigned long long cores = __ballot(is_core);
    if (cores && (threadIdx.x & 63) == 0)
        atomicAdd((unsigned long long*)(d_count + 2), (unsigned long long)__popcll(cores));
}

// ---- regions: smoothness-constrained region growing on the same graph ---------------------------------------------------
// dbscan's shape with the caller's seeds in the place of the core voxels and a predicate on every seed-seed edge: the
// regions are the components of the seeds under the edges whose two normals and value rows agree.  eff[] = the class
// of a seed of the graph and -1 for every other voxel (k_rg_seed); k_cc_init on eff[]; k_rg_link, k_cc_link's sibling
// with the predicate between the class test and the join; k_db_border as it is - a voxel of the graph that is no seed
// joins the region of its nearest seed neighbor by (d2, position), the predicate is not asked there - and flatten,
// mark, scan and label as for components.  tmp: dbscan's layout (DbPlan).
//
// both tests are symmetric in (u, v) bit for bit - the three products commute and the sum keeps its order,
// fl(a - b) = -fl(b - a) and fabs drops the sign - so the forward walk, which sees an edge from its smaller end
// only, decides exactly what the larger end would have decided
struct RgStep {
    double s[NM_REGION_MAX_DIMS];
};

__global__ __launch_bounds__(256) void k_rg_seed(const uint32_t* __restrict__ index_header, uint32_t room,
                                                 const int64_t* __restrict__ cls, const uint8_t* __restrict__ seed,
                                                 int64_t* __restrict__ eff, int64_t* __restrict__ d_count)
{
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0) d_count[2] = 0;          // (the seeds are counted by k_db_border)
    if (v >= m) return;
    const int64_t c = cls ? cls[v] : 0;
    eff[v] = (c >= 0 && (!seed || seed[v])) ? c : -1;
}

// link: one lane per seed, its own normal and value row in registers for the whole walk.  per hit, cheapest first:
// the 8 bytes of eff[u] (seed and same class in one load), the DIMS value columns, the 24 bytes of the normal; a hit
// that fails touches no word of parent[].  the comparisons are written so that NaN is false
template <bool NORMAL, int DIMS>
__global__ __launch_bounds__(256) void k_rg_link(const int64_t* __restrict__ addr,
                                                 const uint32_t* __restrict__ index_header, uint32_t room,
                                                 const uint32_t* __restrict__ leaf,
                                                 const uint32_t* __restrict__ rank, LatticeDev L, double r2,
                                                 int32_t dmin, int32_t W, const int64_t* __restrict__ eff,
                                                 const double* __restrict__ normal, int64_t normal_stride,
                                                 double min_cos, const double* __restrict__ value,
                                                 int64_t value_stride, RgStep step, uint32_t* parent)
{
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= m) return;
    const int64_t c = eff[v];
    if (c < 0) return;
    const int64_t a = addr[v];
    const int32_t ox = (int32_t)(a & (((int64_t)1 << L.wx) - 1));
    const int32_t oy = (int32_t)((a >> L.s0) & (((int64_t)1 << L.wy) - 1));
    const int32_t oz = (int32_t)(a >> L.s1);
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if constexpr (NORMAL) {
        const double* n = normal + (int64_t)v * normal_stride;
        nx = n[0];
        ny = n[1];
        nz = n[2];
    }
    double own[DIMS > 0 ? DIMS : 1];
    if constexpr (DIMS > 0) {
        const double* x = value + (int64_t)v * value_stride;
#pragma unroll
        for (int k = 0; k < DIMS; ++k) own[k] = x[k];
    }
    uint32_t mine = v;       // (as k_cc_link)
    nbr_walk_forward(ox, oy, oz, leaf, rank, L, r2, dmin, W, [&](uint32_t u) {
        if (eff[u] != c) return;
        if constexpr (DIMS > 0) {
            const double* x = value + (int64_t)u * value_stride;
            bool near = true;
#pragma unroll
            for (int k = 0; k < DIMS; ++k) near = near && fabs(own[k] - x[k]) <= step.s[k];
            if (!near) return;
        }
        if constexpr (NORMAL) {
            const double* n = normal + (int64_t)u * normal_stride;
            if (!(fabs((nx * n[0] + ny * n[1]) + nz * n[2]) >= min_cos)) return;
        }
        mine = cc_join(parent, mine, u);
    });
}

// ---- hill climbing: peak-seeking segments of the same graph ------------------------------------------------------------
// every voxel of the graph takes ONE uphill link - a neighbor of its class that is higher than itself - or none, a
// peak; a segment is everything that climbs to the same peak.  no union-find: the links ARE the forest.  k_hc_parent
// writes parent[] whole (k_cc_init is not run), and flatten, mark, scan and label then do what they do for
// components: none of them needs parent[v] <= v (only cc_join orders by position, and it is not used here), a peak is
// a root, and roots in ascending position are segments in ascending peak position.  tmp: the components layout.
//
// "higher" is a strict total order on the voxels of the graph: by value, equal values (-0 == +0) by the SMALLER
// position.  every comparison is false for NaN; a voxel with a NaN value is out of the graph, so no NaN gets here
// as v, and one that gets here as u is no candidate
__device__ __forceinline__ bool hc_higher(double value_u, uint32_t u, double value_v, uint32_t v)
{
    return value_u > value_v || (value_u == value_v && u < v);
}

// parent: one lane per voxel, the lists' walk from the voxel's own centre as k_db_border runs it, the lane's own value
// and class plus three registers for the best candidate.  a hit u is a candidate iff it has v's class, a value that
// is no NaN and hc_higher(u, v).  NO CYCLE CAN FORM: a link goes from v to a voxel strictly above it in a strict total
// order (hc_higher(v, v) is false, so the walk's own hit at d2 = 0 needs no special case), and a chain of links
// strictly ascends in it.  cc_root in k_cc_flatten follows these links with no other exit than a root: a cycle would
// be an endless loop there, so this predicate is the one place where nothing may be loosened.
// among the candidates: !NEAREST (steepest ascent) keeps the largest value, among equal values the smaller d2, among
// equal d2 the smaller position; NEAREST (quick shift) keeps the smallest d2, among equal d2 the larger value, then
// the smaller position.  the walk is in ascending position, so "strictly better replaces" is that last tiebreak.
// every word written is the lane's own: parent[v] = the link, v itself at a peak, CC_NONE outside the graph and in
// the pad of the scratch; keep[], size[] and d_count[1] are zeroed as k_cc_init zeroes them
template <bool NEAREST>
__global__ __launch_bounds__(256) void k_hc_parent(const int64_t* __restrict__ addr,
                                                   const uint32_t* __restrict__ index_header, uint32_t room,
                                                   const uint32_t* __restrict__ leaf,
                                                   const uint32_t* __restrict__ rank, LatticeDev L, double r2,
                                                   int32_t dmin, int32_t W, const int64_t* __restrict__ cls,
                                                   const double* __restrict__ value, uint32_t* __restrict__ parent,
                                                   uint32_t* __restrict__ keep, int64_t* __restrict__ size,
                                                   int64_t* __restrict__ link, int64_t* __restrict__ d_count)
{
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;       // (room <= 2^31)
    if (v >= room) return;
    keep[v] = 0u;
    size[v] = 0;
    if (v == 0) d_count[1] = 0;
    uint32_t up = CC_NONE;
    if (v < m) {
        const int64_t c = cls ? cls[v] : 0;
        const double own = value[v];
        if (c >= 0 && own == own) {
            int32_t ox, oy, oz;
            db_cell(addr[v], L, &ox, &oy, &oz);
            uint32_t best = CC_NONE;
            double best_value = 0.0, best_d2 = 0.0;
            nbr_walk_d2(nm_centre(ox, L.min_x, L.edge, L.half_edge), nm_centre(oy, L.min_y, L.edge, L.half_edge),
                        nm_centre(oz, L.min_z, L.edge, L.half_edge), leaf, rank, L, r2, dmin, W,
                        [&](uint32_t u, double d2) {
                            const double x = value[u];
                            if (!hc_higher(x, u, own, v)) return;        // (NaN too)
                            if (cls && cls[u] != c) return;
                            const bool better =
                                best == CC_NONE ||
                                (NEAREST ? (d2 < best_d2 || (d2 == best_d2 && x > best_value))
                                         : (x > best_value || (x == best_value && d2 < best_d2)));
                            if (better) {
                                best = u;
                                best_value = x;
                                best_d2 = d2;
                            }
                        });
            up = best != CC_NONE ? best : v;
        }
        if (link) link[v] = up != CC_NONE ? (int64_t)up : -1;
    }
    parent[v] = up;
}

// peaks, behind the scan: the kept root r writes its position at its segment's number.  roots are numbered in
// ascending position, so peak[] comes out ascending.  nothing is written where the scratch has no room for the index
__global__ __launch_bounds__(256) void k_hc_peaks(const uint32_t* __restrict__ index_header, uint32_t room,
                                                  const uint32_t* __restrict__ parent,
                                                  const int64_t* __restrict__ size, int64_t min_size,
                                                  const uint32_t* __restrict__ id, int64_t* __restrict__ peak)
{
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= m) return;
    if (parent[v] == v && size[v] >= min_size) peak[id[v]] = (int64_t)v;
}

// ---- adjacency: which segments of a labelling touch, over how many edges, and how high the pass between them lies -----
// the region adjacency graph of a labelling of the voxels, taken off the index: no list of the voxel graph is written.
// one lane per voxel walks the FORWARD half of its window (nbr_walk_forward), so every undirected edge {v, u} is met
// exactly once, from its smaller end, in ascending u - nothing has to be kept from counting twice.  an edge CROSSES
// when both ends carry a label >= 0, the labels differ, the classes agree (and are >= 0) and neither value is NaN.
// how many crossing edges there are is not known before the walk: the walk runs twice, once to count the records of
// every voxel (scanned in place, k_nbr_scan_*), once to write them at the voxel's offset; the host reads the total
// between the two and brings the room.
//
// a RECORD is (key, links, saddle): key = (a << 32) | b with a < b the two labels, links a number of edges, saddle the
// largest min(value[v], value[u]) over them.  consecutive hits of one lane with the SAME label on the other side are one
// record (hits come in ascending position, and neighbors in a row mostly share a segment): the lane keeps one open
// record in registers and closes it when the label changes.  both passes run the same walk, so they agree on the
// number of records.  records are then ordered by key (by the caller: any sort of 64-bit keys) and reduced, one row per
// run of equal keys: links add up, saddles take the maximum - integer adds and a maximum, the same in any order.
//
// tmp of the walk (nm_neighbor_index_adjacency_workspace_bytes), room = the voxel count rounded up to whole scan tiles:
//   header  256 B      word 0: records (the scan's total)
//   partial 8 KB       the scan's per-block sums
//   addr    room * 8   the address of every voxel (k_nbr_addresses)
//   count   room * 4   records of every voxel, then (scanned in place) where its first one goes
// tmp of the reduction, rpad = the record count rounded up to whole scan tiles:
//   header  256 B      word 0: rows (the scan's total)
//   partial 8 KB
//   row     rpad * 4   1 at the first record of every run of equal keys, then (scanned in place) rows before it
struct AdjPlan {
    int64_t room;
    int32_t scan_blocks, tiles_per_block;
    size_t off_partial, off_addr, off_count, bytes;
};

AdjPlan adj_plan_tiles(int64_t tiles)
{
    AdjPlan A;
    A.room = tiles * NBR_SCAN_TILE;
    A.scan_blocks = (int32_t)(tiles < NBR_SCAN_MAX_BLOCKS ? tiles : NBR_SCAN_MAX_BLOCKS);
    A.tiles_per_block = (int32_t)((tiles + A.scan_blocks - 1) / A.scan_blocks);
    A.off_partial = NBR_HEADER_BYTES;
    A.off_addr = A.off_partial + (size_t)NBR_SCAN_MAX_BLOCKS * 4;
    A.off_count = A.off_addr + (size_t)A.room * 8;
    A.bytes = A.off_count + (size_t)A.room * 4;
    return A;
}

AdjPlan adj_plan(int64_t n) { return adj_plan_tiles(n > 0 ? (n + NBR_SCAN_TILE - 1) / NBR_SCAN_TILE : 1); }

// the plan a scratch of `bytes` has room for (at least adj_plan(0).bytes), as cc_plan_of
AdjPlan adj_plan_of(size_t bytes)
{
    const size_t fixed = adj_plan(0).bytes - (size_t)NBR_SCAN_TILE * 12;
    int64_t tiles = (int64_t)((bytes - fixed) / ((size_t)NBR_SCAN_TILE * 12));
    const int64_t most = ((int64_t)1 << 31) / NBR_SCAN_TILE;
    return adj_plan_tiles(tiles < most ? tiles : most);
}

struct AdjRows {
    int64_t rpad;
    int32_t scan_blocks, tiles_per_block;
    size_t off_partial, off_row, bytes;
};

AdjRows adj_rows(int64_t n)
{
    const int64_t tiles = n > 0 ? (n + NBR_SCAN_TILE - 1) / NBR_SCAN_TILE : 1;
    AdjRows R;
    R.rpad = tiles * NBR_SCAN_TILE;
    R.scan_blocks = (int32_t)(tiles < NBR_SCAN_MAX_BLOCKS ? tiles : NBR_SCAN_MAX_BLOCKS);
    R.tiles_per_block = (int32_t)((tiles + R.scan_blocks - 1) / R.scan_blocks);
    R.off_partial = NBR_HEADER_BYTES;
    R.off_row = R.off_partial + (size_t)NBR_SCAN_MAX_BLOCKS * 4;
    R.bytes = R.off_row + (size_t)R.rpad * 4;
    return R;
}

constexpr int64_t ADJ_LABEL_LIMIT = (int64_t)1 << 31;       // labels are packed two to a 64-bit key

// the order-preserving integer image of an fp64 that is no NaN: x < y iff image(x) < image(y), -0 just below +0.
// no such number has the image 0 (that would be a NaN with every bit set), so 0 is "nothing yet" under a maximum
__device__ __forceinline__ unsigned long long adj_image(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double adj_number(unsigned long long image)
{
    const unsigned long long b = (image >> 63) ? (image & 0x7FFFFFFFFFFFFFFFull) : ~image;
    return __longlong_as_double((long long)b);
}

// the walk, both passes.  !EMIT: count[v] = the records of voxel v (0 outside the graph and in the pad of the scratch),
// d_count[1] += the labels that are no valid label (>= 2^31; the host has zeroed it), -1 there where the scratch has no
// room for the index.  EMIT: count[] holds the scanned offsets and header[0] the total; the lane writes its records
// from its offset on, every word its own - or nothing at all, and d_count[0] = -1, where the total exceeds `capacity`
template <bool EMIT>
__global__ __launch_bounds__(256) void k_adj_walk(const int64_t* __restrict__ addr,
                                                  const uint32_t* __restrict__ index_header, uint32_t room,
                                                  const uint32_t* __restrict__ leaf,
                                                  const uint32_t* __restrict__ rank, LatticeDev L, double r2,
                                                  int32_t dmin, int32_t W, const int64_t* __restrict__ label,
                                                  const int64_t* __restrict__ cls,
                                                  const double* __restrict__ value, uint32_t* __restrict__ count,
                                                  const uint32_t* __restrict__ header, int64_t capacity,
                                                  int64_t* __restrict__ key, int64_t* __restrict__ links,
                                                  double* __restrict__ saddle, int64_t* __restrict__ d_count)
{
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;       // (room <= 2^31)
    if (v >= room) return;
    if (EMIT) {
        if ((int64_t)header[0] > capacity) {
            if (v == 0) d_count[0] = -1;
            return;
        }
    } else if (v == 0 && index_header[0] > room) {
        d_count[1] = -1;          // (m is 0 then: nobody adds to this word)
    }
    uint32_t n = 0;
    bool bad = false;
    if (v < m) {
        const int64_t la = label[v];
        const int64_t c = cls ? cls[v] : 0;
        const double own = value ? value[v] : 0.0;
        bad = la >= ADJ_LABEL_LIMIT;
        if (la >= 0 && !bad && c >= 0 && own == own) {
            int32_t ox, oy, oz;
            db_cell(addr[v], L, &ox, &oy, &oz);
            const int64_t at = EMIT ? (int64_t)count[v] : 0;
            int64_t open = -1;          // the label on the other side of the open record; none yet
            int64_t open_links = 0;
            double open_saddle = 0.0;
            auto close = [&]() {
                if (open < 0) return;
                if (EMIT) {
                    const int64_t lo = la < open ? la : open, hi = la < open ? open : la;
                    if (at + n < capacity) {        // (always, for the labels, classes and values the count saw)
                        key[at + n] = (lo << 32) | hi;
                        links[at + n] = open_links;
                        if (saddle) saddle[at + n] = open_saddle;
                    }
                }
                ++n;
            };
            nbr_walk_forward(ox, oy, oz, leaf, rank, L, r2, dmin, W, [&](uint32_t u) {
                const int64_t lb = label[u];
                if (lb < 0 || lb == la || lb >= ADJ_LABEL_LIMIT) return;
                if (cls && cls[u] != c) return;
                const double x = value ? value[u] : 0.0;
                if (x != x) return;
                const double pass = x < own ? x : own;
                if (lb == open) {
                    ++open_links;
                    if (pass > open_saddle) open_saddle = pass;
                } else {
                    close();
                    open = lb;
                    open_links = 1;
                    open_saddle = pass;
                }
            });
            close();
        }
    }
    if (!EMIT) {
        count[v] = n;
        const unsigned long long bads = __ballot(bad);
        if (bads && (threadIdx.x & 63) == 0)
            atomicAdd((unsigned long long*)(d_count + 1), (unsigned long long)__popcll(bads));
    }
}

// reduction, before the scan: 1 at the first record of every run of equal keys (the keys are sorted), 0 in the pad;
// the rows' sums and maxima start from nothing
__global__ __launch_bounds__(256) void k_adj_heads(const int64_t* __restrict__ key, int64_t n, int64_t rpad,
                                                   uint32_t* __restrict__ row, int64_t* __restrict__ links,
                                                   unsigned long long* __restrict__ image)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rpad) return;
    row[i] = (i < n && (i == 0 || key[i] != key[i - 1])) ? 1u : 0u;
    if (i < n) {
        links[i] = 0;
        if (image) image[i] = 0ull;
    }
}

// reduction, behind the scan: record i belongs to row  row[i] + head(i) - 1.  the lanes of a wave hold consecutive
// records, so the records of one row are consecutive lanes: a segmented scan over the wave adds them up, and the last
// lane of every row in the wave hands the wave's part to the row - one atomic add and one atomic maximum per row and
// wave, on integers: the same result whatever the order.  the first record of a row writes its pair
__global__ __launch_bounds__(256) void k_adj_reduce(const int64_t* __restrict__ key,
                                                    const int64_t* __restrict__ order,
                                                    const int64_t* __restrict__ links_in,
                                                    const double* __restrict__ saddle_in, int64_t n,
                                                    const uint32_t* __restrict__ row, int64_t* __restrict__ pair,
                                                    int64_t* __restrict__ links,
                                                    unsigned long long* __restrict__ image)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t r = CC_NONE;
    unsigned long long sum = 0ull, top = 0ull;
    if (i < n) {
        const int64_t k = key[i];
        const bool head = i == 0 || k != key[i - 1];
        r = row[i] + (head ? 1u : 0u) - 1u;
        const int64_t from = order ? order[i] : i;
        sum = (unsigned long long)links_in[from];
        if (saddle_in) top = adj_image(saddle_in[from]);
        if (head) {
            pair[2 * (int64_t)r] = k >> 32;
            pair[2 * (int64_t)r + 1] = k & 0xFFFFFFFFll;
        }
    }
    // (no lane has left: the shuffles below see all 64)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t r_below = __shfl_up(r, off);
        const unsigned long long sum_below = __shfl_up(sum, off);
        const unsigned long long top_below = __shfl_up(top, off);
        if (lane >= off && r_below == r) {
            sum += sum_below;
            top = top_below > top ? top_below : top;
        }
    }
    const uint32_t r_above = __shfl_down(r, 1);
    if (r != CC_NONE && (lane == 63 || r_above != r)) {
        atomicAdd((unsigned long long*)&links[r], sum);
        if (image) atomicMax(&image[r], top);
    }
}

// the maxima back from their integer image to numbers, in place
__global__ __launch_bounds__(256) void k_adj_saddles(const uint32_t* __restrict__ header,
                                                     unsigned long long* __restrict__ image)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)header[0]) return;
    const double x = adj_number(image[e]);
    ((double*)image)[e] = x;
}

// ---- geodesic: shortest paths from seeds over the same graph ------------------------------------------------------------
// dist[v] = the least fixpoint of  dist[v] = min over neighbors u of v's class of fl(dist[u] + w(u, v)),  seeds at 0 and
// the rest from +inf; w = sqrt(d2), d2 as the walk hands it over (bit-symmetric in u and v: the differences are each
// other's negatives) and the square root correctly rounded.  rounded addition is monotone, so relaxing in ANY order
// ends at that one fixpoint: the smallest left-to-right rounded path sum.  the one entry point on the handle that
// iterates: a SWEEP is one full-window walk per voxel, in place; the host enqueues sweeps in batches and reads one
// count per batch.
//
// a sweep's lane reads its neighbors' distances with relaxed agent-scope loads and stores its own word only.  a value
// another lane lowers meanwhile may be seen old or new: both are upper bounds of the fixpoint that some path attains,
// and dist[] only ever falls.  a sweep in which no lane lowered read nothing but the values it started from, which is
// the fixpoint equation holding everywhere: count 0 = done.
//
// tmp: the components layout.  addr[] is written by the relax call that initialises and read by the later ones; the
// header's words 16..21 are three 64-bit sweep counters used in turn: sweep j of a call adds into j % 3 (the LAST one
// into d_count[0] instead), reads (j - 1) % 3 and zeroes (j + 1) % 3.  once a sweep has lowered nothing, the sweeps
// queued behind it return at once: a batch that overshoots the fixpoint costs launches, not walks
constexpr size_t GEO_COUNTER_BYTES = 64;      // where the three counters start in the header

__device__ __forceinline__ double geo_load(double* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// lower: the strict total order the links descend in - by distance, equal distances (-0 == +0) by the smaller position.
// false for NaN
__device__ __forceinline__ bool geo_lower(double dist_u, uint32_t u, double dist_v, uint32_t v)
{
    return dist_u < dist_v || (dist_u == dist_v && u < v);
}

// init: 0 at the seeds of the graph, +inf everywhere else.  nothing where the scratch has no room for the index
__global__ __launch_bounds__(256) void k_geo_init(const uint32_t* __restrict__ index_header, uint32_t room,
                                                  const uint8_t* __restrict__ seed, const int64_t* __restrict__ cls,
                                                  double* __restrict__ dist)
{
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= m) return;
    dist[v] = (seed[v] != 0 && !(cls && cls[v] < 0)) ? 0.0 : INFINITY;
}

// sweep: one lane per voxel, the lists' walk from the voxel's own centre as k_hc_parent runs it.  a neighbor can lower
// the lane's best only if its own distance is below it (w > 0 and rounding is monotone: fl(du + w) >= du), so the
// class, the square root and the sum are formed for those alone - in a sweep that changes little, for hardly any.
// a candidate above max_distance is not taken (+inf: no limit; NaN never gets here).  the walk's own hit at d2 = 0
// fails the first test.  prev: the count of the sweep before (NULL: there is none in this call); mine: where this
// sweep counts its lowered lanes, once per wave; next: the counter the sweep behind this one will use
__global__ __launch_bounds__(256) void k_geo_sweep(const int64_t* __restrict__ addr,
                                                   const uint32_t* __restrict__ index_header, uint32_t room,
                                                   const uint32_t* __restrict__ leaf,
                                                   const uint32_t* __restrict__ rank, LatticeDev L, double r2,
                                                   int32_t dmin, int32_t W, const int64_t* __restrict__ cls,
                                                   double max_distance, double* dist,
                                                   const unsigned long long* prev, unsigned long long* mine,
                                                   unsigned long long* next)
{
    const uint32_t m = index_header[0];
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;       // (room <= 2^31)
    if (v == 0) {
        *next = 0ull;
        if (m > room) *mine = ~0ull;       // the scratch was made for fewer voxels than the index holds: -1
    }
    if (m > room) return;
    if (prev && *prev == 0ull) return;     // the fixpoint was reached before this sweep (the same for every lane)
    bool lowered = false;
    if (v < m) {
        const int64_t c = cls ? cls[v] : 0;
        const double own = dist[v];        // the lane's own word: nobody else writes it
        if (c >= 0 && own > 0.0) {         // (a seed cannot fall: no candidate is below 0)
            int32_t ox, oy, oz;
            db_cell(addr[v], L, &ox, &oy, &oz);
            double best = own;
            nbr_walk_d2(nm_centre(ox, L.min_x, L.edge, L.half_edge), nm_centre(oy, L.min_y, L.edge, L.half_edge),
                        nm_centre(oz, L.min_z, L.edge, L.half_edge), leaf, rank, L, r2, dmin, W,
                        [&](uint32_t u, double d2) {
                            const double du = geo_load(dist + u);
                            if (!(du < best)) return;
                            if (cls && cls[u] != c) return;
                            const double through = du + sqrt(d2);
                            if (through <= max_distance && through < best) best = through;
                        });
            if (best < own) {
                __hip_atomic_store(dist + v, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                lowered = true;
            }
        }
    }
    const unsigned long long wave = __ballot(lowered);
    if (wave && (threadIdx.x & 63) == 0) atomicAdd(mine, (unsigned long long)__popcll(wave));
}

// link: the same walk with the predicate of the contract.  a neighbor u of v's class is a candidate iff
// fl(dist[u] + w) == dist[v] AND geo_lower(u, v); the link is the candidate of the smallest distance, among equal ones
// the smallest position (the walk is in ascending position: "strictly smaller replaces").  NO CYCLE CAN FORM, whatever
// dist[] holds: geo_lower is part of the test and not inferred from the fixpoint, a link goes to a voxel strictly
// below v in a strict total order, and a chain of links strictly descends in it.  cc_root in k_cc_flatten follows the
// links with no other exit than a root, so this is the one place where nothing may be loosened.
// parent[v]: the link; v itself at a seed (dist == 0, in the graph); CC_NONE for unreached voxels (dist not below
// +inf: NaN too), voxels out of the graph and the pad.  a reached voxel that is no seed and has no candidate - an
// ORPHAN, which only a dist[] short of the fixpoint has - is counted in d_count[2], gets link -1 and is its OWN root
// here: chains of links may end in it, and cc_root must find a root there and not CC_NONE, which it would take for a
// position.  k_geo_orphans takes the orphans' trees out again behind the flatten.
// keep[] and size[] are zeroed as k_hc_parent zeroes them; d_count is zeroed by the host
__global__ __launch_bounds__(256) void k_geo_link(const int64_t* __restrict__ addr,
                                                  const uint32_t* __restrict__ index_header, uint32_t room,
                                                  const uint32_t* __restrict__ leaf,
                                                  const uint32_t* __restrict__ rank, LatticeDev L, double r2,
                                                  int32_t dmin, int32_t W, const int64_t* __restrict__ cls,
                                                  const double* __restrict__ dist, uint32_t* __restrict__ parent,
                                                  uint32_t* __restrict__ keep, int64_t* __restrict__ size,
                                                  int64_t* __restrict__ link, int64_t* __restrict__ d_count)
{
    const uint32_t m = cc_voxels(index_header, room);
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;       // (the grid is room / 256 blocks: v < room)
    keep[v] = 0u;
    size[v] = 0;
    uint32_t up = CC_NONE;
    bool orphan = false;
    if (v < m) {
        const int64_t c = cls ? cls[v] : 0;
        const double own = dist[v];
        if (c >= 0 && own < INFINITY) {
            if (own == 0.0) {
                up = v;
            } else {
                int32_t ox, oy, oz;
                db_cell(addr[v], L, &ox, &oy, &oz);
                uint32_t best = CC_NONE;
                double best_dist = 0.0;
                nbr_walk_d2(nm_centre(ox, L.min_x, L.edge, L.half_edge), nm_centre(oy, L.min_y, L.edge, L.half_edge),
                            nm_centre(oz, L.min_z, L.edge, L.half_edge), leaf, rank, L, r2, dmin, W,
                            [&](uint32_t u, double d2) {
                                const double du = dist[u];
                                if (!geo_lower(du, u, own, v)) return;       // (NaN too, and v itself)
                                if (cls && cls[u] != c) return;
                                if (!(du + sqrt(d2) == own)) return;
                                if (best == CC_NONE || du < best_dist) {
                                    best = u;
                                    best_dist = du;
                                }
                            });
                orphan = best == CC_NONE;
                up = orphan ? v : best;
            }
        }
        if (link) link[v] = (up != CC_NONE && !orphan) ? (int64_t)up : -1;
    }
    parent[v] = up;
    const unsigned long long wave = __ballot(orphan);
    if (wave && (threadIdx.x & 63) == 0)
        atomicAdd((unsigned long long*)(d_count + 2), (unsigned long long)__popcll(wave));
}

// behind the flatten every parent[v] is a root: a seed (dist == 0) or an orphan.  whatever hangs below an orphan is in
// no segment: CC_NONE, the orphan itself too, so that mark, scan, label and k_hc_peaks see the seeds' trees only.
// every lane reads and writes its own word of parent[].  d_count[2] = -1 where the scratch has no room for the index
// (k_cc_label does the same for the other two)
__global__ __launch_bounds__(256) void k_geo_orphans(const uint32_t* __restrict__ index_header, uint32_t room,
                                                     const double* __restrict__ dist, uint32_t* __restrict__ parent,
                                                     int64_t* __restrict__ d_count)
{
    const uint32_t m = index_header[0];
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (m > room) {
        if (v == 0) d_count[2] = -1;
        return;
    }
    if (v >= m) return;
    const uint32_t r = parent[v];
    if (r != CC_NONE && !(dist[r] == 0.0)) parent[v] = CC_NONE;
}

// argument checks shared by the entry points that take a built workspace
int nbr_check_index(nm_ctx* ctx, const char* who, const nm_lattice* lat, const void* d_work, size_t work_bytes,
                    LatticeDev* L, NbrPlan* P)
{
    int rc = validate_lattice(ctx, lat);
    if (rc) return rc;
    *L = make_lattice_dev(lat);
    if (!nbr_in_range(*L))
        NM_FAIL(ctx, NM_ERR_LATTICE, "%s: the lattice has 2^%d superblocks, the neighbor index takes at most 2^%d",
                who, L->bx + L->by + L->bz, NM_DENSE_LOG2);
    *P = nbr_plan(*L);
    if (!d_work || work_bytes < P->bytes) NM_FAIL(ctx, NM_ERR_WORKSPACE, "%s: workspace too small", who);
    return NM_OK;
}

}  // namespace

extern "C" size_t nm_neighbor_index_workspace_bytes(int64_t n_search, const nm_lattice* lat)
{
    if (n_search < 0 || validate_lattice(nullptr, lat) != NM_OK) return 0;
    const LatticeDev L = make_lattice_dev(lat);
    if (!nbr_in_range(L)) return 0;
    return nbr_plan(L).bytes;       // (a function of the lattice alone: every superblock has its leaf)
}

extern "C" int nm_neighbor_index_build(nm_ctx* ctx, const double* d_search, int64_t n_search,
                                       int64_t search_stride, const nm_lattice* lat, int64_t* d_count,
                                       void* d_work, size_t work_bytes, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (n_search < 0 || n_search >= (int64_t)1 << 31 || search_stride < 3 || (n_search > 0 && !d_search) ||
        !d_count)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_build: bad arguments");
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_build", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)d_work;
    uint32_t* header = (uint32_t*)w;
    uint32_t* leaf = (uint32_t*)(w + P.off_leaf);
    uint32_t* totals = (uint32_t*)(w + P.off_totals);
    uint32_t* partial = (uint32_t*)(w + P.off_partial);
    uint32_t* rank = (uint32_t*)(w + P.off_rank);
    NM_HIP(ctx, hipMemsetAsync(d_count, 0, 2 * sizeof(int64_t), s));
    // header, leaves, totals (with their pad) and the scan's partial sums lie back to back
    NM_HIP(ctx, hipMemsetAsync(w, 0, P.off_rank, s));
    if (n_search == 0) return NM_OK;      // empty leaves: no list ever reads a rank, M = 0
    k_nbr_build<<<(int)((n_search + 255) / 256), 256, 0, s>>>(d_search, n_search, search_stride, L, leaf,
                                                              d_count + 1);
    const int unit_blocks = (int)((P.units + 3) / 4);
    k_nbr_row_totals<<<unit_blocks, 256, 0, s>>>(leaf, L, P.chunk_log2, P.piece_bits, P.units, totals);
    k_nbr_scan_reduce<<<P.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(totals, P.tiles_per_block, P.totals_padded,
                                                                 partial);
    k_nbr_scan_apply<<<P.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(totals, P.tiles_per_block, P.totals_padded,
                                                                partial, header, d_count);
    k_nbr_rank<<<unit_blocks, 256, 0, s>>>(leaf, L, P.chunk_log2, P.piece_bits, P.units, totals, rank);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

extern "C" int nm_neighbor_index_addresses(nm_ctx* ctx, const nm_lattice* lat, const void* d_work,
                                           size_t work_bytes, int64_t* d_addr_out, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (!d_addr_out) NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_addresses: bad arguments");
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_addresses", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    const char* w = (const char*)d_work;
    const uint64_t words = P.superblocks * NM_LEAF_WORDS;
    k_nbr_addresses<<<(unsigned)((words + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        (const uint32_t*)(w + P.off_leaf), (const uint32_t*)(w + P.off_rank), (const uint32_t*)w, L, words,
        d_addr_out, 0xFFFFFFFFu);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

extern "C" int nm_neighbor_index_lists(nm_ctx* ctx, const double* d_query, int64_t n_query, int64_t query_stride,
                                       const nm_lattice* lat, double radius, const void* d_work,
                                       size_t work_bytes, int32_t* d_nbr_count, const int64_t* d_nbr_offsets,
                                       int64_t* d_nbr_index, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (n_query < 0 || query_stride < 3 || (n_query > 0 && !d_query))
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_lists: bad arguments");
    if (!d_nbr_count && !d_nbr_index)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_lists: nothing to write");
    if (d_nbr_index && !d_nbr_offsets)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_lists: index output needs offsets");
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_lists", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    int32_t dmin = 0;
    const int W = nbr_candidate_width(radius, lat->edge, &dmin);
    if (W < 0) NM_FAIL(ctx, NM_ERR_RADIUS, "radius/edge ratio outside the supported range");
    if (n_query == 0) return NM_OK;
    const char* w = (const char*)d_work;
    k_nbr_lists<<<(unsigned)((n_query + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        d_query, n_query, query_stride, (const uint32_t*)(w + P.off_leaf), (const uint32_t*)(w + P.off_rank), L,
        radius * radius, dmin, W, d_nbr_count, d_nbr_offsets, d_nbr_index);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

// ---- attributes on the index (additive within ABI 7) -------------------------------------------------------------------

extern "C" int nm_neighbor_index_voxel_of(nm_ctx* ctx, const double* d_points, int64_t n, int64_t stride,
                                          const nm_lattice* lat, const void* d_work, size_t work_bytes,
                                          int64_t* d_voxel, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (n < 0 || stride < 3 || (n > 0 && (!d_points || !d_voxel)))
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_voxel_of: bad arguments");
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_voxel_of", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    if (n == 0) return NM_OK;
    const char* w = (const char*)d_work;
    k_nbr_voxel_of<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        d_points, n, stride, L, (const uint32_t*)(w + P.off_leaf), (const uint32_t*)(w + P.off_rank), d_voxel);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

extern "C" size_t nm_neighbor_index_group_workspace_bytes(int64_t n_points)
{
    if (n_points < 0 || n_points >= (int64_t)1 << 31) return 0;
    return grp_plan(n_points, n_points).bytes;
}

extern "C" int nm_neighbor_index_group(nm_ctx* ctx, const int64_t* d_voxel, int64_t n, int64_t m,
                                       int64_t* d_counts, int64_t* d_start, int64_t* d_rows, void* d_tmp,
                                       size_t tmp_bytes, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (n < 0 || n >= (int64_t)1 << 31 || m < 0 || m >= (int64_t)1 << 31 || (n > 0 && (!d_voxel || !d_rows)) ||
        (m > 0 && !d_counts) || !d_start)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_group: bad arguments");
    const GrpPlan G = grp_plan(n, m);
    if (!d_tmp || tmp_bytes < G.bytes) NM_FAIL(ctx, NM_ERR_WORKSPACE, "nm_neighbor_index_group: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)d_tmp;
    uint32_t* header = (uint32_t*)w;
    uint32_t* partial = (uint32_t*)(w + G.off_partial);
    uint32_t* longs = (uint32_t*)(w + G.off_longs);
    uint32_t* cursor = (uint32_t*)(w + G.off_cursor);
    const unsigned row_blocks = (unsigned)((n + 255) / 256), voxel_blocks = (unsigned)((m + 1 + 255) / 256);
    k_grp_zero<<<(unsigned)((G.cursor_len + 255) / 256), 256, 0, s>>>(header, cursor, G.cursor_len);
    if (n > 0) k_grp_count<<<row_blocks, 256, 0, s>>>(d_voxel, n, m, cursor);
    if (m > 0) k_grp_put_counts<<<voxel_blocks, 256, 0, s>>>(cursor, m, d_counts);
    k_nbr_scan_reduce<<<G.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(cursor, G.tiles_per_block, G.cursor_len, partial);
    k_nbr_scan_apply<<<G.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(cursor, G.tiles_per_block, G.cursor_len, partial,
                                                                header, (int64_t*)(w + 16));
    k_grp_put_start<<<voxel_blocks, 256, 0, s>>>(cursor, header, m, d_start);
    if (n > 0 && m > 0) {
        k_grp_fill<<<row_blocks, 256, 0, s>>>(d_voxel, n, m, cursor, d_rows);
        k_grp_order_short<<<voxel_blocks, 256, 0, s>>>(d_start, m, d_rows, header, longs);
        if (n > GRP_SHORT) {
            const int64_t most = n / (GRP_SHORT + 1);
            k_grp_order_long<<<(unsigned)(most < GRP_LONG_BLOCKS ? most : GRP_LONG_BLOCKS), 256, 0, s>>>(
                d_start, d_rows, header, longs);
        }
    }
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

extern "C" int nm_neighbor_index_voxel_reduce(nm_ctx* ctx, const int64_t* d_start, const int64_t* d_rows, int64_t m,
                                              const double* d_attr, int64_t attr_stride, int32_t dims, int32_t op,
                                              double* d_out, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (m < 0 || m >= (int64_t)1 << 31 || dims < 1 || dims > NM_STATS_MAX_DIMS || attr_stride < dims || !d_start ||
        (m > 0 && (!d_rows || !d_attr || !d_out)) || op < NM_REDUCE_MEAN || op > NM_REDUCE_MAX)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_voxel_reduce: bad arguments");
    if (m == 0) return NM_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((m * dims + 255) / 256);
#define NM_REDUCE_LAUNCH(OP) \
    k_nbr_voxel_reduce<OP><<<blocks, 256, 0, s>>>(d_start, d_rows, m, d_attr, attr_stride, dims, d_out)
    switch (op) {
    case NM_REDUCE_MEAN: NM_REDUCE_LAUNCH(GRP_MEAN); break;
    case NM_REDUCE_SUM: NM_REDUCE_LAUNCH(GRP_SUM); break;
    case NM_REDUCE_MIN: NM_REDUCE_LAUNCH(GRP_MIN); break;
    default: NM_REDUCE_LAUNCH(GRP_MAX); break;
    }
#undef NM_REDUCE_LAUNCH
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

extern "C" int nm_neighbor_index_stats(nm_ctx* ctx, const double* d_query, int64_t n_query, int64_t query_stride,
                                       const nm_lattice* lat, double radius, const void* d_work, size_t work_bytes,
                                       const double* d_values, int64_t value_stride, int32_t dims, int32_t* d_count,
                                       double* d_mean, double* d_min, double* d_max, int64_t out_stride,
                                       void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (n_query < 0 || query_stride < 3 || (n_query > 0 && !d_query) || dims < 1 || dims > NM_STATS_MAX_DIMS ||
        value_stride < dims || !d_values)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_stats: bad arguments");
    if (!d_count && !d_mean && !d_min && !d_max)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_stats: nothing to write");
    if ((d_mean || d_min || d_max) && out_stride < dims)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_stats: output stride below the column count");
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_stats", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    int32_t dmin = 0;
    const int W = nbr_candidate_width(radius, lat->edge, &dmin);
    if (W < 0) NM_FAIL(ctx, NM_ERR_RADIUS, "radius/edge ratio outside the supported range");
    if (n_query == 0) return NM_OK;
    const char* w = (const char*)d_work;
    const uint32_t* leaf = (const uint32_t*)(w + P.off_leaf);
    const uint32_t* rank = (const uint32_t*)(w + P.off_rank);
    const unsigned blocks = (unsigned)((n_query + 255) / 256);
#define NM_STATS_LAUNCH(DB)                                                                                       \
    k_nbr_stats<DB><<<blocks, 256, 0, (hipStream_t)stream>>>(d_query, n_query, query_stride, leaf, rank, L,       \
                                                             radius * radius, dmin, W, d_values, value_stride,    \
                                                             dims, d_count, d_mean, d_min, d_max, out_stride)
    if (dims == 1) NM_STATS_LAUNCH(1);
    else if (dims <= 4) NM_STATS_LAUNCH(4);
    else NM_STATS_LAUNCH(16);
#undef NM_STATS_LAUNCH
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

// ---- nearest voxels on the index (additive within ABI 7) ----------------------------------------------------------------

extern "C" size_t nm_neighbor_index_nearest_workspace_bytes(int64_t n_query)
{
    if (n_query < 0 || n_query >= (int64_t)1 << 31) return 0;
    return NN_HEADER_BYTES + ((size_t)n_query * sizeof(uint2) + 15) / 16 * 16;
}

extern "C" int nm_neighbor_index_nearest(nm_ctx* ctx, const double* d_query, int64_t n_query, int64_t query_stride,
                                         const nm_lattice* lat, int32_t k, double max_distance, const void* d_work,
                                         size_t work_bytes, double* d_dist2, int64_t* d_index, int64_t out_stride,
                                         int32_t* d_found, void* d_tmp, size_t tmp_bytes, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (n_query < 0 || n_query >= (int64_t)1 << 31 || query_stride < 3 || (n_query > 0 && !d_query))
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_nearest: bad arguments");
    if (k < 1 || k > NM_NEAREST_MAX_K)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_nearest: k = %d outside [1, %d]", k, NM_NEAREST_MAX_K);
    if (!d_dist2 && !d_index) NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_nearest: nothing to write");
    if (out_stride < k)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_nearest: output stride below k");
    if (!(max_distance >= 0.0))      // (NaN fails)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_nearest: max_distance must be >= 0 (INFINITY: no limit)");
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_nearest", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    int32_t s_limit = -1;
    if (max_distance < INFINITY) {
        int32_t dmin = 0;
        if (nbr_candidate_width(max_distance, lat->edge, &dmin) < 0)
            NM_FAIL(ctx, NM_ERR_RADIUS, "max_distance/edge ratio outside the supported range");
        s_limit = -dmin;
    }
    if (n_query == 0) return NM_OK;
    if (!d_tmp || tmp_bytes < nm_neighbor_index_nearest_workspace_bytes(n_query))
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_nearest: temporary workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const char* w = (const char*)d_work;
    NnArgs A;
    A.query = d_query;
    A.nq = n_query;
    A.qstride = query_stride;
    A.leaf = (const uint32_t*)(w + P.off_leaf);
    A.rank = (const uint32_t*)(w + P.off_rank);
    A.totals = (const uint32_t*)(w + P.off_totals);
    A.header = (const uint32_t*)w;
    A.L = L;
    A.chunk_log2 = P.chunk_log2;
    A.piece_bits = P.piece_bits;
    A.n_totals = P.totals;
    A.k = k;
    A.s_limit = s_limit;
    A.r2 = max_distance * max_distance;
    A.dist2 = d_dist2;
    A.index = d_index;
    A.ostride = out_stride;
    A.found = d_found;
    A.pend_count = (uint32_t*)d_tmp;
    A.pend = (uint2*)((char*)d_tmp + NN_HEADER_BYTES);
    // a limit whose window the near stage reaches leaves nothing for the wide stage
    const bool wide = s_limit < 0 || s_limit > NN_NEAR_CAP;
    if (wide) NM_HIP(ctx, hipMemsetAsync(d_tmp, 0, NN_HEADER_BYTES, s));
    const unsigned near_blocks = (unsigned)((n_query + 255) / 256), wide_blocks = (unsigned)((n_query + 63) / 64);
#define NM_NEAREST_LAUNCH(K)                                         \
    do {                                                             \
        k_nn_near<K><<<near_blocks, 256, 0, s>>>(A);                 \
        if (wide) k_nn_wide<K><<<wide_blocks, 64, 0, s>>>(A);        \
    } while (0)
    if (k == 1) NM_NEAREST_LAUNCH(1);
    else if (k <= 8) NM_NEAREST_LAUNCH(8);
    else if (k <= 16) NM_NEAREST_LAUNCH(16);
    else NM_NEAREST_LAUNCH(32);
#undef NM_NEAREST_LAUNCH
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

// ---- connected components of the voxel graph (additive within ABI 7) ---------------------------------------------------

extern "C" size_t nm_neighbor_index_components_workspace_bytes(int64_t n_voxels)
{
    if (n_voxels < 0 || n_voxels >= (int64_t)1 << 31) return 0;
    return cc_plan(n_voxels).bytes;
}

extern "C" int nm_neighbor_index_components(nm_ctx* ctx, const nm_lattice* lat, double radius, const void* d_work,
                                            size_t work_bytes, const int64_t* d_class, const int64_t* d_weight,
                                            int64_t min_size, int64_t* d_label, int64_t* d_size, int64_t* d_count,
                                            void* d_tmp, size_t tmp_bytes, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (!d_label || !d_size || !d_count) NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_components: bad arguments");
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_components", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    int32_t dmin = 0;
    const int W = radius >= 0.0 ? nbr_candidate_width(radius, lat->edge, &dmin) : -1;      // (NaN fails)
    if (W < 0) NM_FAIL(ctx, NM_ERR_RADIUS, "radius/edge ratio outside the supported range");
    if (!d_tmp || tmp_bytes < cc_plan(0).bytes)
        NM_FAIL(ctx, NM_ERR_WORKSPACE, "nm_neighbor_index_components: temporary workspace too small");
    const CcPlan C = cc_plan_of(tmp_bytes);
    hipStream_t s = (hipStream_t)stream;
    const char* w = (const char*)d_work;
    const uint32_t* index_header = (const uint32_t*)w;
    const uint32_t* leaf = (const uint32_t*)(w + P.off_leaf);
    const uint32_t* rank = (const uint32_t*)(w + P.off_rank);
    char* t = (char*)d_tmp;
    uint32_t* header = (uint32_t*)t;
    uint32_t* partial = (uint32_t*)(t + C.off_partial);
    int64_t* addr = (int64_t*)(t + C.off_addr);
    int64_t* size = (int64_t*)(t + C.off_size);
    uint32_t* parent = (uint32_t*)(t + C.off_parent);
    uint32_t* keep = (uint32_t*)(t + C.off_keep);
    const uint32_t room = (uint32_t)C.room;
    const unsigned blocks = (unsigned)(C.room / 256);
    const uint64_t words = P.superblocks * NM_LEAF_WORDS;
    k_nbr_addresses<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(leaf, rank, index_header, L, words, addr, room);
    k_cc_init<<<blocks, 256, 0, s>>>(index_header, room, d_class, parent, keep, size, d_count);
    k_cc_link<<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, radius * radius, dmin, W, d_class,
                                     parent);
    k_cc_flatten<<<(unsigned)(C.room / CC_FLAT_THREADS), CC_FLAT_THREADS, 0, s>>>(index_header, room, d_weight,
                                                                                  parent, size);
    k_cc_mark<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_count);
    k_nbr_scan_reduce<<<C.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(keep, C.tiles_per_block, C.room, partial);
    k_nbr_scan_apply<<<C.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(keep, C.tiles_per_block, C.room, partial, header,
                                                                d_count);
    k_cc_label<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_label, d_size, d_count);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

// ---- density-based clusters of the voxel graph (additive within ABI 7) -------------------------------------------------

extern "C" size_t nm_neighbor_index_dbscan_workspace_bytes(int64_t n_voxels)
{
    if (n_voxels < 0 || n_voxels >= (int64_t)1 << 31) return 0;
    return db_plan(n_voxels).bytes;
}

extern "C" int nm_neighbor_index_dbscan(nm_ctx* ctx, const nm_lattice* lat, double radius, int64_t min_weight,
                                        const void* d_work, size_t work_bytes, const int64_t* d_class,
                                        const int64_t* d_weight, int64_t min_size, int64_t* d_label,
                                        int64_t* d_size, uint8_t* d_core, int64_t* d_density, int64_t* d_count,
                                        void* d_tmp, size_t tmp_bytes, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (!d_label || !d_size || !d_core || !d_count)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_dbscan: bad arguments");
    if (!(radius >= 0.0))      // (NaN fails)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_dbscan: radius must be >= 0");
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_dbscan", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    int32_t dmin = 0;
    const int W = nbr_candidate_width(radius, lat->edge, &dmin);
    if (W < 0) NM_FAIL(ctx, NM_ERR_RADIUS, "radius/edge ratio outside the supported range");
    if (!d_tmp || tmp_bytes < db_plan(0).bytes)
        NM_FAIL(ctx, NM_ERR_WORKSPACE, "nm_neighbor_index_dbscan: temporary workspace too small");
    const DbPlan D = db_plan_of(tmp_bytes);
    const CcPlan& C = D.C;
    hipStream_t s = (hipStream_t)stream;
    const char* w = (const char*)d_work;
    const uint32_t* index_header = (const uint32_t*)w;
    const uint32_t* leaf = (const uint32_t*)(w + P.off_leaf);
    const uint32_t* rank = (const uint32_t*)(w + P.off_rank);
    char* t = (char*)d_tmp;
    uint32_t* header = (uint32_t*)t;
    uint32_t* partial = (uint32_t*)(t + C.off_partial);
    int64_t* addr = (int64_t*)(t + C.off_addr);
    int64_t* size = (int64_t*)(t + C.off_size);
    uint32_t* parent = (uint32_t*)(t + C.off_parent);
    uint32_t* keep = (uint32_t*)(t + C.off_keep);
    int64_t* eff = (int64_t*)(t + D.off_eff);
    const uint32_t room = (uint32_t)C.room;
    const unsigned blocks = (unsigned)(C.room / 256);
    const uint64_t words = P.superblocks * NM_LEAF_WORDS;
    const double r2 = radius * radius;
    k_nbr_addresses<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(leaf, rank, index_header, L, words, addr, room);
    k_db_density<<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, r2, dmin, W, d_class, d_weight,
                                        min_weight, d_density, d_core, eff, d_count);
    // the core clusters: components on the effective classes
    k_cc_init<<<blocks, 256, 0, s>>>(index_header, room, eff, parent, keep, size, d_count);
    k_cc_link<<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, r2, dmin, W, eff, parent);
    k_db_border<<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, r2, dmin, W, d_class, eff, parent,
                                       d_count);
    k_cc_flatten<<<(unsigned)(C.room / CC_FLAT_THREADS), CC_FLAT_THREADS, 0, s>>>(index_header, room, d_weight,
                                                                                  parent, size);
    k_cc_mark<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_count);
    k_nbr_scan_reduce<<<C.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(keep, C.tiles_per_block, C.room, partial);
    k_nbr_scan_apply<<<C.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(keep, C.tiles_per_block, C.room, partial, header,
                                                                d_count);
    k_cc_label<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_label, d_size, d_count);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

// ---- smoothness-constrained regions of the voxel graph (additive within ABI 7) ------------------------------------------

extern "C" size_t nm_neighbor_index_regions_workspace_bytes(int64_t n_voxels)
{
    if (n_voxels < 0 || n_voxels >= (int64_t)1 << 31) return 0;
    return db_plan(n_voxels).bytes;
}

namespace {

template <bool NORMAL>
void rg_launch_link(int32_t dims, unsigned blocks, hipStream_t s, const int64_t* addr, const uint32_t* index_header,
                    uint32_t room, const uint32_t* leaf, const uint32_t* rank, const LatticeDev& L, double r2,
                    int32_t dmin, int32_t W, const int64_t* eff, const double* normal, int64_t normal_stride,
                    double min_cos, const double* value, int64_t value_stride, const RgStep& step, uint32_t* parent)
{
#define RG_LINK(D)                                                                                                   \
    k_rg_link<NORMAL, D><<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, r2, dmin, W, eff, normal,  \
                                                normal_stride, min_cos, value, value_stride, step, parent)
    switch (dims) {
    case 0: RG_LINK(0); break;
    case 1: RG_LINK(1); break;
    case 2: RG_LINK(2); break;
    case 3: RG_LINK(3); break;
    default: RG_LINK(4); break;
    }
#undef RG_LINK
}

}  // namespace

extern "C" int nm_neighbor_index_regions(nm_ctx* ctx, const nm_lattice* lat, double radius, const void* d_work,
                                         size_t work_bytes, const int64_t* d_class, const int64_t* d_weight,
                                         const uint8_t* d_seed, const double* d_normal, int64_t normal_stride,
                                         double min_cos, const double* d_value, int64_t value_stride, int32_t dims,
                                         const double* max_step, int64_t min_size, int64_t* d_label,
                                         int64_t* d_size, int64_t* d_count, void* d_tmp, size_t tmp_bytes,
                                         void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (!d_label || !d_size || !d_count) NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_regions: bad arguments");
    if (!(radius >= 0.0))      // (NaN fails)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_regions: radius must be >= 0");
    if (dims < 0 || dims > NM_REGION_MAX_DIMS)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_regions: dims = %d outside [0, %d]", dims,
                NM_REGION_MAX_DIMS);
    if (dims > 0 && (!d_value || !max_step || value_stride < dims))
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_regions: %d value columns need d_value, max_step and a "
                "stride of at least %d", dims, dims);
    if (d_normal && (normal_stride < 3 || min_cos != min_cos))
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_regions: normals need a stride of at least 3 and a min_cos "
                "that is a number");
    RgStep step = {};
    for (int32_t k = 0; k < dims; ++k) {
        if (!(max_step[k] >= 0.0))      // (NaN fails)
            NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_regions: max_step[%d] must be >= 0", k);
        step.s[k] = max_step[k];
    }
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_regions", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    int32_t dmin = 0;
    const int W = nbr_candidate_width(radius, lat->edge, &dmin);
    if (W < 0) NM_FAIL(ctx, NM_ERR_RADIUS, "radius/edge ratio outside the supported range");
    if (!d_tmp || tmp_bytes < db_plan(0).bytes)
        NM_FAIL(ctx, NM_ERR_WORKSPACE, "nm_neighbor_index_regions: temporary workspace too small");
    const DbPlan D = db_plan_of(tmp_bytes);
    const CcPlan& C = D.C;
    hipStream_t s = (hipStream_t)stream;
    const char* w = (const char*)d_work;
    const uint32_t* index_header = (const uint32_t*)w;
    const uint32_t* leaf = (const uint32_t*)(w + P.off_leaf);
    const uint32_t* rank = (const uint32_t*)(w + P.off_rank);
    char* t = (char*)d_tmp;
    uint32_t* header = (uint32_t*)t;
    uint32_t* partial = (uint32_t*)(t + C.off_partial);
    int64_t* addr = (int64_t*)(t + C.off_addr);
    int64_t* size = (int64_t*)(t + C.off_size);
    uint32_t* parent = (uint32_t*)(t + C.off_parent);
    uint32_t* keep = (uint32_t*)(t + C.off_keep);
    int64_t* eff = (int64_t*)(t + D.off_eff);
    const uint32_t room = (uint32_t)C.room;
    const unsigned blocks = (unsigned)(C.room / 256);
    const uint64_t words = P.superblocks * NM_LEAF_WORDS;
    const double r2 = radius * radius;
    k_nbr_addresses<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(leaf, rank, index_header, L, words, addr, room);
    k_rg_seed<<<blocks, 256, 0, s>>>(index_header, room, d_class, d_seed, eff, d_count);
    // the regions of the seeds: components on the effective classes, under the edges the predicate lets through
    k_cc_init<<<blocks, 256, 0, s>>>(index_header, room, eff, parent, keep, size, d_count);
    if (d_normal)
        rg_launch_link<true>(dims, blocks, s, addr, index_header, room, leaf, rank, L, r2, dmin, W, eff, d_normal,
                             normal_stride, min_cos, d_value, value_stride, step, parent);
    else
        rg_launch_link<false>(dims, blocks, s, addr, index_header, room, leaf, rank, L, r2, dmin, W, eff, nullptr, 0,
                              0.0, d_value, value_stride, step, parent);
    k_db_border<<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, r2, dmin, W, d_class, eff, parent,
                                       d_count);
    k_cc_flatten<<<(unsigned)(C.room / CC_FLAT_THREADS), CC_FLAT_THREADS, 0, s>>>(index_header, room, d_weight,
                                                                                  parent, size);
    k_cc_mark<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_count);
    k_nbr_scan_reduce<<<C.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(keep, C.tiles_per_block, C.room, partial);
    k_nbr_scan_apply<<<C.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(keep, C.tiles_per_block, C.room, partial, header,
                                                                d_count);
    k_cc_label<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_label, d_size, d_count);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

// ---- peak-seeking segments of the voxel graph (additive within ABI 7) -------------------------------------------------

extern "C" size_t nm_neighbor_index_hill_climb_workspace_bytes(int64_t n_voxels)
{
    if (n_voxels < 0 || n_voxels >= (int64_t)1 << 31) return 0;
    return cc_plan(n_voxels).bytes;
}

extern "C" int nm_neighbor_index_hill_climb(nm_ctx* ctx, const nm_lattice* lat, double radius, int32_t mode,
                                            const void* d_work, size_t work_bytes, const double* d_value,
                                            const int64_t* d_class, const int64_t* d_weight, int64_t min_size,
                                            int64_t* d_label, int64_t* d_size, int64_t* d_peak, int64_t* d_link,
                                            int64_t* d_count, void* d_tmp, size_t tmp_bytes, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (!d_value || !d_label || !d_size || !d_peak || !d_count)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_hill_climb: bad arguments");
    if (mode != NM_CLIMB_HIGHEST && mode != NM_CLIMB_NEAREST)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_hill_climb: mode = %d is neither NM_CLIMB_HIGHEST nor "
                "NM_CLIMB_NEAREST", mode);
    if (!(radius >= 0.0))      // (NaN fails)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_hill_climb: radius must be >= 0");
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_hill_climb", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    int32_t dmin = 0;
    const int W = nbr_candidate_width(radius, lat->edge, &dmin);
    if (W < 0) NM_FAIL(ctx, NM_ERR_RADIUS, "radius/edge ratio outside the supported range");
    if (!d_tmp || tmp_bytes < cc_plan(0).bytes)
        NM_FAIL(ctx, NM_ERR_WORKSPACE, "nm_neighbor_index_hill_climb: temporary workspace too small");
    const CcPlan C = cc_plan_of(tmp_bytes);
    hipStream_t s = (hipStream_t)stream;
    const char* w = (const char*)d_work;
    const uint32_t* index_header = (const uint32_t*)w;
    const uint32_t* leaf = (const uint32_t*)(w + P.off_leaf);
    const uint32_t* rank = (const uint32_t*)(w + P.off_rank);
    char* t = (char*)d_tmp;
    uint32_t* header = (uint32_t*)t;
    uint32_t* partial = (uint32_t*)(t + C.off_partial);
    int64_t* addr = (int64_t*)(t + C.off_addr);
    int64_t* size = (int64_t*)(t + C.off_size);
    uint32_t* parent = (uint32_t*)(t + C.off_parent);
    uint32_t* keep = (uint32_t*)(t + C.off_keep);
    const uint32_t room = (uint32_t)C.room;
    const unsigned blocks = (unsigned)(C.room / 256);
    const uint64_t words = P.superblocks * NM_LEAF_WORDS;
    const double r2 = radius * radius;
    k_nbr_addresses<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(leaf, rank, index_header, L, words, addr, room);
    // the forest: every voxel's uphill link (in the place of k_cc_init and k_cc_link)
    if (mode == NM_CLIMB_NEAREST)
        k_hc_parent<true><<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, r2, dmin, W, d_class,
                                                 d_value, parent, keep, size, d_link, d_count);
    else
        k_hc_parent<false><<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, r2, dmin, W, d_class,
                                                  d_value, parent, keep, size, d_link, d_count);
    k_cc_flatten<<<(unsigned)(C.room / CC_FLAT_THREADS), CC_FLAT_THREADS, 0, s>>>(index_header, room, d_weight,
                                                                                  parent, size);
    k_cc_mark<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_count);
    k_nbr_scan_reduce<<<C.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(keep, C.tiles_per_block, C.room, partial);
    k_nbr_scan_apply<<<C.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(keep, C.tiles_per_block, C.room, partial, header,
                                                                d_count);
    k_cc_label<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_label, d_size, d_count);
    k_hc_peaks<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_peak);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

// ---- the adjacency of a labelling of the voxel graph (additive within ABI 7) -------------------------------------------

extern "C" size_t nm_neighbor_index_adjacency_workspace_bytes(int64_t n_voxels, int64_t n_records)
{
    const int64_t most = (int64_t)1 << 31;
    if (n_voxels < 0 || n_voxels >= most || n_records < 0 || n_records >= most) return 0;
    const size_t walk = adj_plan(n_voxels).bytes, rows = adj_rows(n_records).bytes;
    return walk > rows ? walk : rows;
}

extern "C" int nm_neighbor_index_adjacency(nm_ctx* ctx, const nm_lattice* lat, double radius, const void* d_work,
                                           size_t work_bytes, const int64_t* d_label, const double* d_value,
                                           const int64_t* d_class, int64_t capacity, int64_t* d_key,
                                           int64_t* d_links, double* d_saddle, int64_t* d_count, void* d_tmp,
                                           size_t tmp_bytes, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (!d_label || !d_count) NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_adjacency: bad arguments");
    const bool emit = d_key != nullptr;
    if (emit && (!d_links || capacity < 0 || (d_value != nullptr) != (d_saddle != nullptr)))
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_adjacency: the records need d_key, d_links, a capacity >= 0 "
                "and d_saddle exactly where d_value is given");
    if (!emit && (d_links || d_saddle))
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_adjacency: d_links or d_saddle without d_key");
    if (!(radius >= 0.0))      // (NaN fails)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_adjacency: radius must be >= 0");
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_adjacency", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    int32_t dmin = 0;
    const int W = nbr_candidate_width(radius, lat->edge, &dmin);
    if (W < 0) NM_FAIL(ctx, NM_ERR_RADIUS, "radius/edge ratio outside the supported range");
    if (!d_tmp || tmp_bytes < adj_plan(0).bytes)
        NM_FAIL(ctx, NM_ERR_WORKSPACE, "nm_neighbor_index_adjacency: temporary workspace too small");
    const AdjPlan A = adj_plan_of(tmp_bytes);
    // the scan counts in 32 bits: no voxel has more records than the forward half of its window has cells
    if ((double)A.room * (0.5 * (double)W * (double)W * (double)W) >= 4294967296.0)
        NM_FAIL(ctx, NM_ERR_RADIUS, "nm_neighbor_index_adjacency: %lld voxels with %d^3 candidates each could cross "
                "2^32 edges", (long long)A.room, W);
    hipStream_t s = (hipStream_t)stream;
    const char* w = (const char*)d_work;
    const uint32_t* index_header = (const uint32_t*)w;
    const uint32_t* leaf = (const uint32_t*)(w + P.off_leaf);
    const uint32_t* rank = (const uint32_t*)(w + P.off_rank);
    char* t = (char*)d_tmp;
    uint32_t* header = (uint32_t*)t;
    uint32_t* partial = (uint32_t*)(t + A.off_partial);
    int64_t* addr = (int64_t*)(t + A.off_addr);
    uint32_t* count = (uint32_t*)(t + A.off_count);
    const uint32_t room = (uint32_t)A.room;
    const unsigned blocks = (unsigned)(A.room / 256);
    const double r2 = radius * radius;
    if (emit) {
        // addr[], the scanned count[] and header[0] are the count call's
        k_adj_walk<true><<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, r2, dmin, W, d_label, d_class,
                                                d_value, count, header, capacity, d_key, d_links, d_saddle, d_count);
        NM_HIP(ctx, hipGetLastError());
        return NM_OK;
    }
    const uint64_t words = P.superblocks * NM_LEAF_WORDS;
    NM_HIP(ctx, hipMemsetAsync(d_count, 0, 2 * sizeof(int64_t), s));
    k_nbr_addresses<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(leaf, rank, index_header, L, words, addr, room);
    k_adj_walk<false><<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, r2, dmin, W, d_label, d_class,
                                             d_value, count, header, 0, nullptr, nullptr, nullptr, d_count);
    k_nbr_scan_reduce<<<A.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(count, A.tiles_per_block, A.room, partial);
    k_nbr_scan_apply<<<A.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(count, A.tiles_per_block, A.room, partial, header,
                                                                d_count);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

extern "C" int nm_neighbor_index_adjacency_reduce(nm_ctx* ctx, int64_t n_records, const int64_t* d_key,
                                                  const int64_t* d_order, const int64_t* d_links_in,
                                                  const double* d_saddle_in, int64_t* d_pair, int64_t* d_links,
                                                  double* d_saddle, int64_t* d_count, void* d_tmp, size_t tmp_bytes,
                                                  void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (n_records < 0 || n_records >= (int64_t)1 << 31 || !d_count ||
        (n_records > 0 && (!d_key || !d_links_in || !d_pair || !d_links)) ||
        (d_saddle_in != nullptr) != (d_saddle != nullptr))
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_adjacency_reduce: bad arguments");
    const AdjRows R = adj_rows(n_records);
    if (!d_tmp || tmp_bytes < R.bytes)
        NM_FAIL(ctx, NM_ERR_WORKSPACE, "nm_neighbor_index_adjacency_reduce: temporary workspace too small");
    hipStream_t s = (hipStream_t)stream;
    NM_HIP(ctx, hipMemsetAsync(d_count, 0, 2 * sizeof(int64_t), s));
    if (n_records == 0) return NM_OK;
    char* t = (char*)d_tmp;
    uint32_t* header = (uint32_t*)t;
    uint32_t* partial = (uint32_t*)(t + R.off_partial);
    uint32_t* row = (uint32_t*)(t + R.off_row);
    unsigned long long* image = (unsigned long long*)d_saddle;
    const unsigned blocks = (unsigned)(R.rpad / 256);
    k_adj_heads<<<blocks, 256, 0, s>>>(d_key, n_records, R.rpad, row, d_links, image);
    k_nbr_scan_reduce<<<R.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(row, R.tiles_per_block, R.rpad, partial);
    k_nbr_scan_apply<<<R.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(row, R.tiles_per_block, R.rpad, partial, header,
                                                                d_count);
    k_adj_reduce<<<blocks, 256, 0, s>>>(d_key, d_order, d_links_in, d_saddle_in, n_records, row, d_pair, d_links,
                                        image);
    if (image) k_adj_saddles<<<blocks, 256, 0, s>>>(header, image);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

// ---- shortest paths from seeds over the voxel graph (additive within ABI 7) ---------------------------------------------

extern "C" size_t nm_neighbor_index_geodesic_workspace_bytes(int64_t n_voxels)
{
    if (n_voxels < 0 || n_voxels >= (int64_t)1 << 31) return 0;
    return cc_plan(n_voxels).bytes;
}

extern "C" int nm_neighbor_index_geodesic_relax(nm_ctx* ctx, const nm_lattice* lat, double radius, const void* d_work,
                                                size_t work_bytes, const uint8_t* d_seed, const int64_t* d_class,
                                                double max_distance, int32_t first, int32_t sweeps, double* d_dist,
                                                int64_t* d_count, void* d_tmp, size_t tmp_bytes, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (!d_seed || !d_dist || !d_count) NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_geodesic_relax: bad arguments");
    if (!(radius >= 0.0))      // (NaN fails)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_geodesic_relax: radius must be >= 0");
    if (!(max_distance >= 0.0))
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_geodesic_relax: max_distance must be >= 0 (+inf: no limit)");
    if (sweeps < 1) NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_geodesic_relax: sweeps = %d, must be >= 1", sweeps);
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_geodesic_relax", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    int32_t dmin = 0;
    const int W = nbr_candidate_width(radius, lat->edge, &dmin);
    if (W < 0) NM_FAIL(ctx, NM_ERR_RADIUS, "radius/edge ratio outside the supported range");
    if (!d_tmp || tmp_bytes < cc_plan(0).bytes)
        NM_FAIL(ctx, NM_ERR_WORKSPACE, "nm_neighbor_index_geodesic_relax: temporary workspace too small");
    const CcPlan C = cc_plan_of(tmp_bytes);
    hipStream_t s = (hipStream_t)stream;
    const char* w = (const char*)d_work;
    const uint32_t* index_header = (const uint32_t*)w;
    const uint32_t* leaf = (const uint32_t*)(w + P.off_leaf);
    const uint32_t* rank = (const uint32_t*)(w + P.off_rank);
    char* t = (char*)d_tmp;
    unsigned long long* counter = (unsigned long long*)(t + GEO_COUNTER_BYTES);
    int64_t* addr = (int64_t*)(t + C.off_addr);
    const uint32_t room = (uint32_t)C.room;
    const unsigned blocks = (unsigned)(C.room / 256);
    const double r2 = radius * radius;
    NM_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
    NM_HIP(ctx, hipMemsetAsync(counter, 0, 3 * sizeof(unsigned long long), s));
    if (first) {
        const uint64_t words = P.superblocks * NM_LEAF_WORDS;
        k_nbr_addresses<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(leaf, rank, index_header, L, words, addr,
                                                                        room);
        k_geo_init<<<blocks, 256, 0, s>>>(index_header, room, d_seed, d_class, d_dist);
    }
    for (int32_t j = 0; j < sweeps; ++j)
        k_geo_sweep<<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, r2, dmin, W, d_class, max_distance,
                                           d_dist, j > 0 ? counter + (j - 1) % 3 : nullptr,
                                           j + 1 < sweeps ? counter + j % 3 : (unsigned long long*)d_count,
                                           counter + (j + 1) % 3);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}

extern "C" int nm_neighbor_index_geodesic_finish(nm_ctx* ctx, const nm_lattice* lat, double radius, const void* d_work,
                                                 size_t work_bytes, const int64_t* d_class, const int64_t* d_weight,
                                                 int64_t min_size, const double* d_dist, int64_t* d_label,
                                                 int64_t* d_size, int64_t* d_source, int64_t* d_link,
                                                 int64_t* d_count, void* d_tmp, size_t tmp_bytes, void* stream)
{
    NM_ENTER_STREAM(ctx, stream);
    if (!d_dist || !d_label || !d_size || !d_source || !d_count)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_geodesic_finish: bad arguments");
    if (!(radius >= 0.0))      // (NaN fails)
        NM_FAIL(ctx, NM_ERR_INVALID, "nm_neighbor_index_geodesic_finish: radius must be >= 0");
    LatticeDev L;
    NbrPlan P;
    int rc = nbr_check_index(ctx, "nm_neighbor_index_geodesic_finish", lat, d_work, work_bytes, &L, &P);
    if (rc) return rc;
    int32_t dmin = 0;
    const int W = nbr_candidate_width(radius, lat->edge, &dmin);
    if (W < 0) NM_FAIL(ctx, NM_ERR_RADIUS, "radius/edge ratio outside the supported range");
    if (!d_tmp || tmp_bytes < cc_plan(0).bytes)
        NM_FAIL(ctx, NM_ERR_WORKSPACE, "nm_neighbor_index_geodesic_finish: temporary workspace too small");
    const CcPlan C = cc_plan_of(tmp_bytes);
    hipStream_t s = (hipStream_t)stream;
    const char* w = (const char*)d_work;
    const uint32_t* index_header = (const uint32_t*)w;
    const uint32_t* leaf = (const uint32_t*)(w + P.off_leaf);
    const uint32_t* rank = (const uint32_t*)(w + P.off_rank);
    char* t = (char*)d_tmp;
    uint32_t* header = (uint32_t*)t;
    uint32_t* partial = (uint32_t*)(t + C.off_partial);
    int64_t* addr = (int64_t*)(t + C.off_addr);
    int64_t* size = (int64_t*)(t + C.off_size);
    uint32_t* parent = (uint32_t*)(t + C.off_parent);
    uint32_t* keep = (uint32_t*)(t + C.off_keep);
    const uint32_t room = (uint32_t)C.room;
    const unsigned blocks = (unsigned)(C.room / 256);
    const uint64_t words = P.superblocks * NM_LEAF_WORDS;
    NM_HIP(ctx, hipMemsetAsync(d_count, 0, 3 * sizeof(int64_t), s));
    // (the addresses again: the call stands on its own, whatever scratch the distances were made with)
    k_nbr_addresses<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(leaf, rank, index_header, L, words, addr, room);
    // the forest: every voxel's link towards its seed (in the place of k_cc_init and k_cc_link)
    k_geo_link<<<blocks, 256, 0, s>>>(addr, index_header, room, leaf, rank, L, radius * radius, dmin, W, d_class,
                                      d_dist, parent, keep, size, d_link, d_count);
    k_cc_flatten<<<(unsigned)(C.room / CC_FLAT_THREADS), CC_FLAT_THREADS, 0, s>>>(index_header, room, d_weight,
                                                                                  parent, size);
    k_geo_orphans<<<blocks, 256, 0, s>>>(index_header, room, d_dist, parent, d_count);
    k_cc_mark<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_count);
    k_nbr_scan_reduce<<<C.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(keep, C.tiles_per_block, C.room, partial);
    k_nbr_scan_apply<<<C.scan_blocks, NBR_SCAN_THREADS, 0, s>>>(keep, C.tiles_per_block, C.room, partial, header,
                                                                d_count);
    k_cc_label<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_label, d_size, d_count);
    k_hc_peaks<<<blocks, 256, 0, s>>>(index_header, room, parent, size, min_size, keep, d_source);
    NM_HIP(ctx, hipGetLastError());
    return NM_OK;
}
