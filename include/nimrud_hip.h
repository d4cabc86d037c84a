/*
 * nimrud_hip.h - C ABI of libnimrud_hip.so: the MI355X (gfx950) implementation of the
 * grayhem/nimrud multiscale neighborhood-feature hot path (nimrud/minimal).
 *
 * The reference has no FFI layer: its boundary is the Python module surface of nimrud.minimal.  Each
 * entry point below names the reference code it replaces (paths relative to the reference checkout).
 * The Python package nimrud_amd binds these with ctypes (nimrud_amd/_ffi.py); INTEGRATION.md shows
 * the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only.  every pointer whose name starts with d_ is DEVICE memory (HBM) owned by the
 *     caller; the library never allocates or frees caller-visible memory.  scratch memory is passed in
 *     as (d_work, work_bytes); its required size comes from the matching *_workspace_bytes function.
 *   - point clouds are row-major fp64 arrays; `stride` is the row pitch in doubles (>= 3), so a
 *     (N, 3+F) cloud with feature columns is passed without a copy (minimal/README.md:38-40).
 *     the feature entry points take row pitches below 2^31 doubles (NM_ERR_INVALID otherwise).
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *     unless documented otherwise, and returns NM_OK or a negative nm_status.
 *     nm_last_error(ctx) returns a human-readable message for the last failure on that context.
 *   - one nm_ctx per (device, host thread).  no global state.
 */
#ifndef NIMRUD_HIP_H
#define NIMRUD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nm_ctx nm_ctx;

typedef enum nm_status {
    NM_OK = 0,
    NM_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, stride < 3 ...)            */
    NM_ERR_LATTICE = -2,     /* lattice cannot be addressed (geometry.py:59-60 ValueError), or is
                                outside the device path's limits (see nm_lattice)                     */
    NM_ERR_WORKSPACE = -3,   /* d_work too small                                                       */
    NM_ERR_HIP = -4,         /* a HIP runtime call failed                                              */
    NM_ERR_RADIUS = -5,      /* radius / edge ratio outside the supported range                        */
    NM_ERR_COMM = -6         /* an RCCL call failed                                                    */
} nm_status;

/*
 * The bounding lattice of one analysis scale: VoxelFilter.__init__ / _calculate_shift
 * (nimrud/utils/geometry.py:23-64).  Filled on the host (nimrud_amd/utils/geometry.py does the same
 * arithmetic as the reference) and passed by pointer.
 *   min_corner = cloud.min(0) - edge/2          geometry.py:37
 *   widths     = ceil(log2(span/edge)) per axis geometry.py:56   (sum <= 64, geometry.py:59)
 *   shifts     = cumsum(widths)[:-1]            geometry.py:62
 * Device-path limits: 3 spatial dimensions, every width in [1, 30].
 */
typedef struct nm_lattice {
    double  min_corner[3];
    double  edge;
    int32_t widths[3];
    int32_t shifts[2];
} nm_lattice;

/* ---- context ---------------------------------------------------------------------------------- */

int         nm_create(nm_ctx** out, int device);
void        nm_destroy(nm_ctx* ctx);
const char* nm_last_error(const nm_ctx* ctx);
/* library ABI version (bumped on any signature change) */
int         nm_abi_version(void);

/* ---- asynchronous failures -------------------------------------------------------------------------
 * every call is asynchronous, so a failure that only a kernel can detect (the occupancy-index builder
 * running out of its bounded wait or of leaves; a lattice built on the device that cannot be addressed,
 * geometry.py:59-60) cannot be the return value of the call that enqueued it.  such a failure is STICKY on
 * the context: the library leaves a snapshot of its device-side status words behind every feature call,
 * and the next nm_* call that launches work - or nm_check - returns NM_ERR_HIP / NM_ERR_LATTICE with a
 * message once that snapshot has arrived, and keeps doing so until nm_clear_error.  results of the
 * failed call must be discarded.  nm_check(ctx, 1) waits for the snapshot of the last call (call it after
 * synchronising the stream, before trusting results); nm_check(ctx, 0) only looks.  no reference
 * counterpart (the reference is synchronous and raises in place).                                     */
int nm_check(nm_ctx* ctx, int wait);
int nm_clear_error(nm_ctx* ctx);

/* ---- in-library stage timing ----------------------------------------------------------------------
 * between nm_profile_begin and nm_profile_end every nm_scale_features call brackets its stages with
 * HIP events on the caller's stream.  nm_profile_end synchronises on them and returns the summed
 * device time in milliseconds: ms[0] cell keys + radix sort, ms[1] occupancy index build,
 * ms[2] the fused search/feature kernel(s), ms[3] reserved; *launches = search-kernel launches timed.
 * used by bench.py for the roofline figure; no reference counterpart (the reference's verbose mode
 * prints wall time per scale, multiscale.py:47-65).                                                */
int nm_profile_begin(nm_ctx* ctx);
/* kept for ABI compatibility; no effect since ABI 5: one launch builds all indexes of a ladder before the
 * first search kernel, there is nothing left to overlap (round 1 measured 2 % for the overlapped form).  */
int nm_set_overlap(nm_ctx* ctx, int enabled);
int nm_profile_end(nm_ctx* ctx, double* ms, int64_t* launches);

/* ---- cloud bounds -------------------------------------------------------------------------------
 * per-axis min and max of a cloud: the `points.min(0)` / `points.max(0)` of geometry.py:37-38.
 * d_minmax receives 6 doubles {min x,y,z, max x,y,z}.  the host turns them into an nm_lattice.    */
int nm_bounds(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride,
              double* d_minmax, void* stream);

/* ---- spatial order ------------------------------------------------------------------------------
 * the order the ladder entry points work in internally (nm_order.hip), exposed for inspection and
 * tests; no reference counterpart (the reference never reorders a cloud).  rows sorted by the
 * compact Z-order key of their cell of `lat`.  the key keeps 20 bits and is sorted in two radix passes for
 * clouds of up to 2^22 points, 30 bits in three passes beyond (nm_order_plan); a wider key loses its low
 * bits.  d_order[i] = row of the point in sorted slot i, d_sorted_xyz (n,3) = the coordinates in that
 * order, d_keys_sorted (nullable) = the key of every sorted slot.  radix sort of our own: per-tile digit
 * counts + one flat scan + a scatter kernel per pass, no look-back.                                 */
size_t nm_spatial_order_workspace_bytes(int64_t n);
int nm_spatial_order(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride, const nm_lattice* lat,
                     uint32_t* d_order, double* d_sorted_xyz, uint32_t* d_keys_sorted, void* d_work,
                     size_t work_bytes, void* stream);

/* ---- voxelize -----------------------------------------------------------------------------------
 * VoxelFilter.coordinate_to_address + numpy.unique (geometry.py:103-116, 148-150): the sorted
 * distinct 64-bit voxel addresses x + (y << shifts[0]) + (z << shifts[1]) of the cells
 * floor((p - min_corner)/edge) occupied by the cloud.  position in this array is the reference's
 * search-voxel index.  d_addr_out needs room for n entries; *d_count (device int64) receives M.
 * points outside the lattice make the call fail the way _check_in_bounds does (geometry.py:95-97):
 * d_count[1] receives the number of out-of-bounds points (the host raises ValueError when != 0).  */
size_t nm_voxelize_workspace_bytes(int64_t n);
int nm_voxelize(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride, const nm_lattice* lat,
                int64_t* d_addr_out, int64_t* d_count, void* d_work, size_t work_bytes, void* stream);

/* VoxelFilter.coordinate_to_address (geometry.py:103-116) without the unique: one address per point,
 * in point order.  *d_oob (device int64, nullable) receives the number of points whose cell lies
 * outside [0, 2^width) on some axis (they are clamped); the bounds check proper
 * (_check_in_bounds, geometry.py:83-99) is done by the host with nm_bounds.                         */
int nm_coordinate_to_address(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride,
                             const nm_lattice* lat, int64_t* d_addr_out, int64_t* d_oob,
                             void* stream);

/* VoxelFilter.address_to_coordinate (geometry.py:120-138): centre = cell*e + min_corner + e*0.5,
 * evaluated left to right in fp64 without fused multiply-add.  d_xyz_out is (m,3) row-major.       */
int nm_address_to_coordinate(nm_ctx* ctx, const int64_t* d_addr, int64_t m, const nm_lattice* lat,
                             double* d_xyz_out, void* stream);

/* ---- one analysis scale, fused -------------------------------------------------------------------
 * one_scale_single_core (nimrud/minimal/multiscale.py:70-123) in one call:
 *   voxel-filter the search cloud (multiscale.py:76-77), find for every query point all voxel
 *   centres with Euclidean distance <= radius (cKDTree.query_ball_tree, multiscale.py:87-103;
 *   inclusive, ((dx*dx + dy*dy) + dz*dz) <= r*r in fp64), and write per query point
 *     [population, ||q - centroid||, l1/(l1+l2+l3), l2/(l1+l2+l3)]      features.py:21-57
 *   (eigenvalues of the ddof=1 covariance, descending) into d_feat[row*feat_stride + 0..3].
 * rows are in query order.  feat_stride is in doubles (4*S for the (Nq,4S) matrix of
 * process_single_core, with d_feat pre-offset by 4*s for scale s: multiscale.py:56).
 * neighborhoods with fewer than 2 voxels get zero eigen-features, empty ones zero centroid
 * (multiscale.py:4-5).  d_info (device int64[4], nullable) receives {M = number of occupied voxels,
 * number of neighborhoods with population < 2, passes taken by the search kernel, reserved}.
 * the query cloud may be the search cloud, or its leading n_query rows (same pointer and stride,
 * n_query <= n_search): the cloud is then sorted and indexed once.                                  */
size_t nm_scale_workspace_bytes(int64_t n_query, int64_t n_search, const nm_lattice* lat);
int nm_scale_features(nm_ctx* ctx,
                      const double* d_query, int64_t n_query, int64_t query_stride,
                      const double* d_search, int64_t n_search, int64_t search_stride,
                      const nm_lattice* lat, double radius,
                      double* d_feat, int64_t feat_stride, int64_t* d_info,
                      void* d_work, size_t work_bytes, void* stream);

/* ---- the whole scale ladder ---------------------------------------------------------------------------
 * process_single_core (nimrud/minimal/multiscale.py:27-67) in one call: scale i uses lats[i] and
 * radii[i] and writes columns 4i..4i+3 of the (n_query, feat_stride) matrix d_feat, scales in caller
 * order (multiscale.py:37,56).  numerically identical to calling nm_scale_features per scale, but the
 * cloud is sorted only once (by its cell keys at the finest lattice of the ladder; the coordinates
 * are kept in that order) and every scale's occupancy index is built from that spatially coherent
 * stream without a sort.  d_info (nullable) receives 4 int64 per scale as in nm_scale_features.      */
size_t nm_multiscale_workspace_bytes(int64_t n_query, int64_t n_search, const nm_lattice* lats,
                                     int32_t n_scales);
/* consecutive scales with the same radius/edge ratio run in ONE launch of the search kernel (a wave keeps its
 * 64 queries and walks the scales).  on by default; 0 = one launch per scale (same numbers).          */
int nm_set_fuse_scales(nm_ctx* ctx, int enabled);

/* ---- the whole scale ladder, lattices built on the device ----------------------------------------------
 * process_single_core (multiscale.py:27-67) without a single value visiting the host: the search cloud's
 * extrema (a bounds pass, or d_minmax: 6 doubles ON THE DEVICE {min xyz, max xyz}, e.g. the global extrema a
 * multi-GPU job has agreed on) are turned into every scale's lattice by a kernel - VoxelFilter.__init__ /
 * _calculate_shift, geometry.py:37-64, same arithmetic: min_corner = min - e/2, widths =
 * ceil(log2((max_corner - min_corner)/e)) - and all later kernels read the lattices from device memory.
 * nothing in the call waits for the device: it can be queued behind other work.  (it can also be captured in
 * a hipGraph - the library records no event and queries none while its stream is capturing - and a replay is
 * bit-identical to the eager call, on new data in the same buffers too: tools/graph_probe.py.  replay buys
 * nothing measurable - the step is bound by its kernels, not by their launches - and back-to-back replays of
 * the 10 M-point step stalled in that probe, so the product path does not use graphs.)
 * what a host-side VoxelFilter would have raised (geometry.py:59-60 "edge length is too small to address
 * this space"; no extent on an axis; a width outside the device path's [1,30]) is reported asynchronously
 * as NM_ERR_LATTICE through nm_check (see there).  the workspace depends on the point counts only.
 * bit-identical to nm_multiscale_features with the lattices the host would have built.                 */
size_t nm_ladder_workspace_bytes(int64_t n_query, int64_t n_search, int32_t n_scales);
/* the same when the edge lengths are known: scales of EQUAL edge length have one lattice and share one occupancy
 * index (the reference's ladders are one voxel edge with several radii, nimrud/utils/point_clouds.py:29-35), so
 * they need its memory once.  never more than nm_ladder_workspace_bytes.                                   */
size_t nm_ladder_workspace_bytes_for(int64_t n_query, int64_t n_search, const double* edges, int32_t n_scales);
int nm_ladder_features(nm_ctx* ctx,
                       const double* d_query, int64_t n_query, int64_t query_stride,
                       const double* d_search, int64_t n_search, int64_t search_stride,
                       const double* edges, const double* radii, int32_t n_scales,
                       const double* d_minmax,
                       double* d_feat, int64_t feat_stride, int64_t* d_info,
                       void* d_work, size_t work_bytes, void* stream);
int nm_multiscale_features(nm_ctx* ctx,
                           const double* d_query, int64_t n_query, int64_t query_stride,
                           const double* d_search, int64_t n_search, int64_t search_stride,
                           const nm_lattice* lats, const double* radii, int32_t n_scales,
                           double* d_feat, int64_t feat_stride, int64_t* d_info,
                           void* d_work, size_t work_bytes, void* stream);

/* ---- k-nearest-voxel fallback (BASELINE config 4; no reference counterpart) -----------------------------
 * build-defined extension: while k_min > 0, nm_scale_features / nm_multiscale_features re-evaluate every
 * query whose radius neighborhood holds fewer than k_min voxels on the k_min nearest voxel centres within
 * radius_factor * radius (fewer if there are not that many; ties broken by smaller voxel address).
 * column 0 keeps the radius population; centroid distance and eigen-features come from the k-NN set.
 * k_min <= 16.  the reference has nothing of the kind (its only kNN mention is a classifier with a
 * missing import, prototypes/apc.py:1479); parity is pinned by the build's own oracle
 * (oracle.one_scale_knn: cKDTree.query on the same voxel set).                                       */
int nm_set_knn_fallback(nm_ctx* ctx, int k_min, double radius_factor);

/* ---- covariance output (legacy C_MSO, prototypes/mso.py:1555) -----------------
 * while d_cov is not NULL, nm_scale_features / nm_multiscale_features also write, per query row and
 * scale s, the upper triangle [xx, xy, xz, yy, yz, zz] of the ddof=1 covariance of the neighborhood's
 * voxel centres - the matrix features.pca forms with numpy.cov (features.py:43) before it takes its
 * eigenvalues - to d_cov[row * cov_stride + 6*s + 0..5] (nm_scale_features: s = 0), in the cloud's
 * units squared.  neighborhoods with fewer than 2 voxels give zeros; rows re-evaluated by the kNN
 * fallback get the covariance of the kNN set.  pass NULL to switch it off again.  the reference returns
 * only the two normalised eigenvalues (features.py:57); this is an opt-in extra, checked against
 * numpy.cov on the oracle's neighborhoods.                                                          */
int nm_set_covariance_output(nm_ctx* ctx, double* d_cov, int64_t cov_stride);

/* ---- surface normal output (legacy OG_MSO, prototypes/mso.py:1315) -------------
 * while d_normal is not NULL, the same calls also write, per query row and scale s, the unit
 * eigenvector of the SMALLEST eigenvalue of that covariance - the normal of the best-fitting plane - to
 * d_normal[row * normal_stride + 3*s + 0..2].  the sign is fixed by making the last non-zero component
 * in the order x, y, z positive (normals point up).  zeros for neighborhoods with fewer than 3 voxels;
 * where the two smallest eigenvalues (nearly) coincide the direction is not defined by the data and
 * the vector is some unit vector of that eigenspace.  opt-in extra, checked against numpy.linalg.eigh
 * on the oracle's neighborhoods.  pass NULL to switch it off.                                        */
int nm_set_normal_output(nm_ctx* ctx, double* d_normal, int64_t normal_stride);

/* ---- neighbor lists (parity / inspection mode) -----------------------------------------------------
 * the neighbor_idx lists of multiscale.py:103 as CSR.  two calls: with d_nbr_index == NULL the
 * per-query counts are written to d_nbr_count (int32[n_query]); the caller turns them into offsets
 * (exclusive prefix sum, int64[n_query+1]) and calls again with d_nbr_offsets and d_nbr_index
 * (int64[total]).  indices are positions in the sorted unique address array d_addr (from
 * nm_voxelize), ascending within a query point.                                                     */
int nm_scale_neighbors(nm_ctx* ctx,
                       const double* d_query, int64_t n_query, int64_t query_stride,
                       const int64_t* d_addr, int64_t m, const nm_lattice* lat, double radius,
                       int32_t* d_nbr_count, const int64_t* d_nbr_offsets, int64_t* d_nbr_index,
                       void* stream);

/* ---- neighbor lists from the occupancy index (voxel ranks, no address search) ----------------------------
 * the same lists - positions in np.unique of the search cloud's addresses (geometry.py:148-150), the
 * indices multiscale.py:103 hands to features.take - from an index that is built ONCE per (search cloud,
 * lattice) and queried for any number of query clouds and radii.  the workspace holds a dense occupancy
 * index of the lattice (a 256-byte leaf of 64 row-words per 32x8x8 superblock) and a rank table: per
 * row-word, the number of occupied cells with a smaller address.  a row-word is 32 consecutive addresses, so
 * a voxel's np.unique position is rank[word] + popcount(word below its bit): no sort, no address array, no
 * search, and every list comes out ascending.
 *   range: lattices with at most 2^21 superblocks, i.e. max(w0-5,0) + max(w1-3,0) + max(w2-3,0) <= 21 for
 *     the widths w; nm_neighbor_index_workspace_bytes returns 0 and the other entry points NM_ERR_LATTICE
 *     beyond it (nm_voxelize + nm_scale_neighbors serve every lattice).  the workspace is a function of the
 *     lattice alone (up to 1.5 GB at the limit) and belongs to the caller for as long as it is queried.
 *   a workspace built for one lattice must be queried with THAT lattice (same corner, edge and widths).
 *   nm_neighbor_index_build: d_count (device int64[2]) receives {M = occupied voxels, search points outside
 *     the lattice}; those points are counted, not indexed (the contract of nm_voxelize's d_count[1]).
 *     n_search == 0 is NM_OK: M = 0 and every list is empty.
 *   nm_neighbor_index_addresses: the sorted distinct addresses (what nm_voxelize writes), every occupied cell
 *     stored at its rank; d_addr_out needs room for min(n_search, cells of the lattice) entries.
 *   nm_neighbor_index_lists: the two calls of nm_scale_neighbors (counts, then indices at d_nbr_offsets[q]),
 *     same home cell, same candidate window, same fp64 test ((dx*dx + dy*dy) + dz*dz) <= r*r, bit for bit.
 *     n_query == 0 is NM_OK.
 * nothing here waits for the device; all of it is queued on `stream`.                                  */
size_t nm_neighbor_index_workspace_bytes(int64_t n_search, const nm_lattice* lat);
int nm_neighbor_index_build(nm_ctx* ctx, const double* d_search, int64_t n_search, int64_t search_stride,
                            const nm_lattice* lat, int64_t* d_count, void* d_work, size_t work_bytes,
                            void* stream);
int nm_neighbor_index_addresses(nm_ctx* ctx, const nm_lattice* lat, const void* d_work, size_t work_bytes,
                                int64_t* d_addr_out, void* stream);
int nm_neighbor_index_lists(nm_ctx* ctx, const double* d_query, int64_t n_query, int64_t query_stride,
                            const nm_lattice* lat, double radius, const void* d_work, size_t work_bytes,
                            int32_t* d_nbr_count, const int64_t* d_nbr_offsets, int64_t* d_nbr_index,
                            void* stream);

/* ---- attributes on the neighbor index (new symbols only: additive within ABI 7) -----------------------------
 * the lists name voxels; these carry per-point attributes onto those voxels and reduce them per neighborhood
 * without writing a list.  exact arithmetic order throughout, so results are reproducible bit for bit.
 *   nm_neighbor_index_voxel_of: per point the position of its voxel in nm_neighbor_index_addresses (the cell by
 *     the same fp64 subtract / divide / floor as the build), or -1 where the point lies outside the lattice on
 *     any axis or in a cell no search point occupies.  for the search cloud the index was built from this is
 *     np.unique(addresses, return_inverse=True)[1].
 *   nm_neighbor_index_group: from such voxel numbers (d_voxel[n], values in [0, m) or -1), d_counts[m] = rows
 *     per voxel (np.bincount), d_start[m+1] = their exclusive prefix sum, d_rows[n] = the rows voxel by voxel,
 *     ASCENDING within a voxel: np.argsort(d_voxel, kind="stable") once rows of no voxel (-1, or >= m) are
 *     left out - they are in no segment, and only the first d_start[m] entries of d_rows are written.  the
 *     result is the same on every run.  d_tmp: nm_neighbor_index_group_workspace_bytes(n) bytes for m <= n,
 *     (..)(m) bytes otherwise (16-byte aligned); n, m < 2^31.
 *   nm_neighbor_index_voxel_reduce: d_out[v * dims + c] = the reduction `op` of d_attr[row * attr_stride + c]
 *     over the rows of voxel v.  NM_REDUCE_SUM adds them left to right in ascending row order starting from 0
 *     (np.bincount(inverse, weights=column)), NM_REDUCE_MEAN divides that sum once by the count (an IEEE
 *     division), NM_REDUCE_MIN / MAX are the plain minimum / maximum.  a voxel without rows gives 0.
 *   nm_neighbor_index_stats: per query point, over the voxels nm_neighbor_index_lists would list (same walk,
 *     same test) and the rows d_values[voxel * value_stride + 0..dims) of a voxel table: d_count[q] = how many,
 *     d_mean[q * out_stride + c] = their sum, added left to right in ascending voxel order, divided once by
 *     the count, d_min / d_max the minimum / maximum.  a query point with no voxel in reach gets count 0 and
 *     zeros in all three tables.  any of the four outputs may be NULL, not all of them.
 *   1 <= dims <= NM_STATS_MAX_DIMS, strides in doubles and at least dims.  NaN attribute values are not
 *   supported (like NaN coordinates): which of them a minimum or maximum keeps is unspecified.
 *   errors: NM_ERR_INVALID for bad arguments, NM_ERR_WORKSPACE for too small a workspace, NM_ERR_RADIUS as
 *   nm_neighbor_index_lists, NM_ERR_LATTICE as every entry point that takes the index.                       */
#define NM_STATS_MAX_DIMS 16
enum { NM_REDUCE_MEAN = 0, NM_REDUCE_SUM = 1, NM_REDUCE_MIN = 2, NM_REDUCE_MAX = 3 };
int nm_neighbor_index_voxel_of(nm_ctx* ctx, const double* d_points, int64_t n, int64_t stride,
                               const nm_lattice* lat, const void* d_work, size_t work_bytes, int64_t* d_voxel,
                               void* stream);
size_t nm_neighbor_index_group_workspace_bytes(int64_t n_points);
int nm_neighbor_index_group(nm_ctx* ctx, const int64_t* d_voxel, int64_t n, int64_t m, int64_t* d_counts,
                            int64_t* d_start, int64_t* d_rows, void* d_tmp, size_t tmp_bytes, void* stream);
int nm_neighbor_index_voxel_reduce(nm_ctx* ctx, const int64_t* d_start, const int64_t* d_rows, int64_t m,
                                   const double* d_attr, int64_t attr_stride, int32_t dims, int32_t op,
                                   double* d_out, void* stream);
int nm_neighbor_index_stats(nm_ctx* ctx, const double* d_query, int64_t n_query, int64_t query_stride,
                            const nm_lattice* lat, double radius, const void* d_work, size_t work_bytes,
                            const double* d_values, int64_t value_stride, int32_t dims, int32_t* d_count,
                            double* d_mean, double* d_min, double* d_max, int64_t out_stride, void* stream);

/* ---- the k nearest voxels on the neighbor index (new symbols only: additive within ABI 7) ---------------------
 * what cKDTree(search_voxels).query(points, k, distance_upper_bound) gave (the tree of multiscale.py:87), read
 * off the index: no tree, nothing sorted.
 *   candidates: for a query point all M occupied voxels of the lattice.  a voxel's squared distance is formed as
 *     nm_neighbor_index_lists forms it: the centre (cell * e + min_corner) + e * 0.5, then
 *     ((dx*dx + dy*dy) + dz*dz) in fp64, nothing fused.
 *   order: by (d2, voxel index) ascending; the voxel index is the position in nm_neighbor_index_addresses, so
 *     equal squared distances are broken by the smaller address.  (scipy leaves ties unspecified.)
 *   limit: a voxel qualifies when d2 <= fl(max_distance * max_distance) - inclusive, like the lists (scipy's
 *     distance_upper_bound is exclusive).  INFINITY: no limit.
 *   output: row q has k slots, d_dist2[q * out_stride + j] and d_index[q * out_stride + j]: the first
 *     min(k, qualifying) voxels in that order, then d2 = +infinity and index = -1 (scipy: M) in the unused
 *     slots; columns from k on are not touched.  d_found[q] (may be NULL) = the number of real slots.  either
 *     of d_dist2 / d_index may be NULL, not both.
 *   query points may lie anywhere, outside the lattice too; NaN coordinates are not supported.  the result is a
 *     function of (index, query point, k, max_distance) alone - not of the launch, of the stage that answered,
 *     or of the other queries - and the same bit for bit on every run; rows are in the caller's order.
 *   d_tmp: nm_neighbor_index_nearest_workspace_bytes(n_query) bytes of scratch (the queries the first stage
 *     hands to the second); n_query < 2^31.  not needed for n_query == 0, which is NM_OK and does nothing.
 *   errors, all before anything is queued: NM_ERR_INVALID for k outside [1, NM_NEAREST_MAX_K], out_stride < k,
 *     a negative or NaN max_distance, bad pointers, too small a d_tmp; NM_ERR_RADIUS for a finite max_distance
 *     beyond the ratio nm_neighbor_index_lists accepts; NM_ERR_WORKSPACE / NM_ERR_LATTICE as every entry point
 *     that takes the index.                                                                                  */
#define NM_NEAREST_MAX_K 32
size_t nm_neighbor_index_nearest_workspace_bytes(int64_t n_query);
int nm_neighbor_index_nearest(nm_ctx* ctx, const double* d_query, int64_t n_query, int64_t query_stride,
                              const nm_lattice* lat, int32_t k, double max_distance, const void* d_work,
                              size_t work_bytes, double* d_dist2, int64_t* d_index, int64_t out_stride,
                              int32_t* d_found, void* d_tmp, size_t tmp_bytes, void* stream);

/* ---- connected components of the voxel graph on the neighbor index (new symbols only: additive within ABI 7) --
 * Euclidean cluster extraction: "the voxels that can be reached from here in steps of at most `radius`".  no edge
 * list is written; every voxel walks the forward half of its window once and joins what it finds in a lock-free
 * union-find (no lane ever waits for another).
 *   vertices: the M occupied voxels, named by their position in nm_neighbor_index_addresses.
 *   edges: u ~ v iff nm_neighbor_index_lists, asked with the voxel centres as queries, names v for u (or u for v):
 *     same home cell, window, row skip and test ((dx*dx + dy*dy) + dz*dz) <= r*r, inclusive.
 *   d_class (int64[M], may be NULL = one class): a negative class takes the voxel out of the graph; an edge joins
 *     voxels of EQUAL class only, so every class is segmented by the one call.
 *   d_weight (int64[M], may be NULL = 1 each): a component's size is the sum of its weights (e.g. points per voxel).
 *   min_size: components of a smaller size are dropped.
 *   output: d_label[M] = the component of every voxel, -1 for voxels outside the graph and for dropped components;
 *     d_size[c] = the size of component c (room for M entries); d_count (int64[2]) = {C = components kept,
 *     components before min_size}.  kept components are numbered 0..C-1 in ascending order of their smallest voxel
 *     position.  sizes are integer sums: the result is a function of the arguments alone, bit for bit on every run.
 *   d_tmp: nm_neighbor_index_components_workspace_bytes(M) bytes (16-byte aligned); the query needs no GPU, is
 *     monotone in M and 0 for M < 0 or M >= 2^31.  M itself is known on the device only: a d_tmp that takes the
 *     minimum (the query at 0) but not this index's M labels nothing and sets d_count to {-1, -1}.
 *   errors, all before anything is queued: NM_ERR_INVALID for a null output or lattice, NM_ERR_RADIUS for a NaN or
 *     negative radius and as nm_neighbor_index_lists, NM_ERR_WORKSPACE for too small a d_work or a d_tmp below the
 *     minimum, NM_ERR_LATTICE as every entry point that takes the index.  nothing here waits for the device.      */
size_t nm_neighbor_index_components_workspace_bytes(int64_t n_voxels);
int nm_neighbor_index_components(nm_ctx* ctx, const nm_lattice* lat, double radius, const void* d_work,
                                 size_t work_bytes, const int64_t* d_class, const int64_t* d_weight,
                                 int64_t min_size, int64_t* d_label, int64_t* d_size, int64_t* d_count,
                                 void* d_tmp, size_t tmp_bytes, void* stream);

/* ---- density-based clusters (DBSCAN) of the voxel graph (new symbols only: additive within ABI 7) -------------
 * the graph of nm_neighbor_index_components, but a voxel links only where the cloud is dense, so one chain of
 * stray voxels no longer welds two objects into one.  no list is written and nothing is sorted.
 *   graph: as nm_neighbor_index_components - u ~ v iff the lists name one for the other and both carry the same
 *     class >= 0; a voxel of negative class is out of the graph: label -1, core 0, density 0.
 *   density[v] = the sum of d_weight over v itself and its neighbors (an int64 sum; d_weight NULL = 1 each, so the
 *     density counts voxels).  weights are integers >= 0; negative weights are unsupported and unchecked.
 *   core[v] = density[v] >= min_weight (sklearn's min_samples with sample_weight, the point itself included).
 *   clusters: the connected components of the graph restricted to core voxels.
 *   border: a voxel of the graph that is not core and has a core neighbor joins the cluster of its NEAREST core
 *     neighbor, ordered by (d2 as the lists' test forms it, voxel position): equal distances go to the smaller
 *     position.  a voxel of the graph that is not core and has no core neighbor is noise: label -1.
 *   a cluster's size is the sum of the weights of all its members, core and border; clusters below min_size are
 *     dropped and their members get -1 (d_core is not changed by that).  kept clusters are numbered 0..C-1 in
 *     ascending order of their smallest CORE voxel position.  with d_weight NULL and min_weight <= 1 every voxel of
 *     the graph is core, and labels, sizes and counts are those of nm_neighbor_index_components.
 *   output: d_label[M], d_size (room for M entries), d_core[M] (0 / 1), d_density[M] (may be NULL: not wanted),
 *     d_count (int64[3]) = {C = clusters kept, clusters before min_size, core voxels}.  all of it is a function of
 *     the arguments alone, the same bit for bit on every run.
 *   d_tmp: nm_neighbor_index_dbscan_workspace_bytes(M) bytes (16-byte aligned): the components scratch and 8 bytes
 *     per voxel more; the query needs no GPU, is monotone in M and 0 for M < 0 or M >= 2^31.  a d_tmp that takes
 *     the minimum (the query at 0) but not this index's M labels nothing and sets d_count to {-1, -1, -1}.
 *   errors, all before anything is queued: NM_ERR_INVALID for a null output or lattice and for a NaN or negative
 *     radius, NM_ERR_RADIUS as nm_neighbor_index_lists, NM_ERR_WORKSPACE for too small a d_work or a d_tmp below
 *     the minimum, NM_ERR_LATTICE as every entry point that takes the index.  nothing here waits for the device. */
size_t nm_neighbor_index_dbscan_workspace_bytes(int64_t n_voxels);
int nm_neighbor_index_dbscan(nm_ctx* ctx, const nm_lattice* lat, double radius, int64_t min_weight,
                             const void* d_work, size_t work_bytes, const int64_t* d_class, const int64_t* d_weight,
                             int64_t min_size, int64_t* d_label, int64_t* d_size, uint8_t* d_core,
                             int64_t* d_density, int64_t* d_count, void* d_tmp, size_t tmp_bytes, void* stream);

/* ---- smoothness-constrained regions of the voxel graph (new symbols only: additive within ABI 7) ---------------
 * region growing stated as connected components: the graph of nm_neighbor_index_components, where two voxels link
 * only when their normals and, optionally, a row of per-voxel values agree - so a roof and the wall below it, a
 * kerb and the road come out as regions of their own.  no list is written, nothing is sorted, no seed order.
 *   graph: as nm_neighbor_index_components - u ~ v iff the lists name one for the other and both carry the same
 *     class >= 0; a voxel of negative class is out of the graph: label -1.
 *   seeds: d_seed[v] != 0 makes a voxel of the graph a seed; d_seed NULL makes every voxel of the graph one.  only
 *     seeds link (the caller-supplied analogue of DBSCAN's core).
 *   link rule: a graph edge between two seeds u, v links them iff both of
 *     d_normal given:  fabs((nu.x*nv.x + nu.y*nv.y) + nu.z*nv.z) >= min_cos, unfused, in this order, on the rows
 *       d_normal + v*normal_stride (doubles).  normals are unsigned directions: a sign flip across a wall does not
 *       cut it.  normals are not normalised here.  the test is false for NaN: a NaN normal links nothing, a zero
 *       normal links only where min_cos <= 0.
 *     d_value given (dims > 0):  fabs(value_u[c] - value_v[c]) <= max_step[c] for every c < dims, on the rows
 *       d_value + v*value_stride.  the limit is inclusive; NaN is false.  max_step is HOST memory, dims entries.
 *     hold.  both tests are symmetric in (u, v) bit for bit - the products commute, fl(a - b) = -fl(b - a) - so
 *     testing each edge once, from its smaller end, is the contract and not an approximation of it.
 *   regions: the connected components of the seeds under the linked edges.  a voxel of the graph that is not a seed
 *     joins the region of its NEAREST seed neighbor of its class, ordered by (d2 as the lists' test forms it, voxel
 *     position) - DBSCAN's border rule; the link rule is not asked there, which is what puts the voxels of a crease
 *     back onto a face.  without a seed neighbor it gets -1.
 *   a region's size is the sum of d_weight (NULL = 1 each) over its members, seeds and attached voxels; regions
 *     below min_size are dropped and their members get -1.  kept regions are numbered 0..C-1 in ascending order of
 *     their smallest SEED position.
 *   identities: with d_seed, d_normal NULL and dims 0, labels, sizes and d_count[0..1] are those of
 *     nm_neighbor_index_components; with d_seed a nm_neighbor_index_dbscan call's d_core and no rule, labels and
 *     sizes are those of that call.
 *   output: d_label[M], d_size (room for M entries), d_count (int64[3]) = {C = regions kept, regions before
 *     min_size, seeds in the graph}.  all of it is a function of the arguments alone, the same bit for bit on every
 *     run.
 *   d_tmp: nm_neighbor_index_regions_workspace_bytes(M) bytes (16-byte aligned), the size of the dbscan scratch;
 *     the query needs no GPU, is monotone in M and 0 for M < 0 or M >= 2^31.  a d_tmp that takes the minimum (the
 *     query at 0) but not this index's M labels nothing and sets d_count to {-1, -1, -1}.
 *   errors, all before anything is queued: NM_ERR_INVALID for a null output or lattice, a NaN or negative radius,
 *     dims outside [0, NM_REGION_MAX_DIMS], dims > 0 without d_value or max_step or with value_stride < dims, a
 *     NaN or negative max_step[c], and with d_normal given a normal_stride < 3 or a NaN min_cos; NM_ERR_RADIUS as
 *     nm_neighbor_index_lists, NM_ERR_WORKSPACE for too small a d_work or a d_tmp below the minimum, NM_ERR_LATTICE
 *     as every entry point that takes the index.  nothing here waits for the device. */
#define NM_REGION_MAX_DIMS 4
size_t nm_neighbor_index_regions_workspace_bytes(int64_t n_voxels);
int nm_neighbor_index_regions(nm_ctx* ctx, const nm_lattice* lat, double radius, const void* d_work,
                              size_t work_bytes, const int64_t* d_class, const int64_t* d_weight,
                              const uint8_t* d_seed, const double* d_normal, int64_t normal_stride, double min_cos,
                              const double* d_value, int64_t value_stride, int32_t dims, const double* max_step,
                              int64_t min_size, int64_t* d_label, int64_t* d_size, int64_t* d_count, void* d_tmp,
                              size_t tmp_bytes, void* stream);

/* ---- peak-seeking segments of the voxel graph: hill climbing (new symbols only: additive within ABI 7) ---------
 * components, dbscan and regions are connectivity rules: two objects of one kind that touch - interlocking tree
 * crowns, cars parked bumper to bumper, two density modes joined by a thick bridge - come out as one.  here every
 * voxel takes ONE uphill link, to a neighbor with a higher value, and a segment is everything that climbs to the same
 * peak: crown delineation with height as the value, quick shift with a density as the value and NM_CLIMB_NEAREST.
 * no list is written, nothing is sorted, no atomics in the link step: every voxel writes its own link only.
 *   graph: as nm_neighbor_index_components - u ~ v iff the lists, asked with the voxel centres as queries, name one
 *     for the other (((dx*dx + dy*dy) + dz*dz) <= r*r, inclusive; a voxel is its own neighbor at d2 = 0) and both
 *     carry the same class.  a voxel v is IN THE GRAPH iff its class is >= 0 (d_class NULL = class 0 for all) and
 *     d_value[v] is not NaN; a voxel outside the graph gets label -1 and link -1 and is nobody's candidate.
 *   d_value (fp64[M], contiguous): the height every voxel climbs on.  +-inf are values like any other.
 *   higher(u, v) := value[u] > value[v] || (value[u] == value[v] && u < v), u and v voxel positions.  on the voxels
 *     of the graph this is a strict total order: equal values (-0 == +0) are ordered by the SMALLER position, and
 *     higher(v, v) is false.  every comparison is false for NaN.
 *   candidates: for v in the graph, a neighbor u is a candidate iff class[u] == class[v], value[u] is not NaN and
 *     higher(u, v).  link[v] is chosen among the candidates, d2 being the squared distance of the two centres as the
 *     lists' test forms it, ((dx*dx + dy*dy) + dz*dz) with d = centre(v) - centre(u), unfused:
 *       NM_CLIMB_HIGHEST (steepest ascent): the largest value[u]; among equal values the smaller d2; among equal d2
 *         the smaller position.
 *       NM_CLIMB_NEAREST (quick shift): the smallest d2; among equal d2 the larger value[u]; then the smaller
 *         position.
 *     a voxel of the graph without a candidate is a PEAK: link[v] = v.  links strictly ascend in a strict total
 *     order, so they form a forest whose roots are the peaks: no cycle, whatever the values.
 *   segments: v belongs to the peak its links lead to.  a plateau of equal values climbs towards its smallest
 *     position as far as the radius lets it: a plateau that is not convex at that radius may split into several
 *     peaks.  every segment lies inside one component of nm_neighbor_index_components of the same radius and
 *     classes.  a strictly increasing map of the values that keeps equal values equal changes nothing.
 *   d_weight (int64[M], may be NULL = 1 each): a segment's size is the sum of the weights of its members, the peak
 *     included; segments below min_size are dropped and their members get -1.  kept segments are numbered 0..C-1
 *     in ascending order of their PEAK's position.
 *   output: d_label[M]; d_size (room for M entries), d_size[c] the size of segment c; d_peak (room for M entries),
 *     d_peak[c] the position of segment c's peak, ascending; d_link[M] (may be NULL: not wanted) the uphill link
 *     of every voxel, the voxel itself at a peak, -1 outside the graph - written before anything is merged, so it
 *     does not depend on d_weight or min_size; d_count (int64[2]) = {C = segments kept, peaks before min_size}.
 *     entries of d_size and d_peak from C on are not touched.  all of it is a function of the arguments alone,
 *     the same bit for bit on every run.
 *   d_tmp: nm_neighbor_index_hill_climb_workspace_bytes(M) bytes (16-byte aligned), the size of the components
 *     scratch; the query needs no GPU, is monotone in M and 0 for M < 0 or M >= 2^31.  a d_tmp that takes the
 *     minimum (the query at 0) but not this index's M writes no label, size, peak or link and sets d_count to
 *     {-1, -1}.
 *   cost: one full-window walk per voxel, then the flatten, number and label steps of the components call; the
 *     flatten step follows every voxel's chain of links to its peak, so its time grows with the longest chain.
 *   errors, all before anything is queued: NM_ERR_INVALID for a null d_value, d_label, d_size, d_peak, d_count or
 *     lattice, a mode other than the two, a NaN or negative radius; NM_ERR_RADIUS as nm_neighbor_index_lists,
 *     NM_ERR_WORKSPACE for too small a d_work or a d_tmp below the minimum, NM_ERR_LATTICE as every entry point
 *     that takes the index.  nothing here waits for the device. */
enum { NM_CLIMB_HIGHEST = 0, NM_CLIMB_NEAREST = 1 };
size_t nm_neighbor_index_hill_climb_workspace_bytes(int64_t n_voxels);
int nm_neighbor_index_hill_climb(nm_ctx* ctx, const nm_lattice* lat, double radius, int32_t mode,
                                 const void* d_work, size_t work_bytes, const double* d_value,
                                 const int64_t* d_class, const int64_t* d_weight, int64_t min_size,
                                 int64_t* d_label, int64_t* d_size, int64_t* d_peak, int64_t* d_link,
                                 int64_t* d_count, void* d_tmp, size_t tmp_bytes, void* stream);

/* ---- the adjacency of a labelling of the voxel graph (new symbols only: additive within ABI 7) -------------------
 * which segments touch, over how many voxel edges, and how high the pass between them lies: the region adjacency
 * graph of any labelling of the voxels, taken off the index.  no list of the voxel graph is written.
 *   graph: as nm_neighbor_index_components - voxels u != v are neighbors iff ((dx*dx + dy*dy) + dz*dz) <= r*r on
 *     their centres (inclusive, unfused) and both carry the same class >= 0 (d_class NULL = class 0 for all); with
 *     d_value (fp64[M], may be NULL) a voxel whose value is NaN is out of the graph.
 *   d_label (int64[M]): a negative label is "in no segment"; labels >= 2^31 are not valid (two labels are packed into
 *     a 64-bit key): such voxels are left out and counted in d_count[1].
 *   an edge {u, v} of the graph CROSSES when label[u] and label[v] are both >= 0 and differ.  the result has one row
 *     per unordered pair of labels a < b that at least one crossing edge joins: links = the number of such edges
 *     (every undirected edge once), saddle = the largest min(value[u], value[v]) over them.
 *   three calls, the host reads one count between them (the number of crossing edges is not known before the walk):
 *   1. nm_neighbor_index_adjacency with d_key NULL: every voxel walks the forward half of its window and counts its
 *      records; d_count (int64[2]) = {R = records, labels >= 2^31}; d_count[1] = -1 where d_tmp has no room for the
 *      index's M.  a record is a run of consecutive crossing edges of one voxel towards one label: R <= the number
 *      of crossing edges.
 *   2. the same call, same arguments and the same d_tmp untouched, with d_key (int64[capacity]), d_links
 *      (int64[capacity]) and, iff d_value is given, d_saddle (fp64[capacity]), capacity >= R: record i is
 *      key[i] = (a << 32) | b, links[i], saddle[i].  with capacity < R nothing is written and d_count[0] = -1.
 *   3. the caller orders the keys (any sort of 64-bit integers; the order among equal keys does not matter) and
 *      nm_neighbor_index_adjacency_reduce takes the sorted keys, d_order (int64[R], may be NULL = identity: record
 *      d_order[i] has the key d_key[i]) and the records' links and saddles: d_pair (int64[R][2]), d_links, d_saddle
 *      (room for R entries each, not overlapping the inputs) get one row per run of equal keys, ascending by (a, b);
 *      d_count[0] = E, the rows.  links add up and saddles take the maximum on integers (the saddle through its
 *      order-preserving integer image): the same bit for bit in any order and on every run; -0 and +0 are one number,
 *      of which +0 is written.
 *   d_tmp: nm_neighbor_index_adjacency_workspace_bytes(M, R) bytes serve any of the three calls (M, 0) serves the
 *     first two; the query needs no GPU, is monotone and 0 for counts < 0 or >= 2^31.
 *   errors, all before anything is queued: NM_ERR_INVALID for null d_label / d_count, a NaN or negative radius, record
 *     pointers that do not go together; NM_ERR_RADIUS as nm_neighbor_index_lists, and where room * W^3 / 2 (the most
 *     records the 32-bit scan could have to count) reaches 2^32; NM_ERR_WORKSPACE, NM_ERR_LATTICE as everywhere. */
size_t nm_neighbor_index_adjacency_workspace_bytes(int64_t n_voxels, int64_t n_records);
int nm_neighbor_index_adjacency(nm_ctx* ctx, const nm_lattice* lat, double radius, const void* d_work,
                                size_t work_bytes, const int64_t* d_label, const double* d_value,
                                const int64_t* d_class, int64_t capacity, int64_t* d_key, int64_t* d_links,
                                double* d_saddle, int64_t* d_count, void* d_tmp, size_t tmp_bytes, void* stream);
int nm_neighbor_index_adjacency_reduce(nm_ctx* ctx, int64_t n_records, const int64_t* d_key, const int64_t* d_order,
                                       const int64_t* d_links_in, const double* d_saddle_in, int64_t* d_pair,
                                       int64_t* d_links, double* d_saddle, int64_t* d_count, void* d_tmp,
                                       size_t tmp_bytes, void* stream);

/* merging peaks by prominence (topological persistence) on the rows of the adjacency: HOST code, host pointers, no
 * context and no GPU call - it runs on a machine without a GPU.
 *   n_segments S, peak_value[S] (no NaN); n_rows E, pair[E][2] with 0 <= a < b < S, saddle[E] (no NaN);
 *   min_prominence >= 0, may be +inf.  segment a is HIGHER than b iff peak_value[a] > peak_value[b], or they are
 *   equal and a < b.
 *   the rows are taken by descending saddle, equal saddles by ascending (a, b), through a union-find in which every
 *   segment starts as its own root: ra = find(a), rb = find(b), nothing to do where they are equal; lo the lower of
 *   the two roots, hi the higher; if peak_value[lo] - saddle < min_prominence (fp64, strict) lo is merged under hi
 *   and hi stays the root; otherwise nothing is merged, and if lo has no recorded prominence yet,
 *   prominence[lo] = peak_value[lo] - saddle.
 *   output: root[S], the surviving root of every segment; prominence[S]: of a root what was recorded, +inf if it
 *   never lost; of a merged segment the difference it was merged at.  scratch: E + S int64.
 *   NM_ERR_INVALID for negative counts, null pointers, a NaN or negative min_prominence, a NaN value or saddle, a row
 *   that is no pair a < b of segments; nothing else can fail. */
int nm_merge_by_prominence(int64_t n_segments, const double* peak_value, int64_t n_rows, const int64_t* pair,
                           const double* saddle, double min_prominence, int64_t* scratch, int64_t* root,
                           double* prominence);

/* ---- shortest paths from seeds over the voxel graph: geodesic distance (new symbols only: additive within ABI 7) --
 * how far a voxel is from the nearest seed ALONG the object - through the voxel graph, around gaps and obstacles, where
 * nm_neighbor_index_nearest measures straight through them - and which seed that is: trees from their stems, distance
 * along a wall or a cable, the Voronoi cells of a seed set in the graph metric.  the one query on the index that
 * iterates: a SWEEP is one full-window walk per voxel, and the number of sweeps depends on the data, so there are two
 * entry points and the host reads one count between them.  no list is written, nothing is sorted.
 *   graph: as nm_neighbor_index_components - u ~ v iff the lists, asked with the voxel centres as queries, name one
 *     for the other (((dx*dx + dy*dy) + dz*dz) <= r*r, inclusive) and both carry the same class >= 0 (d_class NULL =
 *     class 0 for all).  a voxel of negative class is out of the graph: distance +inf, label -1, link -1.
 *   edge length: w(u, v) = sqrt(d2), d2 the squared distance of the two centres exactly as the lists' test forms it,
 *     ((dx*dx + dy*dy) + dz*dz), unfused, and the square root the correctly rounded IEEE one.  w is symmetric in
 *     (u, v) bit for bit, and w > 0: two centres are an edge apart or more, up to the rounding of the centres.
 *   seeds: d_seed (uint8[M]); a voxel of the graph with d_seed[v] != 0 has distance 0.  a seed outside the graph is
 *     ignored.
 *   distance: dist[v] is the least fixpoint of dist[v] = min over neighbors u of fl(dist[u] + w(u, v)), seeds at 0,
 *     everything else starting from +inf.  a candidate fl(dist[u] + w) that exceeds max_distance is not taken (the
 *     limit is inclusive; +inf = no limit), so nothing is reached THROUGH a voxel beyond the limit either.  unreached
 *     voxels keep +inf.  rounded addition is monotone, so relaxing in any order ends at this one fixpoint: the minimum
 *     over all paths from a seed of the path's edge lengths summed left to right from the seed, each sum rounded -
 *     what Dijkstra's algorithm in fp64 returns.  the result is a function of the arguments alone, bit for bit.
 *   lower(u, v) := dist[u] < dist[v] || (dist[u] == dist[v] && u < v), u and v voxel positions: a strict total order
 *     on the reached voxels.  every comparison is false for NaN.
 *   link: for a reached voxel v that is no seed, a neighbor u of its class is a candidate iff
 *     fl(dist[u] + w(u, v)) == dist[v] and lower(u, v).  link[v] is the candidate with the smallest dist[u], among
 *     equal ones the smallest position.  link[v] = v at a seed, -1 where v is unreached or out of the graph.  lower
 *     is part of the test and not inferred from the fixpoint: whatever d_dist holds, links strictly descend a strict
 *     total order and form no cycle.  a reached voxel that is no seed and has no candidate exists only where d_dist is
 *     short of the fixpoint: it gets link -1 and label -1, as does (the label) every voxel whose links lead to it,
 *     and it is counted in d_count[2].
 *   segments: v belongs to the seed its links lead to.  a segment's size is the sum of d_weight (int64[M], NULL = 1
 *     each) over its members, the seed included; segments below min_size are dropped: their labels become -1, dist
 *     and link stay.  kept segments are numbered 0..C-1 in ascending seed position; d_source[c] is that position.
 *   1. nm_neighbor_index_geodesic_relax: first != 0 initialises d_dist (fp64[M]) from d_seed and writes the voxels'
 *      addresses into d_tmp; the call then enqueues `sweeps` >= 1 relaxation sweeps, in place.  d_count (int64[1]) =
 *      the voxels lowered in the LAST sweep of the call: 0 means the fixpoint is reached (and was, before that sweep).
 *      sweeps queued behind one that lowered nothing return at once.  calls with first == 0 continue on the same
 *      d_dist with the same arguments and the same d_tmp, untouched in between.  at most M sweeps lower anything.
 *      d_count[0] = -1, and nothing else is written, where d_tmp has no room for the index's M.
 *   2. nm_neighbor_index_geodesic_finish: the links from d_dist, then segments, sizes and sources.  d_label[M];
 *      d_size, d_source (room for M entries each; entries from C on are not touched); d_link[M] (may be NULL: not
 *      wanted), which does not depend on d_weight or min_size; d_count (int64[3]) = {C = segments kept, seeds in the
 *      graph, voxels without a candidate}, {-1, -1, -1} and nothing else written where d_tmp has no room for the
 *      index's M.  the call stands on its own: any d_tmp of the size serves.
 *   d_tmp: nm_neighbor_index_geodesic_workspace_bytes(M) bytes (16-byte aligned), the size of the components scratch;
 *     the query needs no GPU, is monotone in M and 0 for M < 0 or M >= 2^31.
 *   cost: a sweep is one full-window walk per voxel, like the link step of nm_neighbor_index_hill_climb; the number of
 *     sweeps to the fixpoint is about the largest number of edges on a shortest path.  finish is one such walk and
 *     the flatten, number and label steps of the components call; the flatten follows every voxel's links to its seed.
 *   errors, all before anything is queued: NM_ERR_INVALID for a null d_seed, d_dist, d_count (relax), d_dist, d_label,
 *     d_size, d_source, d_count (finish) or lattice, a NaN or negative radius, a NaN or negative max_distance,
 *     sweeps < 1; NM_ERR_RADIUS as nm_neighbor_index_lists, NM_ERR_WORKSPACE for too small a d_work or a d_tmp below
 *     the minimum, NM_ERR_LATTICE as every entry point that takes the index.  nothing here waits for the device. */
size_t nm_neighbor_index_geodesic_workspace_bytes(int64_t n_voxels);
int nm_neighbor_index_geodesic_relax(nm_ctx* ctx, const nm_lattice* lat, double radius, const void* d_work,
                                     size_t work_bytes, const uint8_t* d_seed, const int64_t* d_class,
                                     double max_distance, int32_t first, int32_t sweeps, double* d_dist,
                                     int64_t* d_count, void* d_tmp, size_t tmp_bytes, void* stream);
int nm_neighbor_index_geodesic_finish(nm_ctx* ctx, const nm_lattice* lat, double radius, const void* d_work,
                                      size_t work_bytes, const int64_t* d_class, const int64_t* d_weight,
                                      int64_t min_size, const double* d_dist, int64_t* d_label, int64_t* d_size,
                                      int64_t* d_source, int64_t* d_link, int64_t* d_count, void* d_tmp,
                                      size_t tmp_bytes, void* stream);

/* ---- per-segment descriptors of a labelled cloud (new symbols only: additive within ABI 7) --------------------
 * what a cluster is as an object: how many points, where, its box, its shape and which way it points.  the last
 * stage behind a classifier and nm_neighbor_index_components; the table is a plain fp64 feature matrix.
 *   input: d_xyz rows of `stride` doubles (x, y, z first) - cloud points, or voxel centres with point counts as
 *     weights; d_label[n]: a value in [0, n_segments) names the row's segment, anything else (-1, >= n_segments)
 *     puts the row in no segment; d_weight[n] (may be NULL = 1 each): integers >= 0, frequency weights as
 *     np.cov(..., fweights=).  a row of weight 0 counts for nothing: not for the box, not as a row.  negative weights
 *     and NaN coordinates are unsupported and unchecked.  n, n_segments < 2^31, sum of weights < 2^53.
 *   output: row s of d_table (table_stride >= NM_SEGMENT_COLUMNS doubles apart; columns from 25 on are not touched):
 *       0       n = sum of weights (an integer sum, exact)
 *       1-3     centroid
 *       4-6     bounding box minimum xyz (exact)          7-9   maximum xyz (exact)
 *       10-15   covariance [xx, xy, xz, yy, yz, zz], ddof = 1 (the layout of nm_set_covariance_output)
 *       16-18   its eigenvalues, descending (the solver of the feature kernels, on the matrix scaled to unit trace)
 *       19-21   unit eigenvector of the smallest eigenvalue (the normal); sign as nm_set_normal_output: the last
 *               non-zero of x, y, z positive
 *       22-24   unit eigenvector of the largest eigenvalue (the axis), same construction and sign rule
 *   degenerate segments: no rows, or n == 0: all zeros.  n < 2: covariance, eigenvalues and both vectors zeros.
 *     fewer than 3 rows, or a zero trace: both vectors zeros.  an eigenvalue that is not simple: its vector is some
 *     unit vector of the eigenspace.
 *   arithmetic: n, the row count and the box first (integer sums, minima and maxima: exact in any order).  the pivot
 *     of a segment is its box minimum; d = p - pivot in fp64, S1 = sum of w d, S2 = sum of w d (x) d, then
 *     centroid = pivot + S1 / n and cov = (S2 - S1 S1^T / n) / (n - 1).  no raw moments of p (they lose every digit
 *     on georeferenced coordinates), no floating-point atomics, nothing fused.
 *   order: the summation tree of a segment is a function of its ASCENDING row list alone - not of n, of the other
 *     segments, of where its rows lie in the cloud, of the launch or of the run; results repeat bit for bit.
 *       - the list is cut into consecutive chunks of NM_SEGMENT_CHUNK = 256 rows, counted from the segment's start;
 *       - chunk tree: slot j of 64 adds the terms of rows j, j + 64, j + 128, j + 192 of the chunk left to right;
 *         the slots are then added pairwise, neighbours first: j += j + 1 (j even), j += j + 2 (j % 4 == 0), ...,
 *         j += j + 32.  an absent row is +0;
 *       - segment tree: slot j of 64 adds the chunk sums j, j + 64, j + 128, ... left to right, then the same
 *         pairwise steps.
 *     the term of a row for S1 is w * d, for S2 (w * d_a) * d_b.
 *   work is dealt out by chunks, not by segments: one segment holding every row occupies the device, and segments of
 *     up to 8 rows take eight lanes each.
 *   d_tmp: nm_segment_table_workspace_bytes(n, n_segments) bytes; the query needs no GPU, is monotone in both
 *     arguments and 0 for negative sizes or sizes >= 2^31.
 *   n == 0 with n_segments > 0 zero-fills the table; n_segments == 0 is NM_OK and does nothing.
 *   errors, all before anything is queued: NM_ERR_INVALID for null pointers, negative sizes, sizes >= 2^31,
 *     stride < 3, table_stride < NM_SEGMENT_COLUMNS; NM_ERR_WORKSPACE for too small a d_tmp.  nothing here waits for
 *     the device.                                                                                                */
#define NM_SEGMENT_COLUMNS 25
#define NM_SEGMENT_CHUNK 256
size_t nm_segment_table_workspace_bytes(int64_t n, int64_t n_segments);
int nm_segment_table(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride, const int64_t* d_label,
                     int64_t n_segments, const int64_t* d_weight, double* d_table, int64_t table_stride,
                     void* d_tmp, size_t tmp_bytes, void* stream);

/* ---- explicit neighborhoods -----------------------------------------------------------------------
 * features.population / centroid / pca (features.py:21-57) for a batch of explicit neighborhoods
 * given as CSR over a point array: neighborhood b is d_points[d_offsets[b] .. d_offsets[b+1]) (rows
 * of 3 doubles), d_query row b is its query point.  output as in nm_scale_features.                 */
int nm_neighborhood_features(nm_ctx* ctx, const double* d_points, const int64_t* d_offsets,
                             const double* d_query, int64_t n_neighborhoods,
                             double* d_feat, int64_t feat_stride, void* stream);

/* ---- multi-GPU tiling: halo selection -------------------------------------------------------------
 * no reference counterpart in nimrud/minimal (it is single-process); the legacy partitioners pair a
 * query tile with a search tile grown by the largest scale (prototypes/mso.py:892-927,
 * utils/geometry.py:203-253).  a rank owns one spatial tile; d_boxes holds one axis-aligned box per
 * rank (n_boxes x 6 doubles: lo xyz, hi xyz, already grown by the halo margin), `skip` is the
 * caller's own rank.  nm_halo_count writes, per destination box, how many of the caller's points lie
 * inside it (inclusive); nm_halo_pack writes those points as rows of 3 doubles into d_out, the rows
 * of destination b starting at row d_offsets[b] (order within a destination is unspecified);
 * d_cursor is int64[n_boxes] scratch.  the packed rows are what goes through RCCL's all-to-all.
 * nm_copy_xyz copies the geometry columns of a strided cloud into (n,3) contiguous rows.            */
int nm_halo_count(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride, const double* d_boxes,
                  int32_t n_boxes, int32_t skip, int64_t* d_counts, void* stream);
int nm_halo_pack(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride, const double* d_boxes,
                 int32_t n_boxes, int32_t skip, const int64_t* d_offsets, int64_t* d_cursor,
                 double* d_out, void* stream);
int nm_copy_xyz(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride, double* d_out,
                void* stream);

/* ---- multi-GPU tiling: cell-set halos -----------------------------------------------------------------
 * a Morton-contiguous tile (what BASELINE's north_star shards by) is L-shaped: its bounding box, and with
 * it a box halo, covers far more than the tile.  a tile's CELL SET is the set of cells of a coarse cubic
 * grid occupied by its points, dilated by the margin: NM_HALO_CELLSET_WORDS 32-bit words, one bit per
 * cell, cell index = (z * dim_y + y) * dim_x + x.  the grid is a pure function of the global extrema
 * (d_global_minmax: 6 doubles on the device, identical on every rank) and the margin - cell edge margin/4
 * unless that needs more than 2^21 cells - so every rank computes the same one without talking.
 * nm_halo_cellset writes the caller's own set; nm_halo_count_cells / nm_halo_pack_cells are
 * nm_halo_count / nm_halo_pack with "inside destination r's cell set" (d_cellsets: n_ranks sets back to
 * back, e.g. straight out of an all-gather) in place of the box test.  same idea as the reference's
 * query tile + grown search tile (prototypes/mso.py:892-927), for tiles of any shape.                */
#define NM_HALO_CELLSET_WORDS 65536
size_t nm_halo_cellset_workspace_bytes(void);
int nm_halo_cellset(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride,
                    const double* d_global_minmax, double margin, uint32_t* d_cellset,
                    void* d_work, size_t work_bytes, void* stream);
int nm_halo_count_cells(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride,
                        const double* d_global_minmax, double margin, const uint32_t* d_cellsets,
                        int32_t n_ranks, int32_t skip, int64_t* d_counts, void* stream);
int nm_halo_pack_cells(nm_ctx* ctx, const double* d_xyz, int64_t n, int64_t stride,
                       const double* d_global_minmax, double margin, const uint32_t* d_cellsets,
                       int32_t n_ranks, int32_t skip, const int64_t* d_offsets, int64_t* d_cursor,
                       double* d_out, void* stream);

/* ---- multi-GPU tiling: the halo exchange over RCCL ------------------------------------------------------
 * one process per GPU, one nm_ctx and one RCCL communicator per process.  the communicator is a plain
 * ncclComm_t (passed as void*): create it with nm_comm_create from a 128-byte unique id that rank 0 got
 * from nm_comm_unique_id and handed to the other ranks by any means (the Python host broadcasts it with
 * torch.distributed, which is all it uses torch.distributed for), or pass one the host already owns.
 *
 * nm_halo_exchange is collective over the communicator.  every rank passes its tile (d_xyz: n rows) and
 * the halo margin max_s(radius_s + sqrt(3)/2 edge_s); on return (the sends and receives are enqueued on
 * `stream`) d_recv holds, in rank order, the rows of all other tiles that lie within the margin of this
 * tile - by destination box (NM_HALO_BOXES) or by destination cell set (NM_HALO_CELLS, see above) -
 * *h_recv_rows / *h_sent_rows (HOST) the row counts, and d_global_minmax (device, 6 doubles) the extrema of
 * the WHOLE cloud, from which every rank builds the same lattices as a single-process run
 * (geometry.py:37).  traffic: all-gather of 6 doubles, (cell mode) all-gather of 256 KB, all-gather of
 * n_ranks + 3 int64, then grouped ncclSend / ncclRecv of 24-byte rows between the pairs that share a
 * boundary.  the call synchronises `stream` ONCE, to learn the sizes.  when some rank's buffers are too
 * small EVERY rank returns NM_ERR_WORKSPACE (with its own counts filled in) before anything is sent, so
 * the hosts can grow their buffers and call again.  a tile may be EMPTY (n = 0: it contributes an empty
 * box and receives nothing).  a rank that alone is unwell - a sticky failure of an earlier call, bad cloud
 * arguments - still goes through the collectives, with an empty contribution and its status in the
 * announced row: after the host synchronisation EVERY rank returns that status; nobody waits in an
 * all-gather for a rank that has left.  (nm_halo_plan_from_matrix is that decision as a host function
 * of the gathered matrix - n_ranks rows of n_ranks + 3 int64: rows sent to each rank, send capacity,
 * receive capacity, status - exported so that it can be tested without a communicator.)
 * NM_HALO_REUSE_PLAN (or-ed into mode, by EVERY rank or by none): the tiles have not changed since this
 * context's last full call with the same communicator size, rank, mode, tile size and workspace - boxes, cell
 * sets and the pair counts stand.  the call then packs and exchanges the rows again (the data moves every
 * step) but skips the three all-gathers and the host synchronisation: a step on a static cloud enqueues and
 * returns.  nm_halo_stats counts both kinds of call.  the send staging area is whatever d_work holds beyond
 * nm_halo_workspace_bytes(0, n_ranks).  NM_HALO_INCLUDE_SELF (or-ed into mode) makes a rank its own
 * neighbour as well - it then receives its own tile - which is how a one-rank communicator exercises the
 * whole path.  no reference counterpart: the reference is single-process.                              */
#define NM_COMM_ID_BYTES 128
enum { NM_HALO_BOXES = 0, NM_HALO_CELLS = 1, NM_HALO_INCLUDE_SELF = 4, NM_HALO_REUSE_PLAN = 8 };
int nm_comm_unique_id(void* id_out /* NM_COMM_ID_BYTES, host */);
int nm_comm_create(nm_ctx* ctx, int32_t n_ranks, int32_t rank, const void* id, void** comm_out);
int nm_comm_destroy(nm_ctx* ctx, void* comm);
size_t nm_halo_workspace_bytes(int64_t send_capacity_rows, int32_t n_ranks);
int nm_halo_stats(nm_ctx* ctx, int64_t* host_syncs, int64_t* exchanges);
int nm_halo_plan_from_matrix(const int64_t* matrix, int32_t n_ranks, int32_t rank, int64_t* send_off,
                             int64_t* recv_off, int64_t* sent_rows, int64_t* recv_rows, int32_t* culprit);
int nm_halo_exchange(nm_ctx* ctx, void* nccl_comm, int32_t n_ranks, int32_t rank,
                     const double* d_xyz, int64_t n, int64_t stride, double margin, int32_t mode,
                     double* d_recv, int64_t recv_capacity_rows,
                     int64_t* h_recv_rows, int64_t* h_sent_rows, double* d_global_minmax,
                     void* d_work, size_t work_bytes, void* stream);

/* ---- derived descriptors ------------------------------------------------
 * linearity (l1-l2)/l1, planarity (l2-l3)/l1 and scatter l3/l1 per scale, from the normalised
 * eigenvalues of a feature matrix produced by nm_(multi)scale_features (l3 = 1 - l1 - l2).  the
 * reference's minimal path stops at (l1, l2) (features.py:57); its legacy generation carries full
 * covariance / eigenvector variants (prototypes/mso.py:1315,1555).  d_out is (n, out_stride) with 3
 * columns per scale; undefined rows give zeros.                                                    */
int nm_descriptors(nm_ctx* ctx, const double* d_feat, int64_t n, int32_t n_scales, int64_t feat_stride,
                   double* d_out, int64_t out_stride, void* stream);

/* ---- vector-field operator (legacy V_MSO, prototypes/mso.py:12-173) ----------
 * neighborhood mean of arbitrary per-point attributes on the lattice of nimrud/minimal: the search cloud
 * is voxel-filtered as for the features (geometry.py:103-154); a voxel's attribute vector is the mean of
 * d_attr[row*attr_stride + 0..dims) over the search points in it; query row q receives, in
 * d_out[q*out_stride + 0..dims), the mean of the voxel attributes over the voxel centres within
 * `radius` (inclusive, the predicate of multiscale.py:87-103), zeros if there are none.  1 <= dims <= 16.
 * one scale per call.  the legacy operator (fp32, partition dependent) cannot be reproduced number for
 * number and the reference's current path has none: parity is pinned by the build's own oracle.      */
size_t nm_field_workspace_bytes(int64_t n_query, int64_t n_search, const nm_lattice* lat, int32_t dims);
int nm_field_mean(nm_ctx* ctx,
                  const double* d_query, int64_t n_query, int64_t query_stride,
                  const double* d_search, int64_t n_search, int64_t search_stride,
                  const double* d_attr, int64_t attr_stride, int32_t dims,
                  const nm_lattice* lat, double radius,
                  double* d_out, int64_t out_stride, void* d_work, size_t work_bytes, void* stream);

/* ---- classifier slot -------------------------------------------------------------------------------
 * nimrud/minimal/classification.py is a stub; the reference's classifier is sklearn's
 * RandomForestClassifier (prototypes/apc.py:1463) applied per point with predict / predict_proba
 * (apc.py:1022,1034).  the forest is passed flattened: node arrays of all trees concatenated,
 * children are absolute node indices (-1 at a leaf), `value` is the per-node class distribution
 * normalised to sum 1, `roots` the root node of each tree.  features are cast to fp32 and a sample
 * goes left when (double)(float)x[feature] <= threshold, as sklearn does.
 * d_proba (n, n_classes) row-major (nullable), d_label int32[n] = argmax class position (nullable). */
typedef struct nm_forest {
    const int32_t* d_left;
    const int32_t* d_right;
    const int32_t* d_feature;
    const double*  d_threshold;
    const double*  d_value;
    const int32_t* d_roots;
    int32_t n_nodes;
    int32_t n_trees;
    int32_t n_classes;
    int32_t n_features;
    /* optional fast layout (both or neither): nodes renumbered so that the right child of node i is
     * left(i) + 1, one 16-byte record per node {double threshold; int32 left; int32 feature}; a leaf has
     * left = -1 and feature = its row in d_leaf_value (n_leaves x n_classes, rows sum to 1).
     * d_packed_roots holds the root record of each tree.  with these set (and n_features <= 40) one
     * record load replaces four array loads per node visit.                                         */
    const void*    d_packed;
    const double*  d_leaf_value;
    const int32_t* d_packed_roots;
    int32_t n_leaves;
    /* doubles from one row of d_leaf_value to the next; 0 = n_classes (rows packed).  with rows of 8 doubles,
     * 64-byte aligned and zero-padded behind n_classes (what ForestModel builds for up to 8 classes), a lane's
     * leaf distribution is one cache line fetched with 16-byte loads: the gather of the distributions - 39 % of
     * the forest stage of config 5 with packed rows of 40 bytes - costs half                                    */
    int32_t leaf_stride;
    /* optional compact layout of the same renumbered nodes (needs d_leaf_value and d_packed_roots too, and
     * n_features <= 32): one 8-byte record per node {float threshold; uint32 packed}.  the threshold is the
     * largest fp32 value not above the fp64 threshold - sklearn compares the fp32-cast feature with the fp64
     * threshold, and x_f32 <= t_f64 holds exactly when x_f32 <= that value.  packed: bits 30..13 = the left
     * child's record (so at most 2^18 nodes), bits 12..8 the feature, bits 7..0 zero; a leaf has bit 31 set,
     * its row in d_leaf_value in bits 30..13 and the rest zero.  preferred by nm_forest_eval when present; required by
     * nm_set_forest_output.                                                                             */
    const void*    d_packed8;
} nm_forest;

int nm_forest_eval(nm_ctx* ctx, const nm_forest* forest, const double* d_feat, int64_t n,
                   int64_t feat_stride, double* d_proba, int32_t* d_label, void* stream);

/* the classifier behind the last scale (BASELINE config 5: "random-forest classifier evaluation fused after
 * feature assembly").  while a forest is set, nm_multiscale_features / nm_ladder_features evaluate it on
 * every query row right after the row's last scale, inside the search kernel: the wave that has just written
 * the row reads its 4*S features back while they are still in the XCD's L2, and its 64 lanes - neighbours in
 * space - walk nearly the same paths.  d_proba (n_query, proba_stride) and d_label int32[n_query], rows in
 * query order, either may be NULL; same numbers as nm_forest_eval on the finished matrix (which is what
 * runs instead when the last scale has an unusual radius/edge ratio or the kNN fallback is on).  limits:
 * n_features == 4 * n_scales <= 20, n_classes <= 8, the d_packed8 layout.  context state, like the
 * covariance output; pass forest = NULL to switch it off.  the struct is copied, the arrays must stay
 * alive.                                                                                               */
int nm_set_forest_output(nm_ctx* ctx, const nm_forest* forest, double* d_proba, int64_t proba_stride,
                         int32_t* d_label);
/* where the forest of nm_set_forest_output runs: 1 (default) in the epilogue of the last search kernel; 0 as a
 * launch of its own directly behind the last scale, over the rows in the ladder's spatial order; 2 as a launch of
 * its own over the finished matrix with the trees streamed through LDS (what nm_forest_eval runs).  same
 * numbers.  measured on MI355X, 10 M rows x 32 trees (tools/forest_modes.py): 2.1 ms in the epilogue - the tree
 * walk waits on memory, and there it waits while other waves of the same SIMD run their (vector-ALU bound)
 * search - against 2.5 ms (mode 0) and 3.0 ms (mode 2; 3.5 ms for a row walk from memory in row order). */
int nm_set_forest_mode(nm_ctx* ctx, int in_search_kernel);

#ifdef __cplusplus
}
#endif
#endif /* NIMRUD_HIP_H */
