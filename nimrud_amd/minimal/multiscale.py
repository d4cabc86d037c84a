"""
multiscale operator processing pipeline on the MI355X: the drop-in for nimrud/minimal/multiscale.py.

features are generated for points in the query cloud, using geometry from the search cloud.  for each
scale: voxel-filter the search cloud at `edge_length`, find every occupied voxel centre within
`radius` of each query point, and emit [population, distance to the neighborhood centroid, largest
and middle eigenvalue of the covariance normalised by the eigenvalue sum] (multiscale.py:1-6,70-123).
undefined features (neighborhoods of fewer than two voxels) are zeros, as the reference documents
(multiscale.py:4-5); pass strict=True to get the FloatingPointError the reference actually raises
from numpy.cov in that case.

same names and signatures as the reference:
    process_single_core(query_cloud, search_cloud, edge_lengths, radii, verbose=False)  -> (Nq, 4*S)
    one_scale_single_core(query_cloud, search_cloud, edge_length, radius, verbose=False) -> (Nq, 4)
("single core" is kept for compatibility: the work runs on one GPU.)  additive, for data that already
lives in HBM: process_gpu / one_scale_gpu take and return torch GPU tensors.

each scale is one call into libnimrud_hip.so (nm_scale_features): cell keys -> radix sort -> sparse
occupancy index -> fused search/moments/eigen kernel.  see DESIGN.md.
"""

import ctypes
import math
import time

import numpy as np
import torch

from nimrud_amd import _ffi
from nimrud_amd import device as _device
from nimrud_amd.utils import geometry

# kept for API compatibility with the reference (multiscale.py:18-24).  the GPU path has no kd-tree
# and no host-side chunk loop, so LEAFSIZE and QUERY_CHUNK_SIZE have no effect here.
LEAFSIZE = 300
QUERY_CHUNK_SIZE = 1000
VERBOSITY_INTERVAL = 100


class ScaleInfo(object):
    """what one scale reported: voxels = M (occupied search voxels), degenerate = neighborhoods with
    population < 2, extra_passes = search-kernel passes beyond one per wave, leaves = index leaves."""

    def __init__(self, values):
        self.voxels, self.degenerate, self.extra_passes, self.leaves = (int(v) for v in values)

    def __repr__(self):
        return "ScaleInfo(voxels=%d, degenerate=%d, extra_passes=%d, leaves=%d)" % (
            self.voxels, self.degenerate, self.extra_passes, self.leaves)


def _scale_into(rt, query, search, shared, lo, hi, edge_length, radius, out_view, info_view):
    """enqueue one scale: features of `query` against `search` into out_view (Nq,4 strided)."""
    vf = geometry.VoxelFilter.from_bounds(lo, hi, edge_length, device=rt.device)
    lat = vf.nm_lattice
    nq, ns = query.shape[0], search.shape[0]
    nbytes = rt.lib.nm_scale_workspace_bytes(nq, ns, ctypes.byref(lat))
    work = rt.workspace(nbytes)
    qt = search if shared else query
    rt.check(rt.lib.nm_scale_features(
        rt.ctx, _device.ptr(qt), nq, _device.row_stride(qt),
        _device.ptr(search), ns, _device.row_stride(search),
        ctypes.byref(lat), float(radius),
        _device.ptr(out_view), int(out_view.stride(0)), _device.ptr(info_view),
        _device.ptr(work), work.numel(), rt.stream()))


def _ladder_into(rt, query, search, shared, bounds, edge_lengths, radii, out, info, knn_min=0,
                 knn_radius_factor=3.0):
    """enqueue the whole ladder in one library call (nm_ladder_features): the cloud is sorted once, every
    scale's lattice is built on the device from the search cloud's extrema and every index from that
    order.  nothing visits the host: the call can be queued behind other work.
    bounds: None (the library measures the search cloud) or a (6,) fp64 device tensor {min xyz, max xyz}
    - the global extrema of a multi-GPU job."""
    # the fallback switch is context state in the C ABI: always set it, so no call inherits another's
    rt.check(rt.lib.nm_set_knn_fallback(rt.ctx, int(knn_min), float(knn_radius_factor)))
    n_scales = len(edge_lengths)
    edg = (ctypes.c_double * n_scales)(*[float(e) for e in edge_lengths])
    rad = (ctypes.c_double * n_scales)(*[float(r) for r in radii])
    nq, ns = query.shape[0], search.shape[0]
    nbytes = rt.lib.nm_ladder_workspace_bytes_for(nq, ns, edg, n_scales)     # equal edges share an index
    if nbytes == 0:
        raise ValueError("bad ladder arguments (at most 32 scales per call)")
    work = rt.workspace(nbytes)
    qt = search if shared else query
    if bounds is not None and not (isinstance(bounds, torch.Tensor) and bounds.is_cuda and
                                   bounds.dtype == torch.float64 and bounds.numel() == 6
                                   and bounds.is_contiguous()):
        raise ValueError("bounds must be a contiguous (6,) fp64 tensor on the device")
    rt.check(rt.lib.nm_ladder_features(
        rt.ctx, _device.ptr(qt), nq, _device.row_stride(qt),
        _device.ptr(search), ns, _device.row_stride(search), edg, rad, n_scales,
        _device.ptr(bounds), _device.ptr(out), int(out.stride(0)), _device.ptr(info),
        _device.ptr(work), work.numel(), rt.stream()))


def _report_scale(rt, verbose, nq, info, s, this_edge, this_radius, inner_start):
    """the reference's per-scale progress lines (multiscale.py:47-65)."""
    if not verbose:
        return
    torch.cuda.synchronize(rt.device)
    inner = time.perf_counter() - inner_start
    print("querying {} points against a search space of {} voxels".format(nq, int(info[s, 0])))
    print("using a voxel edge length of {} and radius of {}".format(this_edge, this_radius))
    print("this scale took {}s".format(np.around(inner, 6)))
    print("one scale rate of {} points per second".format(np.around(nq / inner, 3)))
    print("===================================")


def process_gpu(query_cloud, search_cloud, edge_lengths, radii, verbose=False, strict=False,
                return_info=False, out=None, per_scale=False, knn_min=0, knn_radius_factor=3.0,
                cov_out=None, normal_out=None):
    """process_single_core for clouds resident in HBM: torch GPU tensors in, (Nq, 4*S) fp64 GPU tensor
    out.  nothing crosses PCIe, and nothing waits for the device: the lattices are built on the GPU from
    the cloud's extrema (nm_ladder_features), so the call only enqueues work.  what the reference's
    VoxelFilter raises synchronously for an unusable edge length (geometry.py:59-60) therefore surfaces
    at the next synchronisation point: strict / return_info (which read 4 counters per scale back),
    process_single_core, the next call into the library, or `nimrud_amd.device.get_runtime().check_async()`.
    the ladder normally runs as ONE library call that sorts the cloud once for all scales;
    verbose=True or per_scale=True runs one self-contained call per scale instead (same numbers).
    knn_min > 0 switches on the k-nearest-voxel fallback (an extension the reference does not have,
    BASELINE config 4): neighborhoods with fewer than knn_min voxels take their centroid and eigen
    features from the knn_min nearest voxels within knn_radius_factor * radius.
    cov_out, a (Nq, 6*S) fp64 GPU tensor, additionally receives per scale the upper triangle
    [xx, xy, xz, yy, yz, zz] of the neighborhood covariance whose eigenvalues the features are
    (see process_gpu_covariance).  normal_out, (Nq, 3*S), receives the unit
    eigenvector of its smallest eigenvalue - the surface normal, pointing up (process_gpu_normals)."""
    assert len(edge_lengths) == len(radii), \
        "edge_lengths and radii should be equal-length sequences."
    shared = query_cloud is search_cloud
    rt, search = _device.as_cloud(search_cloud)
    query = search if shared else _device.as_cloud(query_cloud, rt.device)[1]
    if search.shape[1] < 3 or query.shape[1] < 3:
        raise ValueError("only 3D spaces supported by the multiscale pipeline")
    if search.shape[0] < 2:
        raise ValueError("need at least 2 points to define a voxel grid")
    n_scales = len(edge_lengths)
    nq = query.shape[0]
    if out is None:
        out = torch.empty((nq, 4 * n_scales), dtype=torch.float64, device=rt.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float64 and out.device == rt.device
              and out.ndim == 2 and out.shape[0] == nq and out.shape[1] >= 4 * n_scales
              and (out.shape[1] == 0 or out.stride(1) == 1)
              and (nq <= 1 or out.stride(0) >= 4 * n_scales)):
        # the kernels write 4*S doubles per row at the row pitch of `out`: anything else would put
        # 8-byte stores outside the allocation
        raise ValueError("out must be a (Nq, >= 4*S) fp64 tensor on the clouds' device with unit column "
                         "stride")
    # the per-scale counters (voxels, degenerate neighborhoods, extra passes, leaves) cost a pass over the
    # index: only when somebody will look at them
    want_info = bool(strict or return_info or verbose)
    info = torch.zeros((max(n_scales, 1), 4), dtype=torch.int64, device=rt.device) if want_info else None
    if n_scales == 0:
        return (out, []) if return_info else out

    if cov_out is not None:
        if not (isinstance(cov_out, torch.Tensor) and cov_out.dtype == torch.float64 and
                cov_out.device == out.device and cov_out.ndim == 2 and cov_out.shape[0] == nq and
                cov_out.shape[1] >= 6 * n_scales and cov_out.stride(1) == 1):
            raise ValueError("cov_out must be a (Nq, >= 6*S) fp64 tensor on the clouds' device")
    if normal_out is not None:
        if not (isinstance(normal_out, torch.Tensor) and normal_out.dtype == torch.float64 and
                normal_out.device == out.device and normal_out.ndim == 2 and normal_out.shape[0] == nq
                and normal_out.shape[1] >= 3 * n_scales and normal_out.stride(1) == 1):
            raise ValueError("normal_out must be a (Nq, >= 3*S) fp64 tensor on the clouds' device")
    outer_start = time.perf_counter()
    rt.check(rt.lib.nm_set_knn_fallback(rt.ctx, int(knn_min), float(knn_radius_factor)))
    lo = hi = None
    if verbose or per_scale:
        lo, hi = _device.cloud_bounds(rt, search)       # the per-scale form builds its lattices here

    def covariance_columns(first_scale):
        # context state of the C ABI, like the fallback switch: set for this call, cleared after it
        if cov_out is not None:
            rt.check(rt.lib.nm_set_covariance_output(
                rt.ctx, ctypes.c_void_p(cov_out.data_ptr() + 48 * first_scale), int(cov_out.stride(0))))
        if normal_out is not None:
            rt.check(rt.lib.nm_set_normal_output(
                rt.ctx, ctypes.c_void_p(normal_out.data_ptr() + 24 * first_scale),
                int(normal_out.stride(0))))

    try:
        if not (verbose or per_scale):
            covariance_columns(0)
            _ladder_into(rt, query, search, shared, None, edge_lengths, radii, out, info,
                         knn_min=knn_min, knn_radius_factor=knn_radius_factor)
            edge_lengths_loop = []
        else:
            edge_lengths_loop = list(zip(edge_lengths, radii))
        for s, (this_edge, this_radius) in enumerate(edge_lengths_loop):
            inner_start = time.perf_counter()
            covariance_columns(s)
            _scale_into(rt, query, search, shared, lo, hi, this_edge, this_radius,
                        out[:, 4 * s:4 * s + 4], info[s] if info is not None else None)
            _report_scale(rt, verbose, nq, info, s, this_edge, this_radius, inner_start)
    finally:
        if cov_out is not None:
            rt.check(rt.lib.nm_set_covariance_output(rt.ctx, None, 0))
        if normal_out is not None:
            rt.check(rt.lib.nm_set_normal_output(rt.ctx, None, 0))
    if verbose:
        torch.cuda.synchronize(rt.device)
        outer = time.perf_counter() - outer_start
        print("calculating all scales took {}s".format(np.around(outer, 6)))
        print("final rate of {} points per second".format(np.around(nq / outer, 3)))

    if strict or return_info:
        host = info.cpu().numpy()
        rt.check_async(wait=True)        # an unusable lattice, an index that timed out or overflowed
        if strict and host[:n_scales, 1].any():
            raise FloatingPointError(
                "%d neighborhoods have fewer than 2 voxels; their covariance is undefined "
                "(the reference raises here from numpy.cov, features.py:43)"
                % int(host[:n_scales, 1].sum()))
        if return_info:
            return out, [ScaleInfo(row) for row in host[:n_scales]]
    return out


def process_gpu_covariance(query_cloud, search_cloud, edge_lengths, radii, **kwargs):
    """(features (Nq, 4*S), covariances (Nq, 6*S)): per scale the four features and the upper triangle
    [xx, xy, xz, yy, yz, zz] of the ddof=1 covariance of the neighborhood's voxel centres - the matrix
    features.pca builds with numpy.cov (features.py:43).  zeros where fewer than 2 voxels."""
    rt, search = _device.as_cloud(search_cloud)
    nq = search.shape[0] if query_cloud is search_cloud else _device.as_cloud(query_cloud, rt.device)[1].shape[0]
    cov = torch.zeros((nq, 6 * len(edge_lengths)), dtype=torch.float64, device=rt.device)
    feats = process_gpu(query_cloud, search_cloud, edge_lengths, radii, cov_out=cov, **kwargs)
    return feats, cov


def process_gpu_normals(query_cloud, search_cloud, edge_lengths, radii, **kwargs):
    """(features (Nq, 4*S), normals (Nq, 3*S)): per scale the unit eigenvector of the smallest eigenvalue
    of the neighborhood covariance, last non-zero component (x, y, z order) positive; zeros where fewer
    than 3 voxels."""
    rt, search = _device.as_cloud(search_cloud)
    nq = search.shape[0] if query_cloud is search_cloud else _device.as_cloud(query_cloud, rt.device)[1].shape[0]
    normals = torch.zeros((nq, 3 * len(edge_lengths)), dtype=torch.float64, device=rt.device)
    feats = process_gpu(query_cloud, search_cloud, edge_lengths, radii, normal_out=normals, **kwargs)
    return feats, normals


def one_scale_gpu(query_cloud, search_cloud, edge_length, radius, verbose=False, strict=False):
    """(Nq,4) GPU tensor for one analysis scale."""
    return process_gpu(query_cloud, search_cloud, [edge_length], [radius], verbose=verbose,
                       strict=strict)


def process_single_core(query_cloud, search_cloud, edge_lengths, radii, verbose=False, strict=False,
                        knn_min=0, knn_radius_factor=3.0):
    """compute features at multiple scales.  returns an array of feature vectors aligned with the
    query cloud: numpy (Nq, 4*S) fp64, scale blocks in caller order (multiscale.py:27-67).
    knn_min / knn_radius_factor: see process_gpu (extension, off by default)."""
    assert len(edge_lengths) == len(radii), \
        "edge_lengths and radii should be equal-length sequences."
    shared = query_cloud is search_cloud
    rt, search = _device.as_cloud(search_cloud)
    query = search if shared else _device.as_cloud(query_cloud, rt.device)[1]
    result = process_gpu(query, search, edge_lengths, radii, verbose=verbose, strict=strict,
                         knn_min=knn_min, knn_radius_factor=knn_radius_factor)
    host = result.cpu().numpy()
    # the copy has synchronised the stream: anything a kernel of this call reported is in by now.  an
    # incomplete result is never returned silently.
    rt.check_async(wait=True)
    return host


def one_scale_single_core(query_cloud, search_cloud, edge_length, radius, verbose=False,
                          strict=False):
    """generate a 4d feature vector representing one analysis scale (multiscale.py:70-123)."""
    return process_single_core(query_cloud, search_cloud, [edge_length], [radius], verbose=verbose,
                               strict=strict)


class NeighborIndex(object):
    """the search side of multiscale.py:103, kept: voxel-filter `search_cloud` at `edge_length` once on the
    device, then ask for the neighbor lists of any number of query clouds and radii (the reference's ladders
    are one voxel edge with several radii, nimrud/utils/point_clouds.py:29-35).

    method "index" (what "auto" takes wherever it applies): a dense occupancy index of the lattice plus a
    rank table (nm_neighbor_index_*): the search that finds a neighbor also names it by its np.unique
    position, nothing is sorted and no address is searched for.  lattices with more than 2^21 superblocks
    are outside that path's range; for them "auto" falls back to method "search", today's sorted unique
    addresses (nm_voxelize) searched per candidate cell (nm_scale_neighbors).  same results by contract.

        .method      "index" or "search"
        .n_voxels    M, the number of occupied voxels
        .addresses() their sorted distinct addresses (VoxelFilter.unique_addresses)
        .voxels()    their centres in that order (VoxelFilter.unique_voxels)
        .lists(query_cloud, radius) -> (offsets int64[Nq+1], index int64[total])
    and, on the index form only (a "search" handle raises ValueError), attributes carried onto those voxels:
        .voxel_of(points)       which voxel each point falls in (np.unique's inverse; -1 for none)
        .point_counts()         search points per voxel
        .members()              (start, rows): the search cloud's rows voxel by voxel, ascending
        .voxel_table(attributes, reduce="mean")   per-voxel mean / sum / min / max of per-point columns
        .neighborhood_stats(query_cloud, radius, voxel_values) -> (count, mean, vmin, vmax) per query point
                                over the voxels lists() would name, without writing the lists
        .nearest(query_cloud, k, max_distance=None) -> (distance (Nq, k), index (Nq, k)): the k nearest voxels
                                of every query point (cKDTree(voxels()).query), ties by the smaller position
        .components(radius, voxel_class=None, voxel_weight=None, min_size=1) -> (labels (M,), sizes (C,)): the
                                connected components of the graph lists(voxels(), radius) spans, without the lists
        .dbscan(radius, min_weight, voxel_weight=None, ...) -> (labels (M,), sizes (C,), core (M,)): components of the
                                dense (core) voxels only, border voxels attached, the rest noise (-1)
        .regions(radius, voxel_normal=None, max_angle=None, voxel_value=None, max_step=None, voxel_seed=None, ...)
                                -> (labels (M,), sizes (C,), seed (M,)): region growing - components of the seed
                                voxels under the edges whose normals / values agree, the other voxels attached
        .hill_climb(radius, voxel_value, link="highest", ...) -> (labels (M,), sizes (C,), peaks (C,)): every voxel
                                steps to a higher neighbor, a segment is what climbs to the same peak - it separates
                                objects that touch, which the three connectivity rules above weld into one
        .adjacency(radius, labels, voxel_value=None, voxel_class=None) -> (pair (E, 2), links (E,), saddle (E,) or
                                None): which segments of a labelling touch, over how many voxel edges, and the
                                highest pass between them - the region adjacency graph, without the lists
        .prominent_peaks(radius, voxel_value, min_prominence, link="highest", ...) -> (labels (M,), sizes (C,),
                                peaks (C,), prominence (C,)): hill_climb with the peaks of low prominence merged
                                into their higher neighbors (topological persistence on adjacency's saddles)
        .geodesic(radius, voxel_seed, max_distance=None, ...) -> (distance (M,), labels (M,), sizes (C,), sources (C,)):
                                the length of the shortest path from a seed to every voxel through the graph, and the
                                seed it starts from - segments grown from seeds (trees from their stems)
        .component_table(labels, voxel_weight=None) -> (C, 25): one row of descriptors per component (segment_table
                                over voxels())
    torch in, torch out; numpy in, numpy out (addresses / voxels / point_counts / members / components / dbscan follow the
    search cloud, lists / neighborhood_stats / nearest the query cloud, voxel_of and voxel_table their argument)."""

    def __init__(self, search_cloud, edge_length, method="auto"):
        if method not in ("auto", "index", "search"):
            raise ValueError("method must be 'auto', 'index' or 'search'")
        self._as_torch = isinstance(search_cloud, torch.Tensor)
        self._source = search_cloud
        self._rt, self._search = _device.as_cloud(search_cloud)
        rt, search = self._rt, self._search
        if search.shape[1] < 3:
            raise ValueError("only 3D spaces supported by the multiscale pipeline")
        self.filter = geometry.VoxelFilter(search[:, :3], edge_length, device=rt.device)
        lat = self.filter.nm_lattice
        ns = search.shape[0]
        nbytes = rt.lib.nm_neighbor_index_workspace_bytes(ns, ctypes.byref(lat))
        if nbytes == 0 and method == "index":
            raise ValueError("the lattice has more than 2^21 superblocks: outside the range of the neighbor "
                             "index (method='auto' falls back to the address search)")
        self.method = "index" if (nbytes and method != "search") else "search"
        self._m = None
        self._addr = None
        self._group = None
        if self.method == "search":
            self._addr = self.filter.unique_addresses(search[:, :3])
            self._m = int(self._addr.shape[0])
            return
        # the handle owns its workspace: it lives as long as the lists are asked for
        self._work = torch.empty(int(nbytes), dtype=torch.uint8, device=rt.device)
        self._count = torch.empty(2, dtype=torch.int64, device=rt.device)
        rt.check(rt.lib.nm_neighbor_index_build(
            rt.ctx, _device.ptr(search), ns, _device.row_stride(search), ctypes.byref(lat),
            _device.ptr(self._count), _device.ptr(self._work), self._work.numel(), rt.stream()))

    @property
    def n_voxels(self):
        if self._m is None:
            m, outside = (int(v) for v in self._count.cpu())
            if outside:     # (cannot happen for the cloud the lattice was made from)
                raise ValueError("some points fall outside filter bounding region")
            self._m = m
        return self._m

    def _addresses_device(self):
        if self._addr is None:
            rt = self._rt
            addr = torch.empty(max(self.n_voxels, 1), dtype=torch.int64, device=rt.device)
            rt.check(rt.lib.nm_neighbor_index_addresses(
                rt.ctx, ctypes.byref(self.filter.nm_lattice), _device.ptr(self._work), self._work.numel(),
                _device.ptr(addr), rt.stream()))
            self._addr = addr[:self.n_voxels]
        return self._addr

    def addresses(self):
        addr = self._addresses_device()
        return addr if self._as_torch else addr.cpu().numpy()

    def voxels(self):
        centres = self.filter.address_to_coordinate(self._addresses_device())
        return centres if self._as_torch else centres.cpu().numpy()

    def _enqueue(self, query, radius, counts, offsets, index):
        """one of the two calls (counts, or indices at the offsets) on whichever path this handle uses."""
        rt = self._rt
        lat = self.filter.nm_lattice
        nq = query.shape[0]
        if self.method == "index":
            rt.check(rt.lib.nm_neighbor_index_lists(
                rt.ctx, _device.ptr(query), nq, _device.row_stride(query), ctypes.byref(lat), radius,
                _device.ptr(self._work), self._work.numel(), _device.ptr(counts), _device.ptr(offsets),
                _device.ptr(index), rt.stream()))
        else:
            rt.check(rt.lib.nm_scale_neighbors(
                rt.ctx, _device.ptr(query), nq, _device.row_stride(query), _device.ptr(self._addr),
                self._addr.shape[0], ctypes.byref(lat), radius, _device.ptr(counts),
                _device.ptr(offsets), _device.ptr(index), rt.stream()))

    def lists(self, query_cloud, radius):
        """(offsets int64[Nq+1], index int64[total]): for every query point the ascending positions, in
        addresses() / voxels(), of the voxels within `radius`.  the query cloud may be the search cloud
        the handle was made from (it is then not uploaded again)."""
        as_torch = isinstance(query_cloud, torch.Tensor)
        rt = self._rt
        query = self._search if query_cloud is self._source else _device.as_cloud(query_cloud, rt.device)[1]
        if query.shape[1] < 3:
            raise ValueError("only 3D spaces supported by the multiscale pipeline")
        radius = float(radius)
        nq = query.shape[0]
        offsets = torch.zeros(nq + 1, dtype=torch.int64, device=rt.device)
        total = 0
        if nq:
            counts = torch.empty(nq, dtype=torch.int32, device=rt.device)
            self._enqueue(query, radius, counts, None, None)
            torch.cumsum(counts, 0, out=offsets[1:])
            total = int(offsets[-1])
        index = torch.empty(max(total, 1), dtype=torch.int64, device=rt.device)
        if total:
            self._enqueue(query, radius, None, offsets, index)
        index = index[:total]
        if as_torch:
            return offsets, index
        return offsets.cpu().numpy(), index.cpu().numpy()

    # ---- attributes: from per-point columns to per-neighborhood numbers (method "index" only) ----------------

    def _need_index(self, what):
        if self.method != "index":
            raise ValueError("%s needs the index form of the handle (method='index'); this one searches "
                             "sorted addresses (method='search')" % what)

    def _query_cloud(self, cloud):
        query = self._search if cloud is self._source else _device.as_cloud(cloud, self._rt.device)[1]
        if query.shape[1] < 3:
            raise ValueError("only 3D spaces supported by the multiscale pipeline")
        return query

    def _voxel_of_device(self, points):
        rt = self._rt
        n = points.shape[0]
        voxel = torch.empty(n, dtype=torch.int64, device=rt.device)
        rt.check(rt.lib.nm_neighbor_index_voxel_of(
            rt.ctx, _device.ptr(points), n, _device.row_stride(points), ctypes.byref(self.filter.nm_lattice),
            _device.ptr(self._work), self._work.numel(), _device.ptr(voxel), rt.stream()))
        return voxel

    def voxel_of(self, points):
        """int64 (N,): for every point the position, in addresses() / voxels(), of the voxel it falls in; -1
        where it lies outside the lattice or in a cell no search point occupies.  for the search cloud itself:
        np.unique(addresses, return_inverse=True)[1]."""
        self._need_index("voxel_of")
        voxel = self._voxel_of_device(self._query_cloud(points))
        return voxel if isinstance(points, torch.Tensor) else voxel.cpu().numpy()

    def _grouping(self):
        """(counts (M,), start (M+1,), rows (Ns,)) of the search cloud on the device, made once."""
        if self._group is None:
            rt = self._rt
            m, ns = self.n_voxels, self._search.shape[0]
            voxel = self._voxel_of_device(self._search)
            counts = torch.empty(max(m, 1), dtype=torch.int64, device=rt.device)
            start = torch.empty(m + 1, dtype=torch.int64, device=rt.device)
            rows = torch.empty(max(ns, 1), dtype=torch.int64, device=rt.device)
            nbytes = rt.lib.nm_neighbor_index_group_workspace_bytes(max(ns, m))
            tmp = rt.workspace(nbytes)
            rt.check(rt.lib.nm_neighbor_index_group(
                rt.ctx, _device.ptr(voxel), ns, m, _device.ptr(counts), _device.ptr(start), _device.ptr(rows),
                _device.ptr(tmp), tmp.numel(), rt.stream()))
            self._group = (counts[:m], start, rows[:ns])
        return self._group

    def point_counts(self):
        """int64 (M,): search points per voxel (np.unique's return_counts)."""
        self._need_index("point_counts")
        counts = self._grouping()[0]
        return counts if self._as_torch else counts.cpu().numpy()

    def members(self):
        """(start int64[M+1], rows int64[Ns]): the rows of the search cloud voxel by voxel - voxel v holds
        rows[start[v]:start[v+1]], ascending.  rows is np.argsort(voxel_of(search_cloud), kind="stable"),
        the same on every run."""
        self._need_index("members")
        _, start, rows = self._grouping()
        return (start, rows) if self._as_torch else (start.cpu().numpy(), rows.cpu().numpy())

    def voxel_table(self, attributes, reduce="mean"):
        """fp64 (M, D): per voxel the `reduce` ("mean", "sum", "min" or "max") of the attribute rows of the
        search points in it.  attributes is (Ns, D) or (Ns,), 1 <= D <= 16.  "sum" adds in ascending row order
        (np.bincount(inverse, weights=column), bit for bit), "mean" divides that sum once by the count.
        NaN attribute values are not supported (like NaN coordinates)."""
        self._need_index("voxel_table")
        if reduce not in _ffi.NM_REDUCE:
            raise ValueError("reduce must be one of 'mean', 'sum', 'min', 'max'")
        rt = self._rt
        attr = torch.as_tensor(attributes).to(device=rt.device, dtype=torch.float64)
        if attr.ndim == 1:
            attr = attr.reshape(-1, 1)
        if attr.ndim != 2 or attr.shape[0] != self._search.shape[0]:
            raise ValueError("attributes must have one row per search point")
        dims = int(attr.shape[1])
        if not 1 <= dims <= _ffi.NM_STATS_MAX_DIMS:
            raise ValueError("between 1 and %d attribute columns per call" % _ffi.NM_STATS_MAX_DIMS)
        attr = _unit_columns(attr)
        _, start, rows = self._grouping()
        m = self.n_voxels
        table = torch.empty((m, dims), dtype=torch.float64, device=rt.device)
        rt.check(rt.lib.nm_neighbor_index_voxel_reduce(
            rt.ctx, _device.ptr(start), _device.ptr(rows), m, _device.ptr(attr), _device.row_stride(attr), dims,
            _ffi.NM_REDUCE[reduce], _device.ptr(table), rt.stream()))
        return table if isinstance(attributes, torch.Tensor) else table.cpu().numpy()

    def _voxel_values(self, voxel_values):
        """a voxel table as an fp64 device tensor (M, D) with unit column stride (a row stride is kept)"""
        values = torch.as_tensor(voxel_values).to(device=self._rt.device, dtype=torch.float64)
        if values.ndim == 1:
            values = values.reshape(-1, 1)
        if values.ndim != 2 or values.shape[0] != self.n_voxels:
            raise ValueError("voxel_values must have one row per voxel")
        if not 1 <= values.shape[1] <= _ffi.NM_STATS_MAX_DIMS:
            raise ValueError("between 1 and %d attribute columns per call" % _ffi.NM_STATS_MAX_DIMS)
        return _unit_columns(values)

    def _stats_into(self, query, radius, values, count, mean, vmin, vmax, out_stride):
        """enqueue nm_neighbor_index_stats: count (Nq,) int32 and three (Nq, D) blocks at row pitch out_stride"""
        rt = self._rt
        rt.check(rt.lib.nm_neighbor_index_stats(
            rt.ctx, _device.ptr(query), query.shape[0], _device.row_stride(query),
            ctypes.byref(self.filter.nm_lattice), float(radius), _device.ptr(self._work), self._work.numel(),
            _device.ptr(values), _device.row_stride(values), int(values.shape[1]), _device.ptr(count), mean, vmin,
            vmax, int(out_stride), rt.stream()))

    def neighborhood_stats(self, query_cloud, radius, voxel_values):
        """(count int32 (Nq,), mean, vmin, vmax fp64 (Nq, D)): over the voxels within `radius` of each query
        point - the voxels lists() names - how many there are and, per column of voxel_values ((M, D) or (M,),
        1 <= D <= 16, e.g. a voxel_table), their mean (summed in ascending voxel order, divided once by the
        count), minimum and maximum.  no list is written.  a query point with no voxel in reach gets count 0
        and zeros in all three tables.  NaN values are not supported (like NaN coordinates)."""
        self._need_index("neighborhood_stats")
        rt = self._rt
        query = self._query_cloud(query_cloud)
        values = self._voxel_values(voxel_values)
        nq, dims = query.shape[0], int(values.shape[1])
        count = torch.zeros(nq, dtype=torch.int32, device=rt.device)
        mean, vmin, vmax = (torch.zeros((nq, dims), dtype=torch.float64, device=rt.device) for _ in range(3))
        self._stats_into(query, radius, values, count, _device.ptr(mean), _device.ptr(vmin), _device.ptr(vmax), dims)
        out = (count, mean, vmin, vmax)
        return out if isinstance(query_cloud, torch.Tensor) else tuple(t.cpu().numpy() for t in out)

    def _nearest_device(self, query, k, max_distance):
        """enqueue nm_neighbor_index_nearest: (d2 fp64 (Nq, k), index int64 (Nq, k), found int32 (Nq,))"""
        rt = self._rt
        nq = query.shape[0]
        dist2 = torch.empty((nq, k), dtype=torch.float64, device=rt.device)
        index = torch.empty((nq, k), dtype=torch.int64, device=rt.device)
        found = torch.empty(nq, dtype=torch.int32, device=rt.device)
        if nq == 0:
            return dist2, index, found
        tmp = rt.workspace(rt.lib.nm_neighbor_index_nearest_workspace_bytes(nq))
        rt.check(rt.lib.nm_neighbor_index_nearest(
            rt.ctx, _device.ptr(query), nq, _device.row_stride(query), ctypes.byref(self.filter.nm_lattice), k,
            max_distance, _device.ptr(self._work), self._work.numel(), _device.ptr(dist2), _device.ptr(index), k,
            _device.ptr(found), _device.ptr(tmp), tmp.numel(), rt.stream()))
        return dist2, index, found

    def nearest(self, query_cloud, k, max_distance=None, squared=False):
        """(distance fp64 (Nq, k), index int64 (Nq, k)): for every query point its k nearest occupied voxels -
        cKDTree(voxels()).query(query_cloud, k, distance_upper_bound), the other half of the tree at
        multiscale.py:87 - nearest first.  the squared distance to a voxel centre is formed as lists() forms it;
        voxels are ordered by (squared distance, position in addresses() / voxels()), so equal distances are
        broken by the smaller position (scipy leaves ties unspecified).  with `max_distance` only voxels with
        d2 <= max_distance * max_distance count: inclusive, like lists() (scipy's distance_upper_bound is
        exclusive); None is no limit.  a row with fewer than k such voxels ends in distance inf and index -1,
        the handle's "none" as in voxel_of (scipy writes M there).  always 2-D, also for k = 1 (scipy squeezes).
        1 <= k <= 32.  distance is torch.sqrt of the squared distance, or that itself with squared=True.  query
        points may lie anywhere, outside the lattice too; the search cloud passed by identity is not uploaded
        again."""
        self._need_index("nearest")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError("k must be an integer")
        k = int(k)
        if not 1 <= k <= _ffi.NM_NEAREST_MAX_K:
            raise ValueError("k must lie in [1, %d]" % _ffi.NM_NEAREST_MAX_K)
        limit = float("inf") if max_distance is None else float(max_distance)
        if not limit >= 0.0:
            raise ValueError("max_distance must be a number >= 0 (None: no limit)")
        query = self._query_cloud(query_cloud)
        dist2, index, _ = self._nearest_device(query, k, limit)
        distance = dist2 if squared else torch.sqrt(dist2)
        if isinstance(query_cloud, torch.Tensor):
            return distance, index
        return distance.cpu().numpy(), index.cpu().numpy()

    def _voxel_integers(self, values, what):
        """an integer array with one entry per voxel as an int64 device tensor (M,)"""
        return _integer_column(values, self.n_voxels, self._rt.device, what, "voxel")

    def _components_device(self, radius, voxel_class, voxel_weight, min_size):
        """enqueue nm_neighbor_index_components on int64 device tensors (or None); one host read, of the counts"""
        rt = self._rt
        m = self.n_voxels
        labels = torch.empty(m, dtype=torch.int64, device=rt.device)
        sizes = torch.empty(max(m, 1), dtype=torch.int64, device=rt.device)
        if m == 0:
            return labels, sizes[:0]
        count = torch.empty(2, dtype=torch.int64, device=rt.device)
        nbytes = int(rt.lib.nm_neighbor_index_components_workspace_bytes(m))
        tmp = rt.workspace(nbytes)
        rt.check(rt.lib.nm_neighbor_index_components(
            rt.ctx, ctypes.byref(self.filter.nm_lattice), radius, _device.ptr(self._work), self._work.numel(),
            _device.ptr(voxel_class), _device.ptr(voxel_weight), min_size, _device.ptr(labels), _device.ptr(sizes),
            _device.ptr(count), _device.ptr(tmp), nbytes, rt.stream()))
        kept = int(count[0])
        if kept < 0:        # (cannot happen: the scratch was sized for this handle's M)
            raise _ffi.NimrudHipError("nm_neighbor_index_components: scratch too small for the index")
        return labels, sizes[:kept]

    def components(self, radius, voxel_class=None, voxel_weight=None, min_size=1):
        """(labels int64 (M,), sizes int64 (C,)): the connected components of the voxel graph - Euclidean cluster
        extraction.  voxels u and v are joined when lists(voxels(), radius) names one for the other (the limit is
        inclusive), and a component is what can be reached in such steps.  no edge list is written.
        voxel_class (integers, (M,)): a negative class takes the voxel out of the graph, and an edge joins voxels of
        equal class only, so one call segments every class; None is one class for all.  voxel_weight (integers,
        (M,), e.g. point_counts()): a component's size is the sum of its weights; None counts voxels.  components
        of a size below min_size are dropped.  kept components are numbered 0..C-1 in ascending order of their
        smallest voxel position; voxels outside the graph or in a dropped component get -1.  the result is a
        function of the arguments alone, the same bit for bit on every run."""
        self._need_index("components")
        radius = float(radius)
        if not radius >= 0.0:
            raise ValueError("radius must be a number >= 0")
        if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)):
            raise ValueError("min_size must be an integer")
        cls = None if voxel_class is None else self._voxel_integers(voxel_class, "voxel_class")
        weight = None if voxel_weight is None else self._voxel_integers(voxel_weight, "voxel_weight")
        labels, sizes = self._components_device(radius, cls, weight, int(min_size))
        return (labels, sizes) if self._as_torch else (labels.cpu().numpy(), sizes.cpu().numpy())

    def _dbscan_device(self, radius, min_weight, voxel_class, voxel_weight, min_size, want_density,
                       check_weight=False):
        """enqueue nm_neighbor_index_dbscan on int64 device tensors (or None): (labels, sizes, core bool, density or
        None); one host read, of the counts - with check_weight the sign of the smallest weight comes down with them"""
        rt = self._rt
        m = self.n_voxels
        labels = torch.empty(m, dtype=torch.int64, device=rt.device)
        sizes = torch.empty(max(m, 1), dtype=torch.int64, device=rt.device)
        core = torch.empty(m, dtype=torch.uint8, device=rt.device)
        density = torch.empty(m, dtype=torch.int64, device=rt.device) if want_density else None
        if m == 0:
            return labels, sizes[:0], core.to(torch.bool), density
        count = torch.empty(3, dtype=torch.int64, device=rt.device)
        nbytes = int(rt.lib.nm_neighbor_index_dbscan_workspace_bytes(m))
        tmp = rt.workspace(nbytes)
        rt.check(rt.lib.nm_neighbor_index_dbscan(
            rt.ctx, ctypes.byref(self.filter.nm_lattice), radius, min_weight, _device.ptr(self._work),
            self._work.numel(), _device.ptr(voxel_class), _device.ptr(voxel_weight), min_size, _device.ptr(labels),
            _device.ptr(sizes), _device.ptr(core), _device.ptr(density), _device.ptr(count), _device.ptr(tmp), nbytes,
            rt.stream()))
        if check_weight and voxel_weight is not None:
            kept, negative = (int(x) for x in torch.stack((count[0], (voxel_weight < 0).any().to(torch.int64))).cpu())
            if negative:
                raise ValueError("voxel_weight must not be negative")
        else:
            kept = int(count[0])
        if kept < 0:        # (cannot happen: the scratch was sized for this handle's M)
            raise _ffi.NimrudHipError("nm_neighbor_index_dbscan: scratch too small for the index")
        return labels, sizes[:kept], core.to(torch.bool), density

    def dbscan(self, radius, min_weight, voxel_weight=None, voxel_class=None, min_size=1, return_density=False):
        """(labels int64 (M,), sizes int64 (C,), core bool (M,)) and, with return_density, density int64 (M,): DBSCAN on
        the voxel graph of components() - voxels u and v are neighbors when lists(voxels(), radius) names one for the
        other and both carry the same voxel_class >= 0 (None: one class for all; a negative class takes the voxel out:
        label -1, not core, density 0).  density[v] is the sum of voxel_weight (integers >= 0, (M,), e.g.
        point_counts(); None counts voxels; a negative weight raises ValueError) over v itself and its neighbors, and v is a CORE voxel where density[v] >=
        min_weight (sklearn's min_samples with sample_weight).  the clusters are the connected components of the core
        voxels.  a voxel that is not core joins the cluster of its nearest core neighbor - by (squared distance as
        lists() forms it, position), equal distances to the smaller position - as a BORDER voxel, and without a core
        neighbor it is noise, label -1.  a cluster's size is the sum of the weights of its members, core and border;
        clusters below min_size are dropped, their members get -1 and `core` stays.  kept clusters are numbered
        0..C-1 in ascending order of their smallest core voxel position.  with voxel_weight None and min_weight <= 1
        every voxel is core and (labels, sizes) are those of components().  the result is a function of the arguments
        alone, the same bit for bit on every run."""
        self._need_index("dbscan")
        radius = float(radius)
        if not radius >= 0.0:
            raise ValueError("radius must be a number >= 0")
        for name, value in (("min_weight", min_weight), ("min_size", min_size)):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
                raise ValueError("%s must be an integer" % name)
        cls = None if voxel_class is None else self._voxel_integers(voxel_class, "voxel_class")
        weight = None if voxel_weight is None else self._voxel_integers(voxel_weight, "voxel_weight")
        out = self._dbscan_device(radius, int(min_weight), cls, weight, int(min_size), bool(return_density),
                                  check_weight=True)
        out = out if return_density else out[:3]
        return out if self._as_torch else tuple(t.cpu().numpy() for t in out)

    def _voxel_rows(self, values, what, most):
        """a per-voxel fp64 table as a device tensor (M, D <= most) with unit column stride (a row stride is kept)"""
        t = torch.as_tensor(values)
        if not t.dtype.is_floating_point:
            raise ValueError("%s must have a floating-point dtype" % what)
        t = t.to(device=self._rt.device, dtype=torch.float64)
        if t.ndim == 1:
            t = t.reshape(-1, 1)
        if t.ndim != 2 or t.shape[0] != self.n_voxels:
            raise ValueError("%s must have one row per voxel" % what)
        if not 1 <= t.shape[1] <= most:
            raise ValueError("%s must have between 1 and %d columns" % (what, most))
        return _unit_columns(t)

    def _regions_device(self, radius, normal, min_cos, value, max_step, seed, voxel_class, voxel_weight, min_size):
        """enqueue nm_neighbor_index_regions on device tensors (or None) - normal fp64 (M, >= 3), value fp64 (M, D),
        seed uint8 (M,), class and weight int64 (M,); max_step: D host floats - (labels, sizes, seed bool: the seeds
        in the graph); one host read, of the counts"""
        rt = self._rt
        m = self.n_voxels
        labels = torch.empty(m, dtype=torch.int64, device=rt.device)
        sizes = torch.empty(max(m, 1), dtype=torch.int64, device=rt.device)
        in_graph = torch.ones(m, dtype=torch.bool, device=rt.device) if voxel_class is None else voxel_class >= 0
        is_seed = in_graph if seed is None else in_graph & (seed != 0)
        if m == 0:
            return labels, sizes[:0], is_seed
        dims = 0 if value is None else int(value.shape[1])
        steps = (ctypes.c_double * max(dims, 1))(*[float(s) for s in max_step])
        count = torch.empty(3, dtype=torch.int64, device=rt.device)
        nbytes = int(rt.lib.nm_neighbor_index_regions_workspace_bytes(m))
        tmp = rt.workspace(nbytes)
        rt.check(rt.lib.nm_neighbor_index_regions(
            rt.ctx, ctypes.byref(self.filter.nm_lattice), radius, _device.ptr(self._work), self._work.numel(),
            _device.ptr(voxel_class), _device.ptr(voxel_weight), _device.ptr(seed), _device.ptr(normal),
            _device.row_stride(normal) if normal is not None else 0, min_cos, _device.ptr(value),
            _device.row_stride(value) if value is not None else 0, dims, steps, min_size, _device.ptr(labels),
            _device.ptr(sizes), _device.ptr(count), _device.ptr(tmp), nbytes, rt.stream()))
        kept = int(count[0])
        if kept < 0:        # (cannot happen: the scratch was sized for this handle's M)
            raise _ffi.NimrudHipError("nm_neighbor_index_regions: scratch too small for the index")
        return labels, sizes[:kept], is_seed

    def regions(self, radius, voxel_normal=None, max_angle=None, voxel_value=None, max_step=None, voxel_seed=None,
                voxel_class=None, voxel_weight=None, min_size=1):
        """(labels int64 (M,), sizes int64 (C,), seed bool (M,)): region growing under a smoothness constraint, stated
        as connected components - the voxel graph of components() (voxels u and v are neighbors when lists(voxels(),
        radius) names one for the other and both carry the same voxel_class >= 0), in which only SEEDS link, and two
        neighboring seeds link only when both of these hold:
          voxel_normal (fp64 (M, 3)) and max_angle (radians) given: fabs(dot(n_u, n_v)) >= cos(max_angle), the dot
            product as (x*x + y*y) + z*z, unfused.  normals are unsigned directions and are not normalised here; a
            NaN normal links nothing, a zero normal only where cos(max_angle) <= 0.
          voxel_value ((M,) or (M, D), D <= 4) and max_step (a scalar or (D,), >= 0) given: fabs(value_u[c] -
            value_v[c]) <= max_step[c] in every column, inclusive; NaN is false.
        voxel_seed (bool or integers, (M,)): non-zero makes a voxel of the graph a seed; None: every voxel of the
        graph.  the regions are the connected components of the seeds under the linked edges.  a voxel of the graph
        that is no seed joins the region of its nearest seed neighbor of its class - by (squared distance as lists()
        forms it, position), the rule above is not asked - and without one it gets -1.  a region's size is the sum
        of voxel_weight (integers, (M,); None counts voxels) over all its members; regions below min_size are
        dropped, their members get -1.  kept regions are numbered 0..C-1 in ascending order of their smallest seed
        position.  `seed` returns the seeds in the graph.  without seeds and rules this is components(); with a
        dbscan() call's core as voxel_seed and no rule, that call's labels and sizes.  the result is a function of
        the arguments alone, the same bit for bit on every run (PCL's RegionGrowing depends on its seed order)."""
        self._need_index("regions")
        radius = float(radius)
        if not radius >= 0.0:
            raise ValueError("radius must be a number >= 0")
        if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)):
            raise ValueError("min_size must be an integer")
        if (voxel_normal is None) != (max_angle is None):
            raise ValueError("voxel_normal and max_angle go together: give both or neither")
        if (voxel_value is None) != (max_step is None):
            raise ValueError("voxel_value and max_step go together: give both or neither")
        normal, min_cos = None, 0.0
        if voxel_normal is not None:
            max_angle = float(max_angle)
            if max_angle != max_angle:
                raise ValueError("max_angle must be a number (radians)")
            min_cos = _min_cos(max_angle)
            normal = self._voxel_rows(voxel_normal, "voxel_normal", 3)
            if normal.shape[1] != 3:
                raise ValueError("voxel_normal must be (M, 3)")
        value, steps = None, ()
        if voxel_value is not None:
            value = self._voxel_rows(voxel_value, "voxel_value", _ffi.NM_REGION_MAX_DIMS)
            dims = int(value.shape[1])
            steps = np.asarray(max_step, dtype=np.float64)
            if steps.ndim == 0:
                steps = np.full(dims, float(steps))
            if steps.shape != (dims,) or not (steps >= 0.0).all():      # (NaN fails)
                raise ValueError("max_step must be a number >= 0, or one per column of voxel_value")
        seed = None
        if voxel_seed is not None:
            if isinstance(voxel_seed, torch.Tensor) and voxel_seed.dtype == torch.bool:
                voxel_seed = voxel_seed.to(torch.uint8)
            elif not isinstance(voxel_seed, torch.Tensor) and np.asarray(voxel_seed).dtype == np.bool_:
                voxel_seed = np.asarray(voxel_seed).astype(np.uint8)
            seed = (self._voxel_integers(voxel_seed, "voxel_seed") != 0).to(torch.uint8)
        cls = None if voxel_class is None else self._voxel_integers(voxel_class, "voxel_class")
        weight = None if voxel_weight is None else self._voxel_integers(voxel_weight, "voxel_weight")
        out = self._regions_device(radius, normal, min_cos, value, steps, seed, cls, weight, int(min_size))
        return out if self._as_torch else tuple(t.cpu().numpy() for t in out)

    def _hill_climb_device(self, radius, value, mode, voxel_class, voxel_weight, min_size, want_link):
        """enqueue nm_neighbor_index_hill_climb on device tensors - value fp64 (M,) contiguous, class and weight int64
        (M,) or None, mode NM_CLIMB_* - (labels, sizes, peaks, link or None); one host read, of the counts"""
        rt = self._rt
        m = self.n_voxels
        labels = torch.empty(m, dtype=torch.int64, device=rt.device)
        sizes = torch.empty(max(m, 1), dtype=torch.int64, device=rt.device)
        peaks = torch.empty(max(m, 1), dtype=torch.int64, device=rt.device)
        link = torch.empty(m, dtype=torch.int64, device=rt.device) if want_link else None
        if m == 0:
            return labels, sizes[:0], peaks[:0], link
        count = torch.empty(2, dtype=torch.int64, device=rt.device)
        nbytes = int(rt.lib.nm_neighbor_index_hill_climb_workspace_bytes(m))
        tmp = rt.workspace(nbytes)
        rt.check(rt.lib.nm_neighbor_index_hill_climb(
            rt.ctx, ctypes.byref(self.filter.nm_lattice), radius, mode, _device.ptr(self._work), self._work.numel(),
            _device.ptr(value), _device.ptr(voxel_class), _device.ptr(voxel_weight), min_size, _device.ptr(labels),
            _device.ptr(sizes), _device.ptr(peaks), _device.ptr(link), _device.ptr(count), _device.ptr(tmp), nbytes,
            rt.stream()))
        kept = int(count[0])
        if kept < 0:        # (cannot happen: the scratch was sized for this handle's M)
            raise _ffi.NimrudHipError("nm_neighbor_index_hill_climb: scratch too small for the index")
        return labels, sizes[:kept], peaks[:kept], link

    def hill_climb(self, radius, voxel_value, link="highest", voxel_class=None, voxel_weight=None, min_size=1,
                   return_link=False):
        """(labels int64 (M,), sizes int64 (C,), peaks int64 (C,)) and, with return_link, link int64 (M,): peak-seeking
        segments of the voxel graph of components() - voxels u and v are neighbors when lists(voxels(), radius) names
        one for the other and both carry the same voxel_class >= 0 (None: one class for all).  voxel_value (floating
        point, (M,)) is the height every voxel climbs on; a voxel with a NaN value or a negative class is out of the
        graph: label -1, link -1.  u is HIGHER than v when value[u] > value[v], or the values are equal and u < v (the
        smaller position) - a strict total order, so links never form a cycle.  every voxel of the graph links to one of
        its higher neighbors of its class:
          link="highest" (steepest ascent, crown delineation with height as the value): the largest value; among equal
            values the smaller squared distance as lists() forms it; among equal distances the smaller position.
          link="nearest" (quick shift, e.g. on dbscan(return_density=True)'s density): the smallest squared distance;
            among equal distances the larger value; then the smaller position.
        a voxel without a higher neighbor is a PEAK and links to itself; a segment is everything whose links lead to
        the same peak, so two objects that touch stay two where components(), dbscan() and regions() weld them.  a
        plateau of equal values climbs to its smallest position as far as the radius lets it (one that is not convex
        at that radius may split).  a segment's size is the sum of voxel_weight (integers, (M,); None counts voxels)
        over its members; segments below min_size are dropped, their members get -1.  kept segments are numbered
        0..C-1 in ascending order of their peak's position, peaks[c] is that position (voxels()[peaks] are the peaks'
        centres).  link is every voxel's uphill neighbor, whatever min_size dropped.  the result is a function of
        the arguments alone, the same bit for bit on every run."""
        self._need_index("hill_climb")
        radius = float(radius)
        if not radius >= 0.0:
            raise ValueError("radius must be a number >= 0")
        if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)):
            raise ValueError("min_size must be an integer")
        if link not in _ffi.NM_CLIMB:
            raise ValueError("link must be 'highest' or 'nearest'")
        value = self._voxel_heights(voxel_value, "voxel_value")
        cls = None if voxel_class is None else self._voxel_integers(voxel_class, "voxel_class")
        weight = None if voxel_weight is None else self._voxel_integers(voxel_weight, "voxel_weight")
        out = self._hill_climb_device(radius, value, _ffi.NM_CLIMB[link], cls, weight, int(min_size),
                                      bool(return_link))
        out = out if return_link else out[:3]
        return out if self._as_torch else tuple(t.cpu().numpy() for t in out)

    def _voxel_heights(self, values, what):
        """a floating-point array with one entry per voxel as a contiguous fp64 device tensor (M,)"""
        t = torch.as_tensor(values)
        if not t.dtype.is_floating_point:
            raise ValueError("%s must have a floating-point dtype" % what)
        if t.ndim != 1 or t.shape[0] != self.n_voxels:
            raise ValueError("%s must have one entry per voxel" % what)
        return t.to(device=self._rt.device, dtype=torch.float64).contiguous()

    def _voxel_seeds(self, values, what):
        """bool or integers with one entry per voxel as a uint8 device tensor (M,): 1 where non-zero"""
        if isinstance(values, torch.Tensor) and values.dtype == torch.bool:
            values = values.to(torch.uint8)
        elif not isinstance(values, torch.Tensor) and np.asarray(values).dtype == np.bool_:
            values = np.asarray(values).astype(np.uint8)
        return (self._voxel_integers(values, what) != 0).to(torch.uint8)

    # sweeps per nm_neighbor_index_geodesic_relax call: the first batch, the factor the next ones grow by, the largest.
    # sweeps queued behind the fixpoint return at once, so a generous batch costs launches only
    _GEODESIC_BATCHES = (8, 2, 256)

    def _geodesic_device(self, radius, seed, max_distance, voxel_class, voxel_weight, min_size, want_link,
                         stages=None):
        """enqueue nm_neighbor_index_geodesic_relax in batches until a batch's last sweep lowers nothing, then
        nm_neighbor_index_geodesic_finish, on device tensors - seed uint8 (M,), class and weight int64 (M,) or None -
        (distance, labels, sizes, sources, link or None); one host read per batch and one of finish's counts.
        stages: a callable(name, sweeps) the timing tool is told the end of every stage through"""
        rt = self._rt
        m = self.n_voxels
        mark = stages if stages is not None else (lambda name, sweeps: None)
        dist = torch.empty(m, dtype=torch.float64, device=rt.device)
        labels = torch.empty(m, dtype=torch.int64, device=rt.device)
        sizes = torch.empty(max(m, 1), dtype=torch.int64, device=rt.device)
        sources = torch.empty(max(m, 1), dtype=torch.int64, device=rt.device)
        link = torch.empty(m, dtype=torch.int64, device=rt.device) if want_link else None
        if m == 0:
            return dist, labels, sizes[:0], sources[:0], link
        lat = ctypes.byref(self.filter.nm_lattice)
        count = torch.empty(3, dtype=torch.int64, device=rt.device)
        nbytes = int(rt.lib.nm_neighbor_index_geodesic_workspace_bytes(m))
        # (its own: the addresses in it must outlive the host reads between the batches)
        tmp = torch.empty(nbytes, dtype=torch.uint8, device=rt.device)
        batch, grow, most = self._GEODESIC_BATCHES
        done, first = 0, 1
        while True:
            if done > m + 1:        # (Bellman-Ford: at most M - 1 sweeps lower anything)
                raise _ffi.NimrudHipError("nm_neighbor_index_geodesic_relax: no fixpoint after %d sweeps of %d voxels"
                                          % (done, m))
            sweeps = min(batch, m + 2 - done)
            rt.check(rt.lib.nm_neighbor_index_geodesic_relax(
                rt.ctx, lat, radius, _device.ptr(self._work), self._work.numel(), _device.ptr(seed),
                _device.ptr(voxel_class), max_distance, first, sweeps, _device.ptr(dist), _device.ptr(count),
                _device.ptr(tmp), nbytes, rt.stream()))
            done += sweeps
            first = 0
            lowered = int(count[0])
            mark("relax", sweeps)
            if lowered < 0:     # (cannot happen: the scratch was sized for this handle's M)
                raise _ffi.NimrudHipError("nm_neighbor_index_geodesic_relax: scratch too small for the index")
            if lowered == 0:
                break
            batch = min(batch * grow, most)
        rt.check(rt.lib.nm_neighbor_index_geodesic_finish(
            rt.ctx, lat, radius, _device.ptr(self._work), self._work.numel(), _device.ptr(voxel_class),
            _device.ptr(voxel_weight), min_size, _device.ptr(dist), _device.ptr(labels), _device.ptr(sizes),
            _device.ptr(sources), _device.ptr(link), _device.ptr(count), _device.ptr(tmp), nbytes, rt.stream()))
        kept, _, orphans = (int(v) for v in count.cpu())
        mark("finish", 0)
        if kept < 0:
            raise _ffi.NimrudHipError("nm_neighbor_index_geodesic_finish: scratch too small for the index")
        if orphans:
            raise _ffi.NimrudHipError("nm_neighbor_index_geodesic_finish: %d reached voxels without a link: the "
                                      "distances are not at their fixpoint" % orphans)
        return dist, labels, sizes[:kept], sources[:kept], link

    def geodesic(self, radius, voxel_seed, max_distance=None, voxel_class=None, voxel_weight=None, min_size=1,
                 return_link=False):
        """(distance fp64 (M,), labels int64 (M,), sizes int64 (C,), sources int64 (C,)) and, with return_link, link
        int64 (M,): shortest paths from seeds over the voxel graph of components() - voxels u and v are neighbors when
        lists(voxels(), radius) names one for the other and both carry the same voxel_class >= 0 (None: one class for
        all); a voxel of negative class is out of the graph: distance +inf, label -1, link -1.  an edge is as long as
        its two centres are apart: sqrt((dx*dx + dy*dy) + dz*dz), the squared distance as lists() forms it.
        voxel_seed (bool or integers, (M,)): non-zero makes a voxel of the graph a seed, at distance 0.  distance[v] is
        the length of the shortest path from any seed to v THROUGH the graph - around gaps and obstacles, where
        nearest() measures through them: the least fixpoint of distance[v] = min over neighbors u of
        fl(distance[u] + w(u, v)), which is what Dijkstra's algorithm in fp64 returns (scipy.sparse.csgraph.dijkstra
        with min_only), bit for bit.  max_distance (a number >= 0; None or inf: no limit): a path longer than that is
        not taken - the limit is inclusive - and nothing is reached through a voxel beyond it.  unreached voxels keep
        +inf, label -1 and link -1.
        u is LOWER than v when distance[u] < distance[v], or they are equal and u < v.  link[v] is, among the neighbors
        u of v's class that are lower than v and have fl(distance[u] + w(u, v)) == distance[v], the one of the
        smallest distance, then of the smallest position; v itself at a seed.  a segment is everything whose links lead
        to the same seed: the Voronoi cells of the seeds in the graph metric - trees from their stems where the crowns
        interlock, with the stem voxels as seeds.  a voxel equally far from two seeds goes by that rule, never by the
        order anything ran in.  a segment's size is the sum of voxel_weight (integers, (M,); None counts voxels) over
        its members; segments below min_size are dropped: their members get -1, distance and link stay.  kept
        segments are numbered 0..C-1 in ascending order of their seed's position, sources[c] is that position.
        the work is relaxation sweeps, one full-window walk per voxel each, about as many as the longest shortest
        path has edges; they are enqueued in growing batches, and the call SYNCHRONISES ONCE PER BATCH to read how many
        voxels the batch's last sweep lowered (and once more for the counts of the segments).  the result is a
        function of the arguments alone, the same bit for bit on every run."""
        self._need_index("geodesic")
        radius = float(radius)
        if not radius >= 0.0:
            raise ValueError("radius must be a number >= 0")
        if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)):
            raise ValueError("min_size must be an integer")
        max_distance = float("inf") if max_distance is None else float(max_distance)
        if not max_distance >= 0.0:
            raise ValueError("max_distance must be a number >= 0, or None")
        seed = self._voxel_seeds(voxel_seed, "voxel_seed")
        cls = None if voxel_class is None else self._voxel_integers(voxel_class, "voxel_class")
        weight = None if voxel_weight is None else self._voxel_integers(voxel_weight, "voxel_weight")
        out = self._geodesic_device(radius, seed, max_distance, cls, weight, int(min_size), bool(return_link))
        out = out if return_link else out[:4]
        return out if self._as_torch else tuple(t.cpu().numpy() for t in out)

    def _adjacency_device(self, radius, label, value, voxel_class, stages=None):
        """enqueue nm_neighbor_index_adjacency (count, then records) and nm_neighbor_index_adjacency_reduce around a
        torch.sort of the records' keys, on device tensors - label int64 (M,), value fp64 (M,) or None, class int64
        (M,) or None - (pair (E, 2), links (E,), saddle (E,) or None); two host reads: the records, then the rows.
        stages: a callable(name) the timing tool is told the end of every stage through"""
        rt = self._rt
        m = self.n_voxels
        mark = stages if stages is not None else (lambda name: None)
        lat = ctypes.byref(self.filter.nm_lattice)

        def empty():
            return (torch.empty((0, 2), dtype=torch.int64, device=rt.device),
                    torch.empty(0, dtype=torch.int64, device=rt.device),
                    None if value is None else torch.empty(0, dtype=torch.float64, device=rt.device))

        if m == 0:
            return empty()
        count = torch.empty(2, dtype=torch.int64, device=rt.device)
        nbytes = int(rt.lib.nm_neighbor_index_adjacency_workspace_bytes(m, 0))
        tmp = torch.empty(nbytes, dtype=torch.uint8, device=rt.device)

        def walk(capacity, key, links, saddle):
            rt.check(rt.lib.nm_neighbor_index_adjacency(
                rt.ctx, lat, radius, _device.ptr(self._work), self._work.numel(), _device.ptr(label),
                _device.ptr(value), _device.ptr(voxel_class), capacity, _device.ptr(key), _device.ptr(links),
                _device.ptr(saddle), _device.ptr(count), _device.ptr(tmp), nbytes, rt.stream()))

        walk(0, None, None, None)
        records, bad = (int(v) for v in count.cpu())
        if bad < 0:         # (cannot happen: the scratch was sized for this handle's M)
            raise _ffi.NimrudHipError("nm_neighbor_index_adjacency: scratch too small for the index")
        if bad:
            raise ValueError("labels must be below 2^31 (%d are not)" % bad)
        mark("count")
        if records == 0:
            return empty()
        key = torch.empty(records, dtype=torch.int64, device=rt.device)
        links = torch.empty(records, dtype=torch.int64, device=rt.device)
        saddle = None if value is None else torch.empty(records, dtype=torch.float64, device=rt.device)
        walk(records, key, links, saddle)
        mark("emit")
        key, order = torch.sort(key, stable=True)
        mark("sort")
        pair = torch.empty((records, 2), dtype=torch.int64, device=rt.device)
        row_links = torch.empty(records, dtype=torch.int64, device=rt.device)
        row_saddle = None if value is None else torch.empty(records, dtype=torch.float64, device=rt.device)
        nbytes_rows = int(rt.lib.nm_neighbor_index_adjacency_workspace_bytes(0, records))
        tmp_rows = tmp if nbytes_rows <= nbytes else torch.empty(nbytes_rows, dtype=torch.uint8, device=rt.device)
        rt.check(rt.lib.nm_neighbor_index_adjacency_reduce(
            rt.ctx, records, _device.ptr(key), _device.ptr(order), _device.ptr(links), _device.ptr(saddle),
            _device.ptr(pair), _device.ptr(row_links), _device.ptr(row_saddle), _device.ptr(count),
            _device.ptr(tmp_rows), tmp_rows.numel(), rt.stream()))
        rows = int(count[0])
        mark("reduce")
        # (copies: the rows do not keep the records' memory alive)
        return (pair[:rows].clone(), row_links[:rows].clone(),
                None if row_saddle is None else row_saddle[:rows].clone())

    def adjacency(self, radius, labels, voxel_value=None, voxel_class=None):
        """(pair int64 (E, 2), links int64 (E,), saddle fp64 (E,) or None): the region adjacency graph of a labelling
        of the voxels - which segments touch, over how many voxel edges, and how high the pass between them lies.
        the graph is that of components(): voxels u != v are neighbors when lists(voxels(), radius) names one for the
        other (the limit is inclusive) and both carry the same voxel_class >= 0 (None: one class for all).  labels
        (integers, (M,)): e.g. what components(), dbscan(), regions() or hill_climb() returned; a negative label is
        "in no segment"; labels must be below 2^31.  voxel_value (floating point, (M,), as in hill_climb): a voxel
        with a NaN value is out of the graph; None: no saddle is formed and the third result is None.
        one row for every unordered pair of distinct labels a < b that at least one edge {u, v} of the graph joins
        (label[u] = a, label[v] = b): links counts those edges, every undirected edge once; saddle is the largest
        min(value[u], value[v]) over them - the height of the pass between the two segments.  rows ascend by (a, b);
        no such pair: arrays of length 0.  no list of the voxel graph is written.  the result is a function of the
        arguments alone, the same bit for bit on every run."""
        self._need_index("adjacency")
        radius = float(radius)
        if not radius >= 0.0:
            raise ValueError("radius must be a number >= 0")
        label = self._voxel_integers(labels, "labels")
        value = None if voxel_value is None else self._voxel_heights(voxel_value, "voxel_value")
        cls = None if voxel_class is None else self._voxel_integers(voxel_class, "voxel_class")
        out = self._adjacency_device(radius, label, value, cls)
        return out if self._as_torch else tuple(None if t is None else t.cpu().numpy() for t in out)

    def _prominent_peaks_device(self, radius, value, mode, min_prominence, voxel_class, voxel_weight, min_size,
                                stages=None):
        """hill_climb, adjacency, the host merge (nm_merge_by_prominence) and the relabelling on device tensors:
        (labels (M,), sizes (C,), peaks (C,), prominence (C,)).  one copy of the rows and peak values to the host, one
        copy of the roots and prominences back"""
        rt = self._rt
        m = self.n_voxels
        mark = stages if stages is not None else (lambda name: None)
        labels0, sizes0, peaks0, _ = self._hill_climb_device(radius, value, mode, voxel_class, None, 1, False)
        mark("hill_climb")
        n_seg = int(peaks0.shape[0])
        if n_seg == 0:      # no voxel in the graph: every label is -1
            return labels0, sizes0, peaks0, torch.empty(0, dtype=torch.float64, device=rt.device)
        pair, _, saddle =self._adjacency_device(radius, labels0, value, voxel_class, stages)
        n_rows = int(pair.shape[0])
        # down in one piece: pair (2E int64), saddle (E fp64 as their bits), the peaks' values (S fp64 as their bits)
        packed = torch.cat((pair.reshape(-1), saddle.view(torch.int64), value[peaks0].view(torch.int64))).cpu().numpy()
        host_pair = np.ascontiguousarray(packed[:2 * n_rows])
        host_saddle = np.ascontiguousarray(packed[2 * n_rows:3 * n_rows]).view(np.float64)
        host_peak = np.ascontiguousarray(packed[3 * n_rows:]).view(np.float64)
        back = np.empty(2 * n_seg, dtype=np.int64)          # root, then the prominences as their bits
        host_root, host_prom = back[:n_seg], back[n_seg:].view(np.float64)
        scratch = np.empty(n_rows + n_seg + 1, dtype=np.int64)
        rc = rt.lib.nm_merge_by_prominence(n_seg, host_peak.ctypes.data, n_rows, host_pair.ctypes.data,
                                           host_saddle.ctypes.data, min_prominence, scratch.ctypes.data,
                                           host_root.ctypes.data, host_prom.ctypes.data)
        if rc:
            raise _ffi.NimrudHipError("nm_merge_by_prominence: status %d" % rc)
        mark("merge")
        back = torch.from_numpy(back).to(rt.device)
        root, prom = back[:n_seg], back[n_seg:].view(torch.float64)
        # sizes per root: integer sums, the same in any order
        inside = labels0 >= 0
        member_root = root[labels0.clamp(min=0)]
        size = torch.zeros(n_seg, dtype=torch.int64, device=rt.device)
        weight = torch.ones(m, dtype=torch.int64, device=rt.device) if voxel_weight is None else voxel_weight
        size.index_add_(0, member_root[inside], weight[inside])
        keep = (root == torch.arange(n_seg, device=rt.device)) & (size >= min_size)
        number = torch.cumsum(keep, 0) - 1
        labels = torch.where(inside & keep[member_root], number[member_root], torch.full_like(labels0, -1))
        mark("relabel")
        return labels, size[keep], peaks0[keep], prom[keep]

    def prominent_peaks(self, radius, voxel_value, min_prominence, link="highest", voxel_class=None,
                        voxel_weight=None, min_size=1):
        """(labels int64 (M,), sizes int64 (C,), peaks int64 (C,), prominence fp64 (C,)): hill_climb()'s segments with
        the peaks of low prominence merged into their higher neighbors - topological persistence.  hill_climb() makes
        a segment of every local maximum, one stray branch above a crown included; here a peak whose prominence, its
        value minus the saddle towards a higher neighbor, stays below min_prominence is given back to that neighbor.
        with link="highest" on height: crown delineation that survives noise; with link="nearest" on dbscan()'s
        density: ToMATo on quick shift.
          1. hill_climb(radius, voxel_value, link, voxel_class) gives segments 0..S-1 with peak values p; segment a
             is HIGHER than b when p[a] > p[b], or they are equal and a < b.
          2. adjacency(radius, labels, voxel_value, voxel_class) gives the highest saddle between touching segments.
          3. the rows are taken by descending saddle, equal saddles by ascending (a, b), through a union-find: of the
             two roots the lower, lo, is merged under the higher when p[lo] - saddle < min_prominence (fp64, strict);
             otherwise nothing is merged and lo's prominence, if none is recorded yet, is p[lo] - saddle.  a root that
             never loses has prominence +inf.
          4. the surviving roots are the segments: a segment's size is the sum of voxel_weight (None: voxels) over
             its members, segments below min_size are dropped (-1), the others numbered 0..C-1 by ascending peak
             position; peaks[c] is the root's peak, prominence[c] its prominence.
        min_prominence is a number >= 0, may be inf.  0 merges nothing: labels, sizes and peaks are hill_climb()'s.
        inf merges every connected piece of the class graph into its highest peak.  min_size acts AFTER the merge: a
        small peak merged into a large one lives on inside it.  the result is a function of the arguments alone."""
        self._need_index("prominent_peaks")
        radius = float(radius)
        if not radius >= 0.0:
            raise ValueError("radius must be a number >= 0")
        min_prominence = _min_prominence(min_prominence)
        if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)):
            raise ValueError("min_size must be an integer")
        if link not in _ffi.NM_CLIMB:
            raise ValueError("link must be 'highest' or 'nearest'")
        value = self._voxel_heights(voxel_value, "voxel_value")
        cls = None if voxel_class is None else self._voxel_integers(voxel_class, "voxel_class")
        weight = None if voxel_weight is None else self._voxel_integers(voxel_weight, "voxel_weight")
        out = self._prominent_peaks_device(radius, value, _ffi.NM_CLIMB[link], min_prominence, cls, weight,
                                           int(min_size))
        return out if self._as_torch else tuple(t.cpu().numpy() for t in out)

    def component_table(self, labels, voxel_weight=None):
        """fp64 (C, 25): segment_table over voxels() for the labels components() returned - one row of descriptors
        per component of the voxel graph (columns: SEGMENT_COLUMNS).  voxels with label -1 are in no segment.
        voxel_weight (integers, (M,), e.g. point_counts()): frequency weights, so that column 0 is the component's
        size in points; None counts voxels.  C is labels.max() + 1 (one host read).  follows the search cloud:
        torch in, torch out; numpy in, numpy out."""
        self._need_index("component_table")
        rt = self._rt
        label = self._voxel_integers(labels, "labels")
        weight = None if voxel_weight is None else self._voxel_integers(voxel_weight, "voxel_weight")
        centres = self.filter.address_to_coordinate(self._addresses_device())
        table = _segment_table_device(rt, centres, label, weight, None)
        return table if self._as_torch else table.cpu().numpy()


def _min_cos(max_angle):
    """the cosine regions() compares fabs(dot) with: cos(max_angle), and 0 from a right angle on - unsigned directions
    are never further apart, but the float pi/2 lies below the real one and its cosine, 6e-17, would still cut normals
    that are perpendicular exactly"""
    return math.cos(max_angle) if max_angle < math.pi / 2 else 0.0


def _min_prominence(min_prominence):
    """the threshold of prominent_peaks as a float: a number >= 0, inf included"""
    try:
        tau = float(min_prominence)
    except (TypeError, ValueError):
        raise ValueError("min_prominence must be a number >= 0")
    if not tau >= 0.0:      # (NaN fails)
        raise ValueError("min_prominence must be a number >= 0")
    return tau


def _integer_column(values, n, device, what, per):
    """an integer array (n,) - torch or numpy, any integer width - as a contiguous int64 tensor on `device`"""
    if isinstance(values, torch.Tensor):
        integral = values.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
        t = values
    else:
        arr = np.asarray(values)
        integral = arr.dtype.kind in "iu"
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64)) if integral else None
    if not integral:
        raise ValueError("%s must have an integer dtype" % what)
    if t.ndim != 1 or t.shape[0] != n:
        raise ValueError("%s must have one entry per %s" % (what, per))
    return t.to(device=device, dtype=torch.int64).contiguous()


def _unit_columns(table):
    """the table itself where its rows can be walked with a row stride, else a contiguous copy"""
    if table.shape[0] > 1 and (table.stride(1) != 1 or table.stride(0) < table.shape[1]):
        return table.contiguous()
    return table if table.shape[0] > 1 else table.contiguous()


def neighbor_lists(query_cloud, search_cloud, edge_length, radius, method="auto"):
    """the neighbor index lists of multiscale.py:103 as CSR (offsets int64[Nq+1], index int64[total]):
    for every query point the ascending positions, in the sorted unique voxel array of
    VoxelFilter.unique_voxels(search_cloud), of the voxels within `radius`.
    one NeighborIndex, built and asked once - keep the handle yourself to ask again with another radius or
    query cloud.  method "auto" reads the lists off the occupancy index and its rank table wherever the
    lattice is in that path's range (every scale of the benchmark configurations) and searches the sorted
    addresses otherwise; "search" forces the address search (the parity mode of earlier versions, some
    hundred times slower per point-scale than the fused feature path); "index" raises ValueError when the
    lattice is out of range.  the results are identical."""
    return NeighborIndex(search_cloud, edge_length, method=method).lists(query_cloud, radius)


def nearest_voxels(query_cloud, search_cloud, edge_length, k, max_distance=None):
    """(distance fp64 (Nq, k), index int64 (Nq, k)): the k nearest voxels of VoxelFilter.unique_voxels(
    search_cloud) for every query point, what cKDTree(search_voxels).query(query_cloud, k) gives on the tree of
    multiscale.py:87 - see NeighborIndex.nearest for order, ties, limit and padding.  one NeighborIndex (method
    "index"), built and asked once - keep the handle yourself to ask again."""
    return NeighborIndex(search_cloud, edge_length, method="index").nearest(query_cloud, k, max_distance)


def cluster_cloud(cloud, edge_length, radius, point_class=None, min_points=1):
    """(point_labels int64 (N,), sizes int64 (C,)): Euclidean cluster extraction of a cloud in one call.  the cloud
    is voxel-filtered at `edge_length`, voxels whose centres lie within `radius` of each other are joined
    (NeighborIndex.components), and every point takes the label of its voxel.  sizes and min_points count POINTS
    (the voxels are weighted by point_counts()): clusters of fewer points are dropped, their points get -1.
    clusters are numbered 0..C-1 in ascending order of their smallest voxel position.
    point_class (integers, (N,), e.g. classify_cloud's labels; magnitudes below 2^53): only voxels of equal class
    are joined.  a voxel's class is the MINIMUM class of the points in it, so a voxel with one point of a negative
    class is out of the graph with all its points.
    one NeighborIndex (method "index"), built and asked once.  torch in, torch out; numpy in, numpy out."""
    index = NeighborIndex(cloud, edge_length, method="index")
    rt = index._rt
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)):
        raise ValueError("min_points must be an integer")
    radius = float(radius)
    if not radius >= 0.0:
        raise ValueError("radius must be a number >= 0")
    voxel_class = None
    if point_class is not None:
        column = _integer_column(point_class, index._search.shape[0], rt.device, "point_class", "point")
        # min of an integer-valued fp64 column: exact
        voxel_class = index.voxel_table(column.to(torch.float64), reduce="min")[:, 0].to(torch.int64)
    weight = index._grouping()[0]
    labels, sizes = index._components_device(radius, voxel_class, weight, int(min_points))
    voxel = index._voxel_of_device(index._search)
    point_labels = torch.where(voxel >= 0, labels[voxel.clamp(min=0)], torch.full_like(voxel, -1))
    if isinstance(cloud, torch.Tensor):
        return point_labels, sizes
    return point_labels.cpu().numpy(), sizes.cpu().numpy()


def dbscan_cloud(cloud, edge_length, radius, min_points, point_class=None, min_cluster_points=1):
    """(point_labels int64 (N,), sizes int64 (C,), point_core bool (N,)): DBSCAN of a cloud in one call, on its voxels.
    the cloud is voxel-filtered at `edge_length`, every voxel is weighted by the points in it (point_counts()), and
    NeighborIndex.dbscan clusters the voxels: a voxel is core where the voxels within `radius` of its centre, itself
    included, hold at least `min_points` POINTS.  every point takes the label and the core flag of its voxel.  sizes
    and min_cluster_points count points too: clusters of fewer points are dropped, their points get -1.  clusters are
    numbered 0..C-1 in ascending order of their smallest core voxel position.
    point_class (integers, (N,); magnitudes below 2^53): a voxel's class is the MINIMUM class of the points in it, as
    in cluster_cloud; density and links stay within a class, a negative class is out.
    one NeighborIndex (method "index"), built and asked once.  torch in, torch out; numpy in, numpy out."""
    index = NeighborIndex(cloud, edge_length, method="index")
    rt = index._rt
    for name, value in (("min_points", min_points), ("min_cluster_points", min_cluster_points)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            raise ValueError("%s must be an integer" % name)
    radius = float(radius)
    if not radius >= 0.0:
        raise ValueError("radius must be a number >= 0")
    voxel_class = None
    if point_class is not None:
        column = _integer_column(point_class, index._search.shape[0], rt.device, "point_class", "point")
        # min of an integer-valued fp64 column: exact
        voxel_class = index.voxel_table(column.to(torch.float64), reduce="min")[:, 0].to(torch.int64)
    weight = index._grouping()[0]
    labels, sizes, core, _ = index._dbscan_device(radius, int(min_points), voxel_class, weight,
                                                  int(min_cluster_points), False)
    voxel = index._voxel_of_device(index._search)
    inside = voxel >= 0
    at = voxel.clamp(min=0)
    point_labels = torch.where(inside, labels[at], torch.full_like(voxel, -1))
    point_core = inside & core[at]
    if isinstance(cloud, torch.Tensor):
        return point_labels, sizes, point_core
    return point_labels.cpu().numpy(), sizes.cpu().numpy(), point_core.cpu().numpy()


def voxel_normals(index, radius, max_curvature=None):
    """(normals fp64 (M, 3), seed bool (M,)) on the device: what smooth_regions hands to NeighborIndex.regions.  the
    normal of a voxel is process_gpu_normals' at its centre over the handle's own search cloud, one scale at the
    handle's edge length and `radius`; its surface variation is 1 - (f[:, 2] + f[:, 3]) of the same call's features,
    the smallest eigenvalue's share of the sum.  a voxel is a seed where the normal is not zero (three voxels or more
    in reach) and, with max_curvature given, where the variation is <= max_curvature."""
    index._need_index("voxel_normals")
    centres = index.filter.address_to_coordinate(index._addresses_device())
    edge = float(index.filter.edge_length)
    features, normals = process_gpu_normals(centres, index._search, [edge], [float(radius)])
    seed = (normals != 0.0).any(dim=1)
    if max_curvature is not None:
        seed = seed & ((1.0 - (features[:, 2] + features[:, 3])) <= float(max_curvature))
    return normals, seed


def smooth_regions(cloud, edge_length, radius, max_angle, normal_radius=None, max_curvature=None, point_class=None,
                   min_points=1):
    """(point_labels int64 (N,), sizes int64 (C,), table fp64 (C, 25)): the smooth surfaces of a cloud in one call -
    planes and gently curved faces come out as regions of their own where cluster_cloud and dbscan_cloud see one blob.
    the cloud is voxel-filtered at `edge_length`; every voxel gets a normal and a surface variation from the voxels
    within `normal_radius` (None: `radius`) of its centre (voxel_normals); voxels with a normal - and, with
    max_curvature given, a variation <= max_curvature - are seeds; NeighborIndex.regions links neighboring seeds
    whose normals differ by at most `max_angle` radians, and hangs every other voxel (a crease, an edge) onto its
    nearest seed neighbor.  every point takes the label of its voxel.  sizes and min_points count POINTS; regions of
    fewer points are dropped, their points get -1.  table is segment_table over the points (SEGMENT_COLUMNS): its
    normal column is the fitted normal of each region, table[:, 0] == sizes.  point_class as in cluster_cloud.
    one NeighborIndex (method "index"); the cloud is uploaded once.  torch in, torch out; numpy in, numpy out."""
    rt, points = _device.as_cloud(cloud)
    index = NeighborIndex(points, edge_length, method="index")
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)):
        raise ValueError("min_points must be an integer")
    radius = float(radius)
    if not radius >= 0.0:
        raise ValueError("radius must be a number >= 0")
    normal_radius = radius if normal_radius is None else float(normal_radius)
    if not normal_radius >= 0.0:
        raise ValueError("normal_radius must be a number >= 0")
    max_angle = float(max_angle)
    if max_angle != max_angle:
        raise ValueError("max_angle must be a number (radians)")
    if max_curvature is not None and not float(max_curvature) >= 0.0:
        raise ValueError("max_curvature must be a number >= 0")
    voxel_class = None
    if point_class is not None:
        column = _integer_column(point_class, points.shape[0], rt.device, "point_class", "point")
        # min of an integer-valued fp64 column: exact
        voxel_class = index.voxel_table(column.to(torch.float64), reduce="min")[:, 0].to(torch.int64)
    weight = index._grouping()[0]
    normals, seed = voxel_normals(index, normal_radius, max_curvature)
    labels, sizes, _ = index._regions_device(radius, normals, _min_cos(max_angle), None, (), seed.to(torch.uint8),
                                             voxel_class, weight, int(min_points))
    voxel = index._voxel_of_device(points)
    point_labels = torch.where(voxel >= 0, labels[voxel.clamp(min=0)], torch.full_like(voxel, -1))
    table = _segment_table_device(rt, points, point_labels, None, int(sizes.shape[0]))
    if isinstance(cloud, torch.Tensor):
        return point_labels, sizes, table
    return point_labels.cpu().numpy(), sizes.cpu().numpy(), table.cpu().numpy()


def peak_segments(cloud, edge_length, radius, point_value=None, link="highest", point_class=None, min_points=1):
    """(point_labels int64 (N,), sizes int64 (C,), peak_xyz fp64 (C, 3), peak_value fp64 (C,)): the peak-seeking
    segments of a cloud in one call - individual tree crowns with the height as the value, the modes of a density.
    the cloud is voxel-filtered at `edge_length`; a voxel's value is the MAXIMUM of point_value (floating point, (N,);
    None: the z column) over its points; NeighborIndex.hill_climb lets every voxel step to a higher voxel within
    `radius` (link "highest" or "nearest", see there) and a segment is what climbs to the same peak.  every point
    takes the label of its voxel.  sizes and min_points count POINTS (the voxels are weighted by point_counts()):
    segments of fewer points are dropped, their points get -1.  segments are numbered 0..C-1 in ascending order of
    their peak's voxel position; peak_xyz are the centres of the peak voxels, peak_value their values.
    point_class as in cluster_cloud: a voxel's class is the MINIMUM class of the points in it, links stay within a
    class, a negative class is out.  NaN point values are not supported (as in voxel_table).
    one NeighborIndex (method "index"), built and asked once.  torch in, torch out; numpy in, numpy out."""
    index = NeighborIndex(cloud, edge_length, method="index")
    rt = index._rt
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)):
        raise ValueError("min_points must be an integer")
    radius = float(radius)
    if not radius >= 0.0:
        raise ValueError("radius must be a number >= 0")
    if link not in _ffi.NM_CLIMB:
        raise ValueError("link must be 'highest' or 'nearest'")
    n = index._search.shape[0]
    if point_value is None:
        column = index._search[:, 2]
    else:
        column = torch.as_tensor(point_value)
        if not column.dtype.is_floating_point:
            raise ValueError("point_value must have a floating-point dtype")
        if column.ndim != 1 or column.shape[0] != n:
            raise ValueError("point_value must have one entry per point")
        column = column.to(device=rt.device, dtype=torch.float64)
    value = index.voxel_table(column, reduce="max")[:, 0].contiguous()
    voxel_class = None
    if point_class is not None:
        classes = _integer_column(point_class, n, rt.device, "point_class", "point")
        # min of an integer-valued fp64 column: exact
        voxel_class = index.voxel_table(classes.to(torch.float64), reduce="min")[:, 0].to(torch.int64)
    weight = index._grouping()[0]
    labels, sizes, peaks, _ = index._hill_climb_device(radius, value, _ffi.NM_CLIMB[link], voxel_class, weight,
                                                       int(min_points), False)
    voxel = index._voxel_of_device(index._search)
    point_labels = torch.where(voxel >= 0, labels[voxel.clamp(min=0)], torch.full_like(voxel, -1))
    peak_xyz = index.filter.address_to_coordinate(index._addresses_device())[peaks]
    peak_value = value[peaks]
    out = (point_labels, sizes, peak_xyz, peak_value)
    return out if isinstance(cloud, torch.Tensor) else tuple(t.cpu().numpy() for t in out)


def prominent_segments(cloud, edge_length, radius, min_prominence, point_value=None, link="highest", point_class=None,
                       min_points=1):
    """(point_labels int64 (N,), sizes int64 (C,), peak_xyz fp64 (C, 3), peak_value fp64 (C,), prominence fp64 (C,)):
    peak_segments with the peaks of low prominence merged into their higher neighbors
    (NeighborIndex.prominent_peaks): crowns that survive a stray branch, density modes that survive a noisy bin.
    the cloud is voxel-filtered at `edge_length`; a voxel's value is the MAXIMUM of point_value (floating point, (N,);
    None: the z column) over its points, its class the MINIMUM of point_class; a peak whose value minus the saddle
    towards a higher neighboring segment is below min_prominence (a number >= 0, may be inf) goes to that neighbor.
    every point takes the label of its voxel.  sizes and min_points count POINTS (the voxels are weighted by
    point_counts()) and act after the merge.  segments are numbered 0..C-1 in ascending order of their peak's voxel
    position; peak_xyz are the centres of the peak voxels, peak_value their values, prominence what
    prominent_peaks reports (+inf for the highest peak of a connected piece).
    one NeighborIndex (method "index"), built and asked once.  torch in, torch out; numpy in, numpy out."""
    index = NeighborIndex(cloud, edge_length, method="index")
    rt = index._rt
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)):
        raise ValueError("min_points must be an integer")
    radius = float(radius)
    if not radius >= 0.0:
        raise ValueError("radius must be a number >= 0")
    min_prominence = _min_prominence(min_prominence)
    if link not in _ffi.NM_CLIMB:
        raise ValueError("link must be 'highest' or 'nearest'")
    n = index._search.shape[0]
    if point_value is None:
        column = index._search[:, 2]
    else:
        column = torch.as_tensor(point_value)
        if not column.dtype.is_floating_point:
            raise ValueError("point_value must have a floating-point dtype")
        if column.ndim != 1 or column.shape[0] != n:
            raise ValueError("point_value must have one entry per point")
        column = column.to(device=rt.device, dtype=torch.float64)
    value = index.voxel_table(column, reduce="max")[:, 0].contiguous()
    voxel_class = None
    if point_class is not None:
        classes = _integer_column(point_class, n, rt.device, "point_class", "point")
        # min of an integer-valued fp64 column: exact
        voxel_class = index.voxel_table(classes.to(torch.float64), reduce="min")[:, 0].to(torch.int64)
    weight = index._grouping()[0]
    labels, sizes, peaks, prominence = index._prominent_peaks_device(
        radius, value, _ffi.NM_CLIMB[link], min_prominence, voxel_class, weight, int(min_points))
    voxel = index._voxel_of_device(index._search)
    point_labels = torch.where(voxel >= 0, labels[voxel.clamp(min=0)], torch.full_like(voxel, -1))
    peak_xyz = index.filter.address_to_coordinate(index._addresses_device())[peaks]
    peak_value = value[peaks]
    out = (point_labels, sizes, peak_xyz, peak_value, prominence)
    return out if isinstance(cloud, torch.Tensor) else tuple(t.cpu().numpy() for t in out)


def geodesic_segments(cloud, edge_length, radius, point_seed, max_distance=None, point_class=None, min_points=1):
    """(point_distance fp64 (N,), point_labels int64 (N,), sizes int64 (C,), source_xyz fp64 (C, 3)): segments grown
    from seed points along the object, in one call - individual trees from their stems where the crowns interlock,
    the distance along a wall or a cable from a marked start.  the cloud is voxel-filtered at `edge_length`; a voxel
    is a seed if ANY of its points has a non-zero point_seed (bool or integers, (N,)); NeighborIndex.geodesic gives
    every voxel the length of its shortest path from a seed through the voxels within `radius` of each other (not
    beyond max_distance, see there) and the seed that path starts from.  every point takes the distance and the label
    of its voxel: +inf and -1 where no path reaches.  sizes and min_points count POINTS (the voxels are weighted by
    point_counts()): segments of fewer points are dropped, their points get -1 and keep their distance.  segments are
    numbered 0..C-1 in ascending order of their seed's voxel position; source_xyz are the centres of the seed voxels.
    point_class as in cluster_cloud: a voxel's class is the MINIMUM class of the points in it, paths stay within a
    class, a negative class is out.
    one NeighborIndex (method "index"), built once; the call synchronises once per batch of sweeps, as geodesic does.
    torch in, torch out; numpy in, numpy out."""
    index = NeighborIndex(cloud, edge_length, method="index")
    rt = index._rt
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)):
        raise ValueError("min_points must be an integer")
    radius = float(radius)
    if not radius >= 0.0:
        raise ValueError("radius must be a number >= 0")
    max_distance = float("inf") if max_distance is None else float(max_distance)
    if not max_distance >= 0.0:
        raise ValueError("max_distance must be a number >= 0, or None")
    n = index._search.shape[0]
    if isinstance(point_seed, torch.Tensor) and point_seed.dtype == torch.bool:
        point_seed = point_seed.to(torch.uint8)
    elif not isinstance(point_seed, torch.Tensor) and np.asarray(point_seed).dtype == np.bool_:
        point_seed = np.asarray(point_seed).astype(np.uint8)
    marks = (_integer_column(point_seed, n, rt.device, "point_seed", "point") != 0).to(torch.float64)
    # max of a 0 / 1 fp64 column: exact
    seed = (index.voxel_table(marks, reduce="max")[:, 0] != 0.0).to(torch.uint8)
    voxel_class = None
    if point_class is not None:
        classes = _integer_column(point_class, n, rt.device, "point_class", "point")
        # min of an integer-valued fp64 column: exact
        voxel_class = index.voxel_table(classes.to(torch.float64), reduce="min")[:, 0].to(torch.int64)
    weight = index._grouping()[0]
    dist, labels, sizes, sources, _ = index._geodesic_device(radius, seed, max_distance, voxel_class, weight,
                                                             int(min_points), False)
    voxel = index._voxel_of_device(index._search)
    at = voxel.clamp(min=0)
    point_labels = torch.where(voxel >= 0, labels[at], torch.full_like(voxel, -1))
    point_distance = torch.where(voxel >= 0, dist[at], torch.full_like(dist[at], float("inf")))
    source_xyz = index.filter.address_to_coordinate(index._addresses_device())[sources]
    out = (point_distance, point_labels, sizes, source_xyz)
    return out if isinstance(cloud, torch.Tensor) else tuple(t.cpu().numpy() for t in out)


# columns of a segment table (nm_segment_table): name -> slice
SEGMENT_COLUMNS = {
    "n": slice(0, 1),
    "centroid": slice(1, 4),
    "min": slice(4, 7),
    "max": slice(7, 10),
    "covariance": slice(10, 16),        # [xx, xy, xz, yy, yz, zz], ddof = 1
    "eigenvalues": slice(16, 19),       # descending
    "normal": slice(19, 22),            # unit eigenvector of the smallest eigenvalue
    "axis": slice(22, 25),              # unit eigenvector of the largest eigenvalue
}


def _segment_table_device(rt, points, label, weight, n_segments):
    """enqueue nm_segment_table on device tensors: points fp64 (N, >= 3), label int64 (N,), weight int64 (N,) or
    None -> fp64 (C, 25).  n_segments None: label.max() + 1, one host read (0 without rows or labels)."""
    n = int(points.shape[0])
    if n_segments is None:
        n_segments = int(label.max()) + 1 if n else 0
        n_segments = max(n_segments, 0)
    elif isinstance(n_segments, bool) or not isinstance(n_segments, (int, np.integer)) or n_segments < 0:
        raise ValueError("n_segments must be an integer >= 0")
    c = int(n_segments)
    table = torch.empty((c, _ffi.NM_SEGMENT_COLUMNS), dtype=torch.float64, device=rt.device)
    if c == 0:
        return table
    nbytes = int(rt.lib.nm_segment_table_workspace_bytes(n, c))
    if nbytes == 0:
        raise ValueError("segment_table: sizes must be below 2^31")
    tmp = rt.workspace(nbytes)
    rt.check(rt.lib.nm_segment_table(
        rt.ctx, _device.ptr(points), n, _device.row_stride(points), _device.ptr(label), c, _device.ptr(weight),
        _device.ptr(table), _ffi.NM_SEGMENT_COLUMNS, _device.ptr(tmp), tmp.numel(), rt.stream()))
    return table


def segment_table(cloud, labels, weights=None, n_segments=None):
    """fp64 (C, 25): one row of descriptors per segment of a labelled cloud (nm_segment_table; columns:
    SEGMENT_COLUMNS) - n, centroid, bounding box, ddof=1 covariance, its eigenvalues (descending), the normal (unit
    eigenvector of the smallest) and the axis (of the largest), both with their last non-zero component positive.
    labels (integers, (N,)): a value in [0, C) names the point's segment; -1 or anything else is no segment.
    weights (integers >= 0, (N,)): frequency weights as np.cov(fweights=), e.g. point counts of voxel centres; a row of
    weight 0 counts for nothing.  n_segments: C; None takes labels.max() + 1 (one host read).
    empty segments are zeros; with n < 2 the covariance and all behind it, with fewer than 3 rows the vectors.  the
    moments are taken about the segment's box minimum, so georeferenced coordinates keep their digits; the summation
    order is a function of the segment's own ascending rows, the same bit for bit on every run, whatever else the
    cloud holds.  a ForestModel takes the table as it is.  torch in, torch out; numpy in, numpy out."""
    rt, points = _device.as_cloud(cloud)
    if points.shape[1] < 3:
        raise ValueError("only 3D spaces supported by the multiscale pipeline")
    n = int(points.shape[0])
    label = _integer_column(labels, n, rt.device, "labels", "point")
    weight = None if weights is None else _integer_column(weights, n, rt.device, "weights", "point")
    table = _segment_table_device(rt, points, label, weight, n_segments)
    return table if isinstance(cloud, torch.Tensor) else table.cpu().numpy()


def cluster_features(cloud, edge_length, radius, point_class=None, min_points=1):
    """(point_labels int64 (N,), sizes int64 (C,), table fp64 (C, 25)): cluster_cloud followed by segment_table over
    the points - every cluster with its descriptors, table[:, 0] == sizes.  arguments as cluster_cloud; the cloud is
    uploaded once.  torch in, torch out; numpy in, numpy out."""
    rt, points = _device.as_cloud(cloud)
    point_labels, sizes = cluster_cloud(points, edge_length, radius, point_class=point_class, min_points=min_points)
    table = _segment_table_device(rt, points, point_labels, None, int(sizes.shape[0]))
    if isinstance(cloud, torch.Tensor):
        return point_labels, sizes, table
    return point_labels.cpu().numpy(), sizes.cpu().numpy(), table.cpu().numpy()
