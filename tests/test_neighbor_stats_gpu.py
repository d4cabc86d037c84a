"""
GPU tests of the attribute operators on multiscale.NeighborIndex (nm_neighbors.hip: k_nbr_voxel_of, the grouping
kernels, k_nbr_voxel_reduce, k_nbr_stats) and of fields.vector_field_stats.  the oracle for the point -> voxel
map, the counts and the voxel tables is numpy on oracle.Lattice addresses (np.unique with return_inverse,
np.bincount, np.minimum.at / np.maximum.at); for the neighborhood statistics it is a plain left-to-right loop
over the handle's own lists.  every comparison is exact except where two differently rounded paths meet
(vector_field_stats against vector_field_mean and the oracle's field mean: the existing field test's bound).
"""

import ctypes

import numpy as np
import pytest
import torch

from nimrud_amd import _ffi, synth
from nimrud_amd import device as _device
from nimrud_amd.minimal import fields, multiscale
from oracle import nimrud_oracle as oracle

pytestmark = pytest.mark.gpu

SCAN_TILE = 4096          # voxels one block of the start scan takes per round (NBR_SCAN_TILE, nm_neighbors.hip)
SHORT = 64                # a segment up to here is ordered by one thread (GRP_SHORT)
LDS_ROWS = 8192           # a longer one by a block, in LDS up to here (GRP_LDS_ROWS), in memory beyond


def uniform_box(n, extent, seed, origin=(0.0, 0.0, 0.0)):
    rs = np.random.RandomState(seed)
    return rs.rand(n, 3) * np.asarray(extent, dtype=np.float64) + np.asarray(origin, dtype=np.float64)


def inverse_of(pts, edge):
    """(sorted distinct addresses, np.unique's inverse) of a cloud on its own lattice"""
    unique, inverse = np.unique(oracle.Lattice(pts, edge).coordinate_to_address(pts), return_inverse=True)
    return unique, inverse.reshape(-1)


def voxel_of_oracle(search, edge, points):
    """the voxel of arbitrary points on the lattice of `search`: the reference's cell arithmetic
    (geometry.py:108-115) without its bounds check, -1 outside the 2^w cells of an axis or in an empty cell"""
    lat = oracle.Lattice(search, edge)
    unique = lat.unique_addresses(search)
    cells = np.floor((points - lat.minimum_corner) / edge)
    inside = np.all((cells >= 0) & (cells < 2.0 ** lat.widths), axis=1)
    c = np.where(inside[:, None], cells, 0).astype(np.int64)
    addr = c[:, 0] + (c[:, 1] << lat.shifts[0]) + (c[:, 2] << lat.shifts[1])
    at = np.minimum(np.searchsorted(unique, addr), len(unique) - 1)
    return np.where(inside & (unique[at] == addr), at, -1), inside


@pytest.fixture(scope="module")
def scene():
    """the cloud, query set and attribute columns of test_gpu_parity.py's field test, the columns repeated with
    other weights up to 16"""
    rs = np.random.RandomState(939)
    pts, labels = synth.scene_cloud(6000, extent=8.0, n_poles=5, n_spheres=2, seed=938)
    extra = rs.rand(300, 3) * 10.0 - 1.0
    attr = np.stack([np.sin(pts[:, 0]), pts[:, 2] ** 2, labels.astype(np.float64),
                     np.full(len(pts), 3.25), rs.rand(len(pts))], axis=1)
    more = [attr[:, c % 5] * (c + 0.5) - rs.rand(len(pts)) for c in range(5, 16)]
    attr16 = np.ascontiguousarray(np.concatenate((attr, np.stack(more, axis=1)), axis=1))
    return {"pts": pts, "extra": extra, "attr": attr, "attr16": attr16,
            "index": {e: multiscale.NeighborIndex(pts, e) for e in (0.1, 0.25)}}


# ---- voxel_of --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", [0.1, 0.25])
def test_voxel_of_is_the_unique_inverse(scene, edge):
    pts, ix = scene["pts"], scene["index"][edge]
    assert ix.method == "index"
    unique, inverse = inverse_of(pts, edge)
    got = ix.voxel_of(pts)
    assert got.dtype == np.int64 and got.shape == (len(pts),)
    assert np.array_equal(got, inverse)
    assert np.array_equal(ix.addresses()[got], unique[inverse])
    # a row-permuted copy (another array: it is uploaded and walked on its own)
    perm = np.random.RandomState(5).permutation(len(pts))
    assert np.array_equal(ix.voxel_of(pts[perm]), inverse[perm])
    # torch in, torch out
    dev = torch.from_numpy(pts).cuda()
    got = multiscale.NeighborIndex(dev, edge).voxel_of(dev[:100])
    assert isinstance(got, torch.Tensor) and np.array_equal(got.cpu().numpy(), inverse[:100])


@pytest.mark.parametrize("edge", [0.1, 0.25])
def test_voxel_of_is_minus_one_outside_the_lattice_and_in_empty_cells(scene, edge):
    pts, ix = scene["pts"], scene["index"][edge]
    lo, hi = pts.min(0), pts.max(0)
    span = edge * 2.0 ** np.asarray(ix.filter.widths, dtype=np.float64)       # the lattice, not the cloud's box
    other = uniform_box(4000, span + 4.0, seed=23, origin=lo - 2.0)
    other = np.vstack((other, uniform_box(2000, hi - lo, seed=24, origin=lo), pts[:300],
                       [[1e9, 0.0, 0.0], [0.0, -1e300, 0.0]]))
    want, inside = voxel_of_oracle(pts, edge, other)
    cells = np.floor((other - (lo - edge / 2)) / edge)
    for a in range(3):                     # beyond every face
        assert (cells[:, a] < 0).any() and (cells[:, a] >= 2.0 ** int(ix.filter.widths[a])).any()
    assert (inside & (want < 0)).sum() > 500 and (want >= 0).sum() >= 300
    assert np.array_equal(ix.voxel_of(other), want)


def test_voxel_of_on_a_lattice_narrower_than_one_leaf_and_a_long_thin_one():
    narrow = uniform_box(300, (10.0, 5.0, 5.0), seed=15)
    thin = uniform_box(5000, (1.0e6, 6.0, 6.0), seed=14)
    thin[:2500, 0] = thin[:2500, 0] % 300.0
    for pts, widths in ((narrow, None), (thin, [20, 3, 3])):
        ix = multiscale.NeighborIndex(pts, 1.0)
        assert ix.method == "index"
        if widths:
            assert [int(w) for w in ix.filter.widths] == widths
        else:
            assert int(ix.filter.widths[0]) < 5
        assert np.array_equal(ix.voxel_of(pts), inverse_of(pts, 1.0)[1])


# ---- point_counts / members ------------------------------------------------------------------------------------

def crowded_cloud():
    """e = 1: voxels with 9000, 3000, 65, 64 and 63 points and 400 with one, rows shuffled - both sides of the
    switch between the one-thread and the block ordering, and of the block ordering's switch out of LDS"""
    rs = np.random.RandomState(31)
    cells = rs.permutation(20 * 20 * 10)[:405]
    cells = np.stack((cells % 20, (cells // 20) % 20, cells // 400), axis=1).astype(np.float64)
    sizes = [LDS_ROWS + 808, 3000, SHORT + 1, SHORT, SHORT - 1] + [1] * 400
    # (the lattice starts half an edge below the lowest point: a cluster this tight stays in one of its cells)
    pts = np.repeat(cells, sizes, axis=0) + 0.25 + 0.1 * rs.rand(sum(sizes), 3)
    return pts[rs.permutation(len(pts))], sorted(sizes)


def check_grouping(pts, edge):
    _, inverse = inverse_of(pts, edge)
    ix = multiscale.NeighborIndex(pts, edge)
    counts = ix.point_counts()
    start, rows = ix.members()
    want_counts = np.bincount(inverse)
    assert counts.dtype == np.int64 and start.dtype == np.int64 and rows.dtype == np.int64
    assert ix.n_voxels == len(want_counts)
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(start, np.concatenate(([0], np.cumsum(want_counts))))
    assert np.array_equal(rows, np.argsort(inverse, kind="stable"))
    # again on the same handle, and from a fresh build
    again = ix.members()
    fresh = multiscale.NeighborIndex(pts, edge).members()
    for other in (again, fresh):
        assert np.array_equal(other[0], start) and np.array_equal(other[1], rows)
    return want_counts


def test_grouping_with_a_scan_across_tiles():
    pts = synth.uniform_cloud(70000, extent=10.0, seed=41)
    counts = check_grouping(pts, 0.25)
    assert len(counts) > 2 * SCAN_TILE


def test_grouping_with_short_and_long_segments():
    pts, sizes = crowded_cloud()
    counts = check_grouping(pts, 1.0)
    assert sorted(counts.tolist()) == sizes
    assert counts.max() > LDS_ROWS and SHORT < 3000 <= LDS_ROWS


def test_grouping_another_cloud_leaves_rows_of_no_voxel_out():
    """the C entry point on a cloud that is not the search cloud: voxel numbers -1, more voxels than rows"""
    rt = _device.get_runtime()
    rs = np.random.RandomState(43)
    m, n = 5000, 3000
    voxel = rs.randint(-1, 40, size=n).astype(np.int64)            # 40 voxels in use, some rows in none
    voxel[rs.rand(n) < 0.3] = m - 1 - rs.randint(0, 5)
    d_voxel = torch.from_numpy(voxel).to(rt.device)
    counts = torch.full((m,), -7, dtype=torch.int64, device=rt.device)
    start = torch.full((m + 1,), -7, dtype=torch.int64, device=rt.device)
    rows = torch.full((n,), -7, dtype=torch.int64, device=rt.device)
    nbytes = rt.lib.nm_neighbor_index_group_workspace_bytes(m)
    tmp = torch.empty(nbytes, dtype=torch.uint8, device=rt.device)
    args = (rt.ctx, _device.ptr(d_voxel), n, m, _device.ptr(counts), _device.ptr(start), _device.ptr(rows))
    rt.check(rt.lib.nm_neighbor_index_group(*args, _device.ptr(tmp), nbytes, rt.stream()))
    kept = voxel >= 0
    want_counts = np.bincount(voxel[kept], minlength=m)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert np.array_equal(start.cpu().numpy(), np.concatenate(([0], np.cumsum(want_counts))))
    total = int(kept.sum())
    want_rows = np.flatnonzero(kept)[np.argsort(voxel[kept], kind="stable")]
    assert np.array_equal(rows.cpu().numpy()[:total], want_rows)
    assert np.all(rows.cpu().numpy()[total:] == -7)                 # nothing behind the last segment is touched
    # too small a workspace is refused before anything is launched
    small = rt.lib.nm_neighbor_index_group_workspace_bytes(n)
    assert small < nbytes
    assert rt.lib.nm_neighbor_index_group(*args, _device.ptr(tmp), small, rt.stream()) == _ffi.NM_ERR_WORKSPACE
    assert rt.lib.nm_neighbor_index_group(*args[:2], -1, m, *args[4:], _device.ptr(tmp), nbytes,
                                          rt.stream()) == _ffi.NM_ERR_INVALID


# ---- voxel_table -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", [0.1, 0.25])
def test_voxel_table_against_numpy(scene, edge):
    pts, ix = scene["pts"], scene["index"][edge]
    _, inverse = inverse_of(pts, edge)
    counts = np.bincount(inverse)
    for attr in (scene["attr"][:, 1], scene["attr"], scene["attr16"]):          # D = 1 as a vector, 5, 16
        cols = attr.reshape(len(pts), -1)
        want_sum = np.stack([np.bincount(inverse, weights=cols[:, c]) for c in range(cols.shape[1])], axis=1)
        want_min = np.full(want_sum.shape, np.inf)
        want_max = np.full(want_sum.shape, -np.inf)
        for c in range(cols.shape[1]):
            np.minimum.at(want_min[:, c], inverse, cols[:, c])
            np.maximum.at(want_max[:, c], inverse, cols[:, c])
        got = ix.voxel_table(attr, reduce="sum")
        assert got.dtype == np.float64 and got.shape == want_sum.shape
        assert np.array_equal(got, want_sum)
        assert np.array_equal(ix.voxel_table(attr), want_sum / counts[:, None])             # the default: mean
        assert np.array_equal(ix.voxel_table(attr, reduce="mean"), want_sum / counts[:, None])
        assert np.array_equal(ix.voxel_table(attr, reduce="min"), want_min)
        assert np.array_equal(ix.voxel_table(attr, reduce="max"), want_max)
    # torch in, torch out; a table with a row stride
    wide = torch.from_numpy(scene["attr16"]).cuda()
    got = ix.voxel_table(wide[:, :5], reduce="sum")
    assert isinstance(got, torch.Tensor)
    want = np.stack([np.bincount(inverse, weights=scene["attr"][:, c]) for c in range(5)], axis=1)
    assert np.array_equal(got.cpu().numpy(), want)


def test_voxel_table_argument_checks(scene):
    pts, ix = scene["pts"], scene["index"][0.1]
    with pytest.raises(ValueError, match="between 1 and 16 attribute columns"):
        ix.voxel_table(np.zeros((len(pts), 17)))
    with pytest.raises(ValueError, match="one row per search point"):
        ix.voxel_table(scene["attr"][:-1])
    with pytest.raises(ValueError):
        ix.voxel_table(scene["attr"], reduce="median")


# ---- neighborhood_stats ----------------------------------------------------------------------------------------

def loop_stats(offsets, index, values):
    """count, mean, min, max per query by a plain left-to-right loop over the listed voxels' rows of `values`"""
    nq, dims = len(offsets) - 1, values.shape[1]
    mean, vmin, vmax = np.zeros((nq, dims)), np.zeros((nq, dims)), np.zeros((nq, dims))
    for q in range(nq):
        rows = values[index[offsets[q]:offsets[q + 1]]]
        k = len(rows)
        if k == 0:
            continue
        for c, vals in enumerate(rows.T.tolist()):
            s = 0.0
            for v in vals:
                s += v
            mean[q, c] = s / k
        vmin[q], vmax[q] = rows.min(axis=0), rows.max(axis=0)
    return np.diff(offsets).astype(np.int32), mean, vmin, vmax


@pytest.fixture(scope="module", params=[(0.1, 0.3), (0.1, 0.45), (0.25, 1.2)], ids=lambda p: "e%g-r%g" % p)
def stats_case(request, scene):
    """one (edge, radius): the queries (the scene and 300 points of which some lie outside), the handle of that
    edge, its 16-column mean table and the loop's results for it - column c does not depend on the others, so
    the narrower tables are checked against the leading columns"""
    edge, radius = request.param
    ix = scene["index"][edge]
    query = np.concatenate((scene["pts"], scene["extra"]))
    table = ix.voxel_table(scene["attr16"], reduce="mean")
    offsets, index = ix.lists(query, radius)
    return {"ix": ix, "query": query, "radius": radius, "table": table,
            "want": loop_stats(offsets, index, table)}


@pytest.mark.parametrize("dims", [1, 5, 16])
def test_neighborhood_stats_against_the_lists(stats_case, dims):
    ix, query, radius, table = (stats_case[k] for k in ("ix", "query", "radius", "table"))
    want_count, want_mean, want_min, want_max = stats_case["want"]
    values = table[:, 0] if dims == 1 else np.ascontiguousarray(table[:, :dims])
    count, mean, vmin, vmax = ix.neighborhood_stats(query, radius, values)
    assert count.dtype == np.int32 and count.shape == (len(query),)
    assert mean.dtype == vmin.dtype == vmax.dtype == np.float64
    assert mean.shape == vmin.shape == vmax.shape == (len(query), dims)
    assert np.array_equal(count, want_count)
    assert np.array_equal(mean, want_mean[:, :dims])
    assert np.array_equal(vmin, want_min[:, :dims])
    assert np.array_equal(vmax, want_max[:, :dims])
    empty = count == 0
    assert empty.any() and not empty.all()
    assert not mean[empty].any() and not vmin[empty].any() and not vmax[empty].any()
    if dims >= 4:          # the constant column: a sequential sum of k times 3.25 and one division are exact
        assert np.all(table[:, 3] == 3.25)
        assert np.all(mean[~empty, 3] == 3.25) and np.all(vmin[~empty, 3] == 3.25)


def test_neighborhood_stats_of_strided_tables(stats_case):
    ix, query, radius, table = (stats_case[k] for k in ("ix", "query", "radius", "table"))
    want_count, want_mean, want_min, want_max = stats_case["want"]
    # rows 32 doubles apart on the device, five columns used; torch in (the query cloud decides), torch out
    wide = torch.full((len(table), 32), np.nan, dtype=torch.float64, device="cuda")
    wide[:, :16] = torch.from_numpy(table).cuda()
    view = wide[:, :5]
    assert view.stride(0) == 32
    count, mean, vmin, vmax = ix.neighborhood_stats(torch.from_numpy(query).cuda(), radius, view)
    assert isinstance(count, torch.Tensor) and isinstance(mean, torch.Tensor)
    assert np.array_equal(count.cpu().numpy(), want_count)
    assert np.array_equal(mean.cpu().numpy(), want_mean[:, :5])
    assert np.array_equal(vmin.cpu().numpy(), want_min[:, :5])
    assert np.array_equal(vmax.cpu().numpy(), want_max[:, :5])
    # every other column of a numpy table
    count, mean, vmin, vmax = ix.neighborhood_stats(query, radius, table[:, ::2])
    assert np.array_equal(count, want_count)
    assert np.array_equal(mean, want_mean[:, ::2])
    assert np.array_equal(vmin, want_min[:, ::2]) and np.array_equal(vmax, want_max[:, ::2])


def test_neighborhood_stats_on_the_inclusive_boundary():
    """points at half-integers, e = 1, r = 3: voxel centres ARE the points, candidates sit at exactly r
    (test_inclusive_boundary_on_a_lattice_aligned_cloud): the statistics include what the lists include"""
    rs = np.random.RandomState(19)
    cells = np.unique(rs.randint(0, [40, 20, 12], size=(4000, 3)), axis=0)
    pts = cells + 0.5
    ix = multiscale.NeighborIndex(pts, 1.0)
    offsets, index = ix.lists(pts, 3.0)
    d2 = ((ix.voxels()[index] - np.repeat(pts, np.diff(offsets), axis=0)) ** 2).sum(1)
    assert d2.max() == 9.0
    values = np.stack((np.arange(ix.n_voxels, dtype=np.float64), rs.rand(ix.n_voxels)), axis=1)
    count, mean, vmin, vmax = ix.neighborhood_stats(pts, 3.0, values)
    assert np.array_equal(count, np.diff(offsets))
    # column 0 is the voxel number: the extremes are the ends of the (ascending) list
    assert np.array_equal(vmin[:, 0], index[offsets[:-1]]) and np.array_equal(vmax[:, 0], index[offsets[1:] - 1])
    want = loop_stats(offsets, index, values)
    assert np.array_equal(mean, want[1]) and np.array_equal(vmin, want[2]) and np.array_equal(vmax, want[3])


def test_stats_entry_point_argument_checks(scene):
    rt = _device.get_runtime()
    pts, ix = scene["pts"], scene["index"][0.1]
    lat = ix.filter.nm_lattice
    query = torch.from_numpy(pts[:64]).to(rt.device)
    values = torch.zeros((ix.n_voxels, 16), dtype=torch.float64, device=rt.device)
    count = torch.zeros(64, dtype=torch.int32, device=rt.device)
    out = torch.zeros((64, 16), dtype=torch.float64, device=rt.device)
    null = ctypes.c_void_p(0)

    def call(radius=0.3, d_values=_device.ptr(values), vstride=16, dims=4, d_count=_device.ptr(count),
             d_mean=_device.ptr(out), ostride=16, d_query=_device.ptr(query)):
        return rt.lib.nm_neighbor_index_stats(rt.ctx, d_query, 64, 3, ctypes.byref(lat), radius,
                                              _device.ptr(ix._work), ix._work.numel(), d_values, vstride, dims,
                                              d_count, d_mean, null, null, ostride, rt.stream())

    assert call() == _ffi.NM_OK
    for bad in (dict(dims=0), dict(dims=17), dict(vstride=3), dict(ostride=3), dict(d_values=null),
                dict(d_query=null), dict(d_count=null, d_mean=null)):
        assert call(**bad) == _ffi.NM_ERR_INVALID
    assert call(radius=500.0) == _ffi.NM_ERR_RADIUS
    assert call(d_mean=null, ostride=0) == _ffi.NM_OK                      # counts alone need no output stride
    # voxel_of and voxel_reduce
    voxel = torch.zeros(64, dtype=torch.int64, device=rt.device)
    args = (ctypes.byref(lat), _device.ptr(ix._work), ix._work.numel())
    assert rt.lib.nm_neighbor_index_voxel_of(rt.ctx, _device.ptr(query), 64, 2, *args, _device.ptr(voxel),
                                             rt.stream()) == _ffi.NM_ERR_INVALID
    assert rt.lib.nm_neighbor_index_voxel_of(rt.ctx, _device.ptr(query), 64, 3, *args, null,
                                             rt.stream()) == _ffi.NM_ERR_INVALID
    assert rt.lib.nm_neighbor_index_voxel_of(rt.ctx, _device.ptr(query), 64, 3, args[0], args[1], 1024,
                                             _device.ptr(voxel), rt.stream()) == _ffi.NM_ERR_WORKSPACE
    start, rows = (torch.from_numpy(a).to(rt.device) for a in ix.members())
    attr = torch.zeros((len(pts), 4), dtype=torch.float64, device=rt.device)
    table = torch.zeros((ix.n_voxels, 4), dtype=torch.float64, device=rt.device)

    def reduce(dims=4, stride=4, op=0, d_attr=_device.ptr(attr)):
        return rt.lib.nm_neighbor_index_voxel_reduce(rt.ctx, _device.ptr(start), _device.ptr(rows), ix.n_voxels,
                                                     d_attr, stride, dims, op, _device.ptr(table), rt.stream())

    assert reduce() == _ffi.NM_OK
    for bad in (dict(dims=0), dict(dims=17), dict(stride=3), dict(op=4), dict(op=-1), dict(d_attr=null)):
        assert reduce(**bad) == _ffi.NM_ERR_INVALID
    rt.lib.nm_clear_error(rt.ctx)


# ---- fields.vector_field_stats ---------------------------------------------------------------------------------

def test_vector_field_stats_against_the_field_mean_and_the_oracle(scene):
    pts, attr = scene["pts"], scene["attr"]
    query = np.concatenate((pts[:1500], scene["extra"]))
    edges, radii = [0.1, 0.25], [0.3, 1.2]
    count, mean, vmin, vmax = fields.vector_field_stats(query, pts, attr, edges, radii)
    assert count.shape == (len(query), 2) and count.dtype == np.int32
    assert mean.shape == vmin.shape == vmax.shape == (len(query), 10)
    field = fields.vector_field_mean(query, pts, attr, edges, radii)
    for s, (e, r) in enumerate(zip(edges, radii)):
        want = oracle.one_scale_field_mean(query, pts, attr, e, r)
        bound = 1e-12 * max(1.0, np.abs(want).max())
        block = mean[:, 5 * s:5 * s + 5]
        assert np.abs(block - want).max() <= bound
        assert np.abs(block - field[:, 5 * s:5 * s + 5]).max() <= bound
        assert np.array_equal(count[:, s], oracle.one_scale_fast(query, pts, e, r)[:, 0])
        # per scale, what the handle gives on its own
        ix = scene["index"][e]
        one = ix.neighborhood_stats(query, r, ix.voxel_table(attr))
        assert np.array_equal(count[:, s], one[0])
        for got, alone in zip((mean, vmin, vmax), one[1:]):
            assert np.array_equal(got[:, 5 * s:5 * s + 5], alone)
    with pytest.raises(ValueError):
        fields.vector_field_stats(query, pts, np.zeros((len(pts), 17)), [0.1], [0.3])
    with pytest.raises(ValueError):
        fields.vector_field_stats(query, pts, attr[:-1], [0.1], [0.3])


def test_vector_field_stats_builds_one_handle_per_distinct_edge(scene, monkeypatch):
    built = []
    init = multiscale.NeighborIndex.__init__

    def counting(self, search_cloud, edge_length, method="auto"):
        built.append(float(edge_length))
        init(self, search_cloud, edge_length, method=method)

    monkeypatch.setattr(multiscale.NeighborIndex, "__init__", counting)
    dev = torch.from_numpy(scene["pts"]).cuda()
    attr = torch.from_numpy(scene["attr"][:, 1]).cuda()                       # one column, given as a vector
    count, mean, vmin, vmax = fields.vector_field_stats_gpu(dev, dev, attr, [0.1, 0.1], [0.3, 0.45])
    assert built == [0.1]
    assert isinstance(mean, torch.Tensor) and mean.shape == (len(dev), 2) and count.shape == (len(dev), 2)
    count = count.cpu().numpy()
    assert np.all(count[:, 0] <= count[:, 1]) and (count[:, 0] < count[:, 1]).any()
    fields.vector_field_stats_gpu(dev, dev, attr, [0.1, 0.25, 0.1], [0.3, 1.2, 0.2])
    assert built == [0.1, 0.1, 0.25]


# ---- a handle that searches sorted addresses -----------------------------------------------------------------------

def test_a_search_handle_raises_from_the_five_methods(scene):
    pts = scene["pts"]
    ix = multiscale.NeighborIndex(pts, 0.1, method="search")
    assert ix.method == "search"
    calls = (lambda: ix.voxel_of(pts), ix.point_counts, ix.members, lambda: ix.voxel_table(scene["attr"]),
             lambda: ix.neighborhood_stats(pts, 0.3, np.zeros((ix.n_voxels, 2))))
    for call in calls:
        with pytest.raises(ValueError, match="index form"):
            call()
