"""
GPU tests of NeighborIndex.nearest / multiscale.nearest_voxels (nm_neighbors.hip: k_nn_near, k_nn_wide) against the
brute-force reference of tests/nearest_reference.py, which test_nearest_cpu.py pins to scipy's cKDTree.query.
squared distances and indices are compared bit for bit; the square root within 1 ulp (torch and numpy need not
round alike; on the MI355X the scene came out bit-equal).

the kernel's buckets are k = 1, 2..8, 9..16, 17..32: the scene enters each at its smallest and largest k.
"""

import ctypes

import numpy as np
import pytest
import torch

import nearest_reference as ref
from nimrud_amd import _ffi
from nimrud_amd import device as _device
from nimrud_amd.minimal import multiscale

pytestmark = pytest.mark.gpu

INF = float("inf")


class Case(object):
    """a search cloud, its handle, its queries and all squared distances (made once, never changed)"""

    def __init__(self, cloud, query, edge):
        self.cloud, self.query, self.edge = cloud, query, edge
        self.index = multiscale.NeighborIndex(cloud, edge, method="index")
        self.voxels = ref.voxels_of(cloud, edge)
        self.d2 = ref.all_d2(self.voxels, query)
        self.d2.setflags(write=False)

    def want(self, k, limit=None):
        return ref.nearest(self.voxels, self.query, k, limit, d2=self.d2)


@pytest.fixture(scope="module")
def scene():
    cloud, query = ref.scene_cloud()
    return Case(cloud, query, ref.SCENE_EDGE)


@pytest.fixture(scope="module")
def island():
    cloud = ref.island_cloud()
    return Case(cloud, cloud, ref.ISLAND_EDGE)


@pytest.fixture(scope="module")
def far():
    cloud, query = ref.far_cloud()
    return Case(cloud, query, 0.1)


def c_nearest(index, query, k, limit, dist2, idx, out_stride, found=None, tmp="auto", work=None, lattice=None):
    """nm_neighbor_index_nearest itself: (status, message)"""
    rt = index._rt
    nq = query.shape[0]
    if isinstance(tmp, str):
        tmp = torch.empty(rt.lib.nm_neighbor_index_nearest_workspace_bytes(nq), dtype=torch.uint8, device=rt.device)
    work = index._work if work is None else work
    lat = index.filter.nm_lattice if lattice is None else lattice
    rc = rt.lib.nm_neighbor_index_nearest(
        rt.ctx, _device.ptr(query), nq, _device.row_stride(query), ctypes.byref(lat), k, limit, _device.ptr(work),
        work.numel(), _device.ptr(dist2), _device.ptr(idx), out_stride, _device.ptr(found), _device.ptr(tmp),
        tmp.numel() if tmp is not None else 0, rt.stream())
    torch.cuda.synchronize()
    msg = rt.lib.nm_last_error(rt.ctx)
    return rc, (msg.decode("utf-8", "replace") if msg else "")


def found_of(index, query, k, limit):
    q = torch.from_numpy(np.ascontiguousarray(query)).cuda()
    idx = torch.empty((len(query), k), dtype=torch.int64, device="cuda")
    found = torch.full((len(query),), -7, dtype=torch.int32, device="cuda")
    rc, msg = c_nearest(index, q, k, INF if limit is None else limit, None, idx, k, found=found)
    assert rc == _ffi.NM_OK, msg
    return found.cpu().numpy(), idx.cpu().numpy()


def assert_rows(got, want, k):
    got_d2, got_i = got
    want_d2, want_i = want[0], want[1]
    assert got_d2.dtype == np.float64 and got_i.dtype == np.int64
    assert got_d2.shape == got_i.shape == (len(want_d2), k)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(got_d2, want_d2)          # bit for bit; inf == inf


# ---- 1. scene ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("limit", [None, 0.6])
@pytest.mark.parametrize("k", [1, 2, 8, 9, 16, 17, 32])
def test_scene_matches_the_reference_bit_for_bit(scene, k, limit):
    want = scene.want(k, limit)
    assert_rows(scene.index.nearest(scene.query, k, max_distance=limit, squared=True), want, k)
    found, idx = found_of(scene.index, scene.query, k, limit)
    assert np.array_equal(found, want[2]) and np.array_equal(idx, want[1])
    # the default return: the square root, within 1 ulp of numpy's
    dist, idx = scene.index.nearest(scene.query, k, max_distance=limit)
    root = np.sqrt(want[0])
    real = np.isfinite(root)
    assert np.array_equal(idx, want[1]) and np.array_equal(np.isfinite(dist), real)
    print("sqrt: %d of %d real slots differ from numpy's" % ((dist[real] != root[real]).sum(), real.sum()))
    assert (np.abs(dist[real] - root[real]) <= np.spacing(root[real])).all()


# ---- 2. ties -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 8, 27])
def test_island_ties_go_to_the_smaller_voxel_index(island, k):
    assert_rows(island.index.nearest(island.query, k, squared=True), island.want(k), k)


# ---- 3. agreement with lists() -------------------------------------------------------------------------------------

@pytest.mark.parametrize("which, r", [("island", 0.5), ("scene", 0.6)])
def test_limited_rows_are_the_lists(which, r, request):
    case = request.getfixturevalue(which)
    if which == "island":
        assert (case.d2 == r * r).any()             # voxels exactly at the limit: the inclusive boundary
    offsets, index = case.index.lists(case.query, r)
    _, got = case.index.nearest(case.query, 32, max_distance=r)
    counts = np.diff(offsets)
    assert (counts < 32).any() and (counts > 0).any()
    for q in np.nonzero(counts < 32)[0]:
        real = got[q][got[q] >= 0]
        assert np.array_equal(np.sort(real), index[offsets[q]:offsets[q + 1]]), q


# ---- 4. fewer than k -----------------------------------------------------------------------------------------------

def test_fewer_voxels_than_k_pads_with_inf_and_minus_one():
    cloud = np.array([[0.0, 0.0, 0.0], [3.0, 0.5, 0.2], [0.4, 4.0, 1.0], [5.0, 5.0, 5.0], [1.0, 2.0, 6.5]])
    query = np.vstack((cloud, [[2.0, 2.0, 2.0], [-3.0, 9.0, 1.0]]))
    case = Case(cloud, query, 0.5)
    assert len(case.voxels) == 5
    d2, idx = case.index.nearest(query, 8, squared=True)
    assert_rows((d2, idx), case.want(8), 8)
    assert (idx[:, :5] >= 0).all() and (idx[:, 5:] == -1).all() and np.isinf(d2[:, 5:]).all()
    assert (found_of(case.index, query, 8, None)[0] == 5).all()


def test_zero_limit_finds_the_own_voxel_only(island):
    d2, idx = island.index.nearest(island.query, 8, max_distance=0.0, squared=True)
    assert np.array_equal(idx[:, 0], island.index.voxel_of(island.query))
    assert (d2[:, 0] == 0.0).all() and (idx[:, 1:] == -1).all() and np.isinf(d2[:, 1:]).all()
    assert (found_of(island.index, island.query, 8, 0.0)[0] == 1).all()


# ---- 5. far away: the wide stage and the compaction ---------------------------------------------------------------

def test_far_queries_take_the_wide_stage(far):
    want = far.want(8)
    assert [int(w) for w in far.index.filter.widths] == [8, 8, 8]
    assert np.sqrt(want[0][:, 7]).max() / far.edge > 100.0        # some k-th neighbor is over 100 cells away
    assert_rows(far.index.nearest(far.query, 8, squared=True), want, 8)


# ---- 6. every stage boundary ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sparse():
    cloud, query = ref.sparse_box()
    return Case(cloud, query, 0.25)


@pytest.mark.parametrize("limit", [None, 2.0])
@pytest.mark.parametrize("k", [1, 8, 32])
def test_kth_distances_from_under_a_cell_to_tens_of_cells(sparse, k, limit):
    want = sparse.want(k, limit)
    if limit is None:
        cells = np.sqrt(sparse.want(1)[0][:, 0]) / sparse.edge, np.sqrt(sparse.want(32)[0][:, 31]) / sparse.edge
        assert cells[0].min() < 1.0 and cells[1].max() > 30.0
    assert_rows(sparse.index.nearest(sparse.query, k, max_distance=limit, squared=True), want, k)


# ---- 7. shapes and plumbing ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", [0, 1, 63, 257])
def test_any_number_of_queries(scene, nq):
    d2, idx = scene.index.nearest(scene.query[:nq], 8, squared=True)
    want = scene.want(8)
    assert_rows((d2, idx), (want[0][:nq], want[1][:nq]), 8)


def test_strides_and_single_outputs_through_the_c_entry_point(scene):
    k, n = 8, 257
    want = scene.want(k)
    wide = torch.zeros((n, 5), dtype=torch.float64, device="cuda")
    wide[:, :3] = torch.from_numpy(scene.query[:n]).cuda()
    wide[:, 3:] = 1e30
    query = wide[:, :3]
    assert _device.row_stride(query) == 5
    # torch in, torch out, rows of stride 5
    d2, idx = scene.index.nearest(query, k, squared=True)
    assert isinstance(d2, torch.Tensor) and isinstance(idx, torch.Tensor) and d2.is_cuda and idx.is_cuda
    assert_rows((d2.cpu().numpy(), idx.cpu().numpy()), (want[0][:n], want[1][:n]), k)
    # out_stride > k: the padding columns are not touched
    d2 = torch.full((n, k + 3), -5.0, dtype=torch.float64, device="cuda")
    idx = torch.full((n, k + 3), -9, dtype=torch.int64, device="cuda")
    rc, msg = c_nearest(scene.index, query, k, INF, d2, idx, k + 3)
    assert rc == _ffi.NM_OK, msg
    assert_rows((d2[:, :k].cpu().numpy(), idx[:, :k].cpu().numpy()), (want[0][:n], want[1][:n]), k)
    assert (d2[:, k:] == -5.0).all() and (idx[:, k:] == -9).all()
    # one output only
    only_i = torch.full((n, k), -9, dtype=torch.int64, device="cuda")
    rc, msg = c_nearest(scene.index, query, k, INF, None, only_i, k)
    assert rc == _ffi.NM_OK and np.array_equal(only_i.cpu().numpy(), want[1][:n]), msg
    only_d = torch.full((n, k), -5.0, dtype=torch.float64, device="cuda")
    rc, msg = c_nearest(scene.index, query, k, INF, only_d, None, k)
    assert rc == _ffi.NM_OK and np.array_equal(only_d.cpu().numpy(), want[0][:n]), msg


def test_numpy_in_numpy_out_identity_and_the_one_shot_form(scene):
    d2, idx = scene.index.nearest(scene.query, 8, squared=True)
    assert isinstance(d2, np.ndarray) and isinstance(idx, np.ndarray)
    got = multiscale.nearest_voxels(scene.query, scene.cloud, scene.edge, 8, max_distance=0.6)
    want = scene.index.nearest(scene.query, 8, max_distance=0.6)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the search cloud by identity: the handle's own copy is walked (an upload would go through as_cloud)
    calls = []
    original = _device.as_cloud
    _device.as_cloud = lambda *a, **kw: calls.append(1) or original(*a, **kw)
    try:
        own = scene.index.nearest(scene.cloud, 1, squared=True)
    finally:
        _device.as_cloud = original
    assert not calls
    assert_rows(own, ref.nearest(scene.voxels, scene.cloud, 1), 1)
    assert np.array_equal(own[1][:, 0], scene.index.voxel_of(scene.cloud))       # a point's nearest voxel is its own


# ---- 8. purity -----------------------------------------------------------------------------------------------------

def test_same_call_twice_and_permuted_queries(scene, far):
    for case, k in ((scene, 32), (far, 8)):
        a = case.index.nearest(case.query, k, squared=True)
        b = case.index.nearest(case.query, k, squared=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        perm = np.random.RandomState(3).permutation(len(case.query))
        c = case.index.nearest(case.query[perm], k, squared=True)
        assert np.array_equal(c[0], a[0][perm]) and np.array_equal(c[1], a[1][perm])


def test_a_row_does_not_depend_on_the_other_queries(scene, far):
    cloud = np.vstack((scene.cloud, far.cloud))
    index = multiscale.NeighborIndex(cloud, 0.25, method="index")
    near_q, far_q = scene.query, far.query
    n = min(len(near_q), len(far_q))
    mixed = np.empty((2 * n, 3))
    mixed[0::2], mixed[1::2] = near_q[:n], far_q[:n]
    got = index.nearest(mixed, 8, squared=True)
    alone_near = index.nearest(near_q[:n], 8, squared=True)
    alone_far = index.nearest(far_q[:n], 8, squared=True)
    for c in (0, 1):
        assert np.array_equal(got[c][0::2], alone_near[c]) and np.array_equal(got[c][1::2], alone_far[c])
    assert_rows(got, ref.nearest(ref.voxels_of(cloud, 0.25), mixed, 8), 8)


# ---- 9. errors -----------------------------------------------------------------------------------------------------

def test_argument_errors_through_the_c_entry_point(scene, far):
    k, n = 8, 100
    query = torch.from_numpy(scene.query[:n]).cuda()
    d2 = torch.full((n, k), -5.0, dtype=torch.float64, device="cuda")
    idx = torch.full((n, k), -9, dtype=torch.int64, device="cuda")
    short = torch.empty(64, dtype=torch.uint8, device="cuda")
    assert scene.index._work.numel() < far.index._work.numel()
    cases = [
        (dict(k=0), _ffi.NM_ERR_INVALID),
        (dict(k=33), _ffi.NM_ERR_INVALID),
        (dict(out_stride=k - 1), _ffi.NM_ERR_INVALID),
        (dict(dist2=None, idx=None), _ffi.NM_ERR_INVALID),
        (dict(limit=-1.0), _ffi.NM_ERR_INVALID),
        (dict(limit=float("nan")), _ffi.NM_ERR_INVALID),
        (dict(limit=1e6), _ffi.NM_ERR_RADIUS),
        (dict(lattice=far.index.filter.nm_lattice), _ffi.NM_ERR_WORKSPACE),      # the index of another lattice
        (dict(tmp=short), _ffi.NM_ERR_INVALID),
        (dict(tmp=None), _ffi.NM_ERR_INVALID),
    ]
    rt = scene.index._rt
    for change, status in cases:
        args = dict(k=k, limit=INF, dist2=d2, idx=idx, out_stride=k)
        args.update(change)
        rc, msg = c_nearest(scene.index, query, **args)
        assert rc == status and msg, (change, rc, msg)
        assert (d2 == -5.0).all() and (idx == -9).all(), change
    rt.check_async(wait=True)               # nothing sticky: the context is as usable as before
    rc, msg = c_nearest(scene.index, query, k, INF, d2, idx, k)
    assert rc == _ffi.NM_OK and np.array_equal(idx.cpu().numpy(), scene.want(k)[1][:n]), msg
    # no queries: NM_OK, nothing done, no scratch needed
    rc, msg = c_nearest(scene.index, query[:0], k, INF, d2, idx, k, tmp=None)
    assert rc == _ffi.NM_OK


def test_argument_errors_in_python(scene):
    for bad in (0, 33, -1, 2.0, "3", True, None):
        with pytest.raises(ValueError):
            scene.index.nearest(scene.query, bad)
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError):
            scene.index.nearest(scene.query, 4, max_distance=bad)
    with pytest.raises(ValueError):
        scene.index.nearest(scene.query[:, :2], 4)
    with pytest.raises(ValueError):
        scene.index.nearest(scene.query, 4, max_distance=1e6)          # the ratio lists() refuses too
    searching = multiscale.NeighborIndex(scene.cloud, scene.edge, method="search")
    with pytest.raises(ValueError, match="index form"):
        searching.nearest(scene.query, 4)
