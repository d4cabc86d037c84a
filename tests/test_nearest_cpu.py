"""
CPU tests for NeighborIndex.nearest: they pin the yardstick the GPU tests (test_nearest_gpu.py) are measured against.
  (a) on a cloud without exact ties the brute-force reference of tests/nearest_reference.py IS scipy's
      cKDTree.query: identical indices, bit-identical distances;
  (b) the dyadic island really is full of exact ties, at the k-th place too - where scipy is no witness and the
      (d2, voxel index) rule decides;
  (c) the library exports the new symbols under ABI 7.
"""

import ctypes

import numpy as np
import pytest
from scipy.spatial import cKDTree

import nearest_reference as ref
from nimrud_amd import _ffi


@pytest.fixture(scope="module")
def scene():
    cloud, query = ref.scene_cloud()
    voxels = ref.voxels_of(cloud, ref.SCENE_EDGE)
    return cloud, query, voxels, ref.all_d2(voxels, query)


def test_scene_is_what_the_issue_describes(scene):
    cloud, query, voxels, _ = scene
    assert cloud.shape == (3000, 3) and query.shape == (1300, 3) and len(voxels) == 884
    lo, hi = cloud.min(0) - ref.SCENE_EDGE / 2, cloud.max(0) + ref.SCENE_EDGE / 2
    assert ((query < lo) | (query > hi)).any(axis=1).sum() > 50        # queries outside the lattice


@pytest.mark.parametrize("limit", [None, 0.6])
@pytest.mark.parametrize("k", [1, 8, 32])
def test_reference_is_ckdtree_query_where_nothing_ties(scene, k, limit):
    _, query, voxels, d2 = scene
    m = len(voxels)
    # scipy is a valid witness only where no row has two equal squared distances among its first k + 1
    head = np.sort(d2, axis=1)[:, :k + 1]
    assert (np.diff(head, axis=1) > 0).all()
    # (its bound is exclusive: no voxel of this cloud sits exactly at it)
    if limit is not None:
        assert not (d2 == limit * limit).any()
    want_d2, want_i, found = ref.nearest(voxels, query, k, limit, d2=d2)
    dist, idx = cKDTree(voxels, leafsize=300).query(query, k, distance_upper_bound=np.inf if limit is None else limit)
    dist, idx = dist.reshape(len(query), k), idx.reshape(len(query), k)
    assert np.array_equal(np.where(idx == m, -1, idx), want_i)
    assert np.array_equal(dist, np.sqrt(want_d2))          # bit for bit, inf in the unused slots
    assert np.array_equal(found, (idx < m).sum(axis=1))
    if limit is not None:
        assert (found == 0).any() and (found == k).any()       # the limit bites, and not everywhere


def test_island_ties_everywhere_and_at_the_kth_place():
    cloud = ref.island_cloud()
    voxels = ref.voxels_of(cloud, ref.ISLAND_EDGE)
    assert np.array_equal(voxels, cloud[np.lexsort((cloud[:, 0], cloud[:, 1], cloud[:, 2]))])   # cell centres
    d2 = ref.all_d2(voxels, cloud)
    assert np.array_equal(d2 * 16.0, np.rint(d2 * 16.0))           # exact: multiples of e^2
    s = np.sort(d2, axis=1)
    assert (np.diff(s[:, :9], axis=1) == 0).any(axis=1).all()      # every row ties among its first nine
    kth_ties = int((s[:, 7] == s[:, 8]).sum())                     # k = 8: the 8th and 9th are equally far
    assert 2 * kth_ties > len(cloud), (kth_ties, len(cloud))
    # the tie rule, spelled out: within equal d2 the smaller voxel index comes first
    want_d2, want_i, _ = ref.nearest(voxels, cloud, 8, d2=d2)
    same = want_d2[:, 1:] == want_d2[:, :-1]
    assert (want_i[:, 1:][same] > want_i[:, :-1][same]).all()
    # r = 0.5 is hit exactly (the inclusive boundary of the lists)
    assert (d2 == 0.25).any()


def test_far_and_sparse_inputs_reach_every_stage():
    cloud, query = ref.far_cloud()
    lat = ref.oracle.Lattice(cloud, 0.1)
    assert [int(w) for w in lat.widths] == [8, 8, 8]               # 256 cells a side, 2^13 superblocks
    voxels = ref.voxels_of(cloud, 0.1)
    d2, _, found = ref.nearest(voxels, query, 8)
    assert (found == 8).all() and np.sqrt(d2[:, 7]).max() / 0.1 > 100.0
    cloud, query = ref.sparse_box()
    voxels = ref.voxels_of(cloud, 0.25)
    for k in (1, 8, 32):
        d2, _, _ = ref.nearest(voxels, query, k)
    cells = np.sqrt(ref.nearest(voxels, query, 1)[0][:, 0]) / 0.25
    assert cells.min() < 1.0
    assert np.sqrt(d2[:, 31]).max() / 0.25 > 30.0


def test_exports_and_constants():
    lib = ctypes.CDLL(_ffi.LIBRARY_PATH)
    assert hasattr(lib, "nm_neighbor_index_nearest") and hasattr(lib, "nm_neighbor_index_nearest_workspace_bytes")
    assert _ffi.NM_NEAREST_MAX_K == 32
    lib = _ffi.load()
    assert lib.nm_abi_version() == 7
    bytes_for = lib.nm_neighbor_index_nearest_workspace_bytes
    assert 0 < bytes_for(0) <= bytes_for(1) < bytes_for(100000)
    assert bytes_for(-1) == 0 and bytes_for(1 << 31) == 0
