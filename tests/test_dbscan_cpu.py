"""
CPU tests for NeighborIndex.dbscan: they pin the yardstick the GPU tests (test_dbscan_gpu.py) are measured against -
the numpy reference of tests/dbscan_reference.py - to sklearn.cluster.DBSCAN with sample_weight and to graphs labelled
by hand, and check that the library declares, binds and exports the new symbols under ABI 7.
"""

import ctypes
import os

import numpy as np
import pytest
from sklearn.cluster import DBSCAN

import components_reference as cref
import dbscan_reference as ref
from nimrud_amd import _ffi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nimrud_hip.h")
SYMBOLS = ("nm_neighbor_index_dbscan", "nm_neighbor_index_dbscan_workspace_bytes")
E = ref.EDGE


def centres(cells):
    return (np.asarray(cells, dtype=np.float64) + 0.5) * E


@pytest.fixture(scope="module")
def lattices():
    """name -> (cell centres in position order, weights, edges per radius), made once and never changed"""
    out = {}
    for name, m in (("random", 17991), ("thin", 9481)):
        cells = np.unique(ref.lattice_cells(name), axis=0)
        cells = cells[np.lexsort((cells[:, 0], cells[:, 1], cells[:, 2]))]          # address order: z, y, x
        assert len(cells) == m
        voxels = centres(cells)
        voxels.setflags(write=False)
        out[name] = (voxels, ref.case_weights(m), {})
    return out


@pytest.mark.parametrize("name,rho,min_weight", ref.CASES)
def test_the_reference_is_sklearns_dbscan_with_sample_weight(lattices, name, rho, min_weight):
    voxels, weight, edges = lattices[name]
    m = len(voxels)
    if rho not in edges:
        edges[rho] = cref.edges(voxels, rho * E)
    i, j = edges[rho]
    labels, sizes, core, density, total = ref.dbscan_of_edges(voxels, (i, j), min_weight, weight)
    sk = DBSCAN(eps=rho * E, min_samples=min_weight).fit(voxels, sample_weight=weight)
    sk_core = np.zeros(m, dtype=bool)
    sk_core[sk.core_sample_indices_] = True
    print("%s, %g e, min_weight %d: %d core, %d border, %d noise, %d clusters" % (
        name, rho, min_weight, core.sum(), ((labels >= 0) & ~core).sum(), (labels < 0).sum(), len(sizes)))
    assert np.array_equal(core, sk_core)
    assert np.array_equal(labels < 0, sk.labels_ < 0)                               # noise
    # the two labelings of the core voxels: a bijection
    pairs = np.unique(np.stack((labels[core], sk.labels_[core]), axis=1), axis=0)
    assert len(pairs) == len(sizes) == total == len(set(sk.labels_[sk.labels_ >= 0]))
    assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))
    # every border voxel carries the label of one of its core neighbors (which one, DBSCAN leaves open)
    border = (labels >= 0) & ~core
    src, dst = np.concatenate((i, j)), np.concatenate((j, i))
    hit = border[src] & core[dst] & (labels[src] == labels[dst])
    assert np.array_equal(np.unique(src[hit]), np.nonzero(border)[0])
    # density, sizes and numbering as the contract words them
    assert sizes.sum() == weight[labels >= 0].sum()
    if len(sizes):
        first = np.full(len(sizes), m)
        np.minimum.at(first, labels[core], np.nonzero(core)[0])
        assert (np.diff(first) > 0).all()
    else:
        assert not core.any() and (labels == -1).all()
    if (name, rho, min_weight) == ("random", 2.2, 60):
        assert len(sizes) == 0                                                      # no core voxel at all


def test_the_cases_cover_border_noise_and_several_clusters(lattices):
    voxels, weight, _ = lattices["random"]
    labels, sizes, core, density = ref.dbscan(voxels, 1.5 * E, 12, weight)
    assert core.any() and (~core & (labels >= 0)).any() and (labels < 0).any() and len(sizes) > 1
    assert density.min() >= 1 and density.dtype == np.int64


def test_a_tie_between_two_clusters_goes_to_the_smaller_position():
    voxels = centres(ref.TIE_CELLS)
    labels, sizes, core, density = ref.dbscan(voxels, E, ref.TIE_MIN_WEIGHT, ref.TIE_WEIGHTS)
    assert density.tolist() == ref.TIE_DENSITY
    assert core.tolist() == [True] * 5 + [False] + [True] * 3 + [False]
    # voxel 5 is one edge from voxel 1 (cluster 1) and from voxel 8 (cluster 0): the smaller POSITION wins
    assert labels.tolist() == ref.TIE_LABELS and sizes.tolist() == ref.TIE_SIZES
    # a nearer core neighbor beats a smaller position: cells 0 2 4 5 7 of a row at two edges, the light voxel at 4 is
    # two cells from voxel 1 and one cell from voxel 3
    row = centres([(x, 0, 0) for x in (0, 2, 4, 5, 7)])
    labels, sizes, core, density = ref.dbscan(row, 2.0 * E, 12, [9, 5, 0, 5, 9])
    assert density.tolist() == [14, 14, 10, 14, 14] and core.tolist() == [True, True, False, True, True]
    assert labels.tolist() == [0, 0, 1, 1, 1] and sizes.tolist() == [14, 14]


def test_two_blocks_and_a_bridge():
    cells = ref.bridge_cells()
    cells = cells[np.lexsort((cells[:, 0], cells[:, 1], cells[:, 2]))]
    voxels = centres(cells)
    assert len(cref.components(voxels, E)[1]) == 1                                  # single linkage welds them
    labels, sizes, core, density = ref.dbscan(voxels, E, 5)
    assert sizes.tolist() == [217, 217]
    on_bridge = (cells[:, 0] >= 6) & (cells[:, 0] < 16)
    assert on_bridge.sum() == 10 and not core[on_bridge].any() and (density[on_bridge] == 3).all()
    x = cells[on_bridge, 0]
    assert labels[on_bridge][x == 6].tolist() == [0] and labels[on_bridge][x == 15].tolist() == [1]
    assert (labels[on_bridge][(x > 6) & (x < 15)] == -1).all()
    # the corners of the blocks (density 4) are border, everything else in them is core
    corner = ~on_bridge & (density == 4)
    assert corner.sum() == 16 and not core[corner].any() and core[~on_bridge & ~corner].all()
    assert (labels[cells[:, 0] < 6] == 0).all() and (labels[cells[:, 0] >= 16] == 1).all()


def test_min_weight_one_is_components_and_min_size_drops_border_with_the_cluster():
    voxels = centres(np.unique(cref.random_lattice_cells(), axis=0)[:3000])
    pairs = cref.edges(voxels, E)
    cls = np.random.default_rng(5).integers(-1, 3, len(voxels))
    for min_weight in (1, 0, -3):
        got = ref.dbscan_of_edges(voxels, pairs, min_weight, None, cls, 2)
        want = cref.components_of_edges(len(voxels), pairs, cls, None, 2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[4] == want[2]
        assert np.array_equal(got[2], cls >= 0)
    # a bar 0..6 with a light middle: [4 4 1 1 1 4 4] at min_weight 5 - voxel 3 is border of the first bar
    bar = centres([(x, 0, 0) for x in range(7)])
    weight = [4, 4, 1, 1, 1, 4, 4]
    labels, sizes, core, density = ref.dbscan(bar, E, 5, weight)
    assert density.tolist() == [8, 9, 6, 3, 6, 9, 8] and core.tolist() == [True] * 3 + [False] + [True] * 3
    assert labels.tolist() == [0, 0, 0, 0, 1, 1, 1] and sizes.tolist() == [10, 9]
    labels, sizes, core, density = ref.dbscan(bar, E, 5, weight, None, 10)
    assert labels.tolist() == [0, 0, 0, 0, -1, -1, -1] and sizes.tolist() == [10] and core.sum() == 6
    labels, sizes, core, density = ref.dbscan(bar, E, 5, weight, [0, 0, 0, 0, 1, 1, 1])
    assert density.tolist() == [8, 9, 6, 2, 5, 9, 8] and labels.tolist() == [0, 0, 0, 0, 1, 1, 1]
    labels, sizes, core, density = ref.dbscan(bar, E, 5, weight, [0, 0, -1, 0, 0, 0, 0])
    assert density.tolist() == [8, 8, 0, 2, 6, 9, 8] and labels.tolist() == [0, 0, -1, 1, 1, 1, 1]


def test_both_symbols_are_declared_bound_and_exported():
    with open(HEADER) as f:
        header = f.read()
    exported = ctypes.CDLL(_ffi.LIBRARY_PATH)
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(exported, name), name
    restype, argtypes = _ffi.SIGNATURES["nm_neighbor_index_dbscan"]
    assert restype is ctypes.c_int and len(argtypes) == 17
    assert "negative weights are unsupported" in header
    assert _ffi.load().nm_abi_version() == 7 == _ffi.ABI_VERSION


def test_workspace_query_is_a_host_function_that_grows_with_m():
    lib = _ffi.load()
    bytes_for = lib.nm_neighbor_index_dbscan_workspace_bytes
    assert bytes_for(-1) == 0 and bytes_for(-(1 << 40)) == 0 and bytes_for(1 << 31) == 0
    counts = (0, 1, 4095, 4096, 4097, 18000, 10 ** 6, 10 ** 6 + 1, 10 ** 8, (1 << 31) - 1)
    sizes = [bytes_for(n) for n in counts]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert all(s % 16 == 0 for s in sizes)
    # the components scratch and the effective class of every voxel: 8 bytes per voxel of the scratch's room more
    for n, s in zip(counts, sizes):
        room = max((n + 4095) // 4096, 1) * 4096
        assert s == lib.nm_neighbor_index_components_workspace_bytes(n) + 8 * room
    assert bytes_for(10 ** 6) >= 32 * 10 ** 6
