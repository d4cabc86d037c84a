"""
CPU tests for NeighborIndex.components: they pin the yardstick the GPU tests (test_components_gpu.py) are measured
against - the numpy + scipy reference of tests/components_reference.py on graphs small enough to label by hand - and
check that the library declares, binds and exports the new symbols under ABI 7.
"""

import ctypes
import os

import numpy as np

import components_reference as ref
from nimrud_amd import _ffi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nimrud_hip.h")
SYMBOLS = ("nm_neighbor_index_components", "nm_neighbor_index_components_workspace_bytes")


def centres(cells):
    return (np.asarray(cells, dtype=np.float64) + 0.5) * ref.EDGE


def bar(x0, n, y=0, z=0):
    return [(x0 + i, y, z) for i in range(n)]


def test_two_bars():
    voxels = centres(bar(0, 5) + bar(0, 4, y=2))
    labels, sizes = ref.components(voxels, ref.EDGE)                # face neighbors only: the limit is inclusive
    assert labels.tolist() == [0] * 5 + [1] * 4 and sizes.tolist() == [5, 4]
    labels, sizes = ref.components(voxels, 0.999 * ref.EDGE)
    assert labels.tolist() == list(range(9)) and sizes.tolist() == [1] * 9
    labels, sizes = ref.components(voxels, 2.0 * ref.EDGE)          # two cells: the bars touch
    assert labels.tolist() == [0] * 9 and sizes.tolist() == [9]
    # interleaved positions: numbering follows the smallest member, not the order scipy met the components in
    mixed = centres([(0, 2, 0), (0, 0, 0), (1, 2, 0), (1, 0, 0), (2, 0, 0)])
    labels, sizes = ref.components(mixed, ref.EDGE)
    assert labels.tolist() == [0, 1, 0, 1, 1] and sizes.tolist() == [2, 3]


def test_a_bar_cut_by_a_class_change():
    voxels = centres(bar(0, 7))
    labels, sizes = ref.components(voxels, ref.EDGE, voxel_class=[4, 4, 4, 2, 2, 2, 2])
    assert labels.tolist() == [0, 0, 0, 1, 1, 1, 1] and sizes.tolist() == [3, 4]
    # a removed voxel cuts too, and is in no component; equal classes on either side do not reach across it
    labels, sizes = ref.components(voxels, ref.EDGE, voxel_class=[0, 0, 0, -1, 0, 0, 0])
    assert labels.tolist() == [0, 0, 0, -1, 1, 1, 1] and sizes.tolist() == [3, 3]
    # ... unless the radius does
    labels, sizes = ref.components(voxels, 2.0 * ref.EDGE, voxel_class=[0, 0, 0, -5, 0, 0, 0])
    assert labels.tolist() == [0, 0, 0, -1, 0, 0, 0] and sizes.tolist() == [6]


def test_min_size_drops_the_middle_component_and_the_rest_keep_their_order():
    voxels = centres(bar(0, 3) + bar(5, 1) + bar(8, 2))
    labels, sizes = ref.components(voxels, ref.EDGE, min_size=2)
    assert labels.tolist() == [0, 0, 0, -1, 1, 1] and sizes.tolist() == [3, 2]
    # sizes are sums of weights: now the first bar is the small one
    weight = [1, 1, 1, 10, 2, 3]
    labels, sizes, total = ref.components_of_edges(6, ref.edges(voxels, ref.EDGE), None, weight, 4)
    assert labels.tolist() == [-1, -1, -1, 0, 1, 1] and sizes.tolist() == [10, 5] and total == 3
    labels, sizes = ref.components(voxels, ref.EDGE, voxel_weight=weight, min_size=11)
    assert (labels == -1).all() and sizes.shape == (0,) and sizes.dtype == np.int64


def test_the_snake_is_a_path_that_is_not_in_position_order():
    cells = ref.snake_cells()
    n = len(cells)
    assert n >= 4096 and len(np.unique(cells, axis=0)) == n
    assert (np.abs(np.diff(cells, axis=0)).sum(axis=1) == 1).all()                 # consecutive: face neighbors
    assert cells[:, 0].max() >= 32 and cells[:, 1].max() >= 8 and cells[:, 2].max() >= 8      # superblock borders
    order = np.lexsort((cells[:, 0], cells[:, 1], cells[:, 2]))                    # position = address order
    assert (np.diff(order) != 1).sum() > 100
    voxels = centres(cells[order])
    i, j = ref.edges(voxels, ref.EDGE)
    assert len(i) == n - 1                                                         # nothing but the path's steps
    labels, sizes = ref.components(voxels, ref.EDGE)
    assert (labels == 0).all() and sizes.tolist() == [n]
    cut = np.zeros(n, dtype=np.int64)
    cut[np.nonzero(order == 1500)[0][0]] = -1                                      # the path's 1501st cell
    labels, sizes = ref.components(voxels, ref.EDGE, voxel_class=cut)
    assert sorted(sizes.tolist()) == [1500, n - 1501] and (labels == -1).sum() == 1


def test_the_random_lattice_has_the_component_counts_scipy_was_seen_to_find():
    cells = np.unique(ref.random_lattice_cells(), axis=0)
    assert len(cells) == 17991                       # several 4096-entry scan tiles
    voxels = centres(cells)
    found = [len(ref.components(voxels, r * ref.EDGE)[1]) for r in (1.0, 1.5, 2.2)]
    assert found == [8235, 719, 33]


def test_both_symbols_are_declared_bound_and_exported():
    with open(HEADER) as f:
        header = f.read()
    exported = ctypes.CDLL(_ffi.LIBRARY_PATH)
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(exported, name), name
    restype, argtypes = _ffi.SIGNATURES["nm_neighbor_index_components"]
    assert restype is ctypes.c_int and len(argtypes) == 14
    assert _ffi.load().nm_abi_version() == 7 == _ffi.ABI_VERSION


def test_workspace_query_is_monotone_and_zero_on_a_negative_count():
    bytes_for = _ffi.load().nm_neighbor_index_components_workspace_bytes
    assert bytes_for(-1) == 0 and bytes_for(-(1 << 40)) == 0
    sizes = [bytes_for(n) for n in (0, 1, 4095, 4096, 4097, 18000, 10 ** 6, 10 ** 6 + 1, 10 ** 8, (1 << 31) - 1)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert all(s % 16 == 0 for s in sizes)
    assert bytes_for(10 ** 6) >= 24 * 10 ** 6          # address, size, parent and number of every voxel
