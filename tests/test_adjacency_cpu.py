"""
CPU tests (no GPU) of the numpy reference for NeighborIndex.adjacency / prominent_peaks (tests/adjacency_reference.py),
pinned to graphs worked out by hand, and of the library's host merge (nm_merge_by_prominence, called through ctypes:
it makes no GPU call) against that reference.
"""

import numpy as np
import pytest

import adjacency_reference as ref
import components_reference as cref
import hill_climb_reference as href
from nimrud_amd import _ffi

E = ref.EDGE
INF = float("inf")


def row(n):
    voxels = ref.centres(ref.row_cells(n))
    return voxels, cref.edges(voxels, E)


def c_merge(p, pair, saddle, min_prominence):
    """nm_merge_by_prominence itself: (status, root, prom)"""
    lib = _ffi.load()
    p = np.ascontiguousarray(p, dtype=np.float64)
    pair = np.ascontiguousarray(pair, dtype=np.int64).reshape(-1, 2)
    saddle = np.ascontiguousarray(saddle, dtype=np.float64)
    n_seg, n_rows = len(p), len(pair)
    root = np.full(n_seg, -7, dtype=np.int64)
    prom = np.full(n_seg, -7.0)
    scratch = np.zeros(n_seg + n_rows + 1, dtype=np.int64)
    rc = lib.nm_merge_by_prominence(n_seg, p.ctypes.data, n_rows, pair.ctypes.data, saddle.ctypes.data,
                                    float(min_prominence), scratch.ctypes.data, root.ctypes.data, prom.ctypes.data)
    return rc, root, prom


def merge(p, pair, saddle, min_prominence):
    """the reference's (root, prom), which the library's host merge must equal"""
    root, prom = ref.merge_by_prominence(p, pair, saddle, min_prominence)
    rc, got_root, got_prom = c_merge(p, pair, saddle, min_prominence)
    assert rc == _ffi.NM_OK
    assert np.array_equal(got_root, root) and np.array_equal(got_prom, prom, equal_nan=True)
    return root, prom


def peaks_on_row(values, min_prominence, **kwargs):
    voxels, edges = row(len(values))
    value = np.asarray(values, dtype=np.float64)
    out = ref.prominent_peaks_of_edges(voxels, edges, value, min_prominence, **kwargs)
    # the same through the library's host merge
    mode = kwargs.get("mode", "highest")
    cls = kwargs.get("voxel_class")
    labels0, _, peaks0, _, _ = href.hill_climb_of_edges(voxels, edges, value, mode, voxel_class=cls)
    pair, _, saddle = ref.adjacency_of_edges(labels0, edges, value, cls)
    merge(value[peaks0], pair, saddle, min_prominence)
    return out


# ---- a line of five ---------------------------------------------------------------------------------------------------

def test_a_line_of_five():
    voxels, edges = row(5)
    value = np.asarray(ref.LINE_VALUES)
    labels, sizes, peaks, _, _ = href.hill_climb_of_edges(voxels, edges, value, "highest")
    assert labels.tolist() == ref.LINE_LABELS and peaks.tolist() == ref.LINE_PEAKS
    pair, links, saddle = ref.adjacency_of_edges(labels, edges, value)
    assert pair.tolist() == [[0, 1]] and links.tolist() == [1] and saddle.tolist() == [2.0]
    assert pair.dtype == links.dtype == np.int64 and saddle.dtype == np.float64
    # the lower peak's prominence is exactly 1: the test is strict
    for mode in href.MODES:
        labels, sizes, peaks, prom = peaks_on_row(ref.LINE_VALUES, 1.0, mode=mode)
        assert labels.tolist() == [0, 0, 1, 1, 1] and sizes.tolist() == [2, 3] and peaks.tolist() == [1, 3]
        assert prom.tolist() == [1.0, INF]
        labels, sizes, peaks, prom = peaks_on_row(ref.LINE_VALUES, np.nextafter(1.0, 2), mode=mode)
        assert labels.tolist() == [0] * 5 and sizes.tolist() == [5] and peaks.tolist() == [3] and prom.tolist() == [INF]
        # 0 is hill_climb exactly
        got = peaks_on_row(ref.LINE_VALUES, 0.0, mode=mode)
        want = href.hill_climb_of_edges(voxels, edges, value, mode)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
        labels, sizes, peaks, prom = peaks_on_row(ref.LINE_VALUES, INF, mode=mode)
        assert labels.tolist() == [0] * 5 and peaks.tolist() == [3]


# ---- three peaks in a chain ------------------------------------------------------------------------------------------------

def test_three_peaks_in_a_chain():
    a, b, c = 10.0, 8.0, 6.0
    values = ref.chain_values(a, b, c, s_ab=4.0, s_bc=5.0)
    voxels, edges = row(7)
    labels0, _, peaks0, _, _ = href.hill_climb_of_edges(voxels, edges, np.asarray(values), "highest")
    assert labels0.tolist() == [0, 0, 0, 1, 1, 2, 2] and peaks0.tolist() == ref.CHAIN_PEAKS
    pair, links, saddle = ref.adjacency_of_edges(labels0, edges, np.asarray(values))
    assert pair.tolist() == [[0, 1], [1, 2]] and links.tolist() == [1, 1] and saddle.tolist() == [4.0, 5.0]
    # C - s_BC = 1 < 2 <= B - s_AB = 4: C goes to B, B stays
    labels, sizes, peaks, prom = peaks_on_row(values, 2.0)
    assert labels.tolist() == [0, 0, 0, 1, 1, 1, 1] and peaks.tolist() == [1, 3] and prom.tolist() == [INF, 4.0]
    # both merge: C into B at saddle 5, then B (with C) into A at saddle 4
    labels, sizes, peaks, prom = peaks_on_row(values, 4.5)
    assert labels.tolist() == [0] * 7 and peaks.tolist() == [1] and sizes.tolist() == [7] and prom.tolist() == [INF]
    # exactly at B's prominence: strict, B stays
    assert peaks_on_row(values, 4.0)[2].tolist() == [1, 3]
    # nothing merges below C's prominence; the prominences are the first failures
    labels, sizes, peaks, prom = peaks_on_row(values, 1.0)
    assert peaks.tolist() == ref.CHAIN_PEAKS and prom.tolist() == [INF, 4.0, 1.0]
    # a row is judged by the ROOTS it joins: B = 6 between A = 10 and C = 8 (the pass voxel 4 climbs to C).  (A, B) at
    # 5.5 comes first: B's rise 0.5 < 1, B goes to A; then (B, C) at 5 joins the roots A and C: C's rise is 3
    values = ref.chain_values(10.0, 6.0, 8.0, s_ab=5.5, s_bc=5.0)
    labels, sizes, peaks, prom = peaks_on_row(values, 1.0)
    assert labels.tolist() == [0, 0, 0, 0, 1, 1, 1] and peaks.tolist() == [1, 5] and prom.tolist() == [INF, 3.0]


def test_a_row_that_fails_and_a_lower_row_between_the_same_roots():
    # A, B, C, D = 10, 8, 6, 5.5.  (C, D) at 5.4: D's rise 0.1 < 1, D goes to C.  (B, C) at 4: C's rise 2 >= 1 fails,
    # recorded.  (B, D) at 3 lies between the SAME roots B and C: it fails again, and C's prominence stays the first, 2
    p = [10.0, 8.0, 6.0, 5.5]
    pair = [[0, 1], [1, 2], [1, 3], [2, 3]]
    saddle = [1.0, 4.0, 3.0, 5.4]
    root, prom = merge(p, pair, saddle, 1.0)
    assert root.tolist() == [0, 1, 2, 2]
    assert prom[0] == INF and prom[1] == 7.0 and prom[2] == 2.0 and prom[3] == pytest.approx(0.1, abs=1e-12)
    # with the threshold above both: everything ends in A
    root, prom = merge(p, pair, saddle, 8.0)
    assert root.tolist() == [0, 0, 0, 0] and prom[0] == INF


def test_equal_saddles_are_taken_in_pair_order():
    # C = 3 touches A = 6 and B = 7 at the same saddle 2: the row (A, C) comes first, C goes to A - not to the higher
    # B, where merging all low roots of a level into the highest at once would send it
    root, prom = merge([6.0, 7.0, 3.0], [[0, 2], [1, 2]], [2.0, 2.0], 2.0)
    assert root.tolist() == [0, 1, 0] and prom.tolist() == [4.0, INF, 1.0]
    # the segments renumbered so that the other row comes first: now C goes to B
    root, prom = merge([7.0, 6.0, 3.0], [[0, 2], [1, 2]], [2.0, 2.0], 2.0)
    assert root.tolist() == [0, 1, 0] and prom.tolist() == [INF, 4.0, 1.0]
    # equal peaks: the smaller number is the higher one
    root, prom = merge([5.0, 5.0], [[0, 1]], [4.5], 1.0)
    assert root.tolist() == [0, 0]
    # -0 and +0 are one saddle: the pair order decides, not the sign
    root, _ = merge([6.0, 7.0, 3.0], [[0, 2], [1, 2]], [-0.0, 0.0], 4.0)
    assert root.tolist() == [0, 1, 0]
    root, _ = merge([6.0, 7.0, 3.0], [[0, 2], [1, 2]], [0.0, -0.0], 4.0)
    assert root.tolist() == [0, 1, 0]


# ---- further cases -------------------------------------------------------------------------------------------------------------

def test_a_plateau():
    # the U of hill_climb's tests: one plateau, two peaks of equal value; the pass between them lies at the same value
    voxels = ref.centres(href.u_cells())
    edges = cref.edges(voxels, E)
    value = np.zeros(13)
    labels0, _, peaks0, _, _ = href.hill_climb_of_edges(voxels, edges, value, "highest")
    assert labels0.tolist() == href.U_LABELS
    pair, links, saddle = ref.adjacency_of_edges(labels0, edges, value)
    assert pair.tolist() == [[0, 1]] and links.tolist() == [1] and saddle.tolist() == [0.0]
    labels, sizes, peaks, prom = ref.prominent_peaks_of_edges(voxels, edges, value, 0.0)
    assert labels.tolist() == href.U_LABELS and prom.tolist() == [INF, 0.0]
    # any threshold above 0 makes it one: the peak of the smaller position is the higher
    labels, sizes, peaks, prom = ref.prominent_peaks_of_edges(voxels, edges, value, 5e-324)
    assert labels.tolist() == [0] * 13 and peaks.tolist() == [0] and sizes.tolist() == [13]


def test_classes_nan_and_labels_outside():
    voxels, edges = row(5)
    value = np.asarray(ref.LINE_VALUES)
    labels = np.asarray(ref.LINE_LABELS)
    # two classes side by side: no row across
    for cls in ([0, 0, 1, 1, 1], [0, 0, -1, 1, 1], [3, 3, 2, 2, 2]):
        pair, links, saddle = ref.adjacency_of_edges(labels, edges, value, cls)
        assert pair.shape == (0, 2) and links.shape == (0,) and saddle.shape == (0,)
    pair, links, saddle = ref.adjacency_of_edges(labels, edges, value, [4, 4, 4, 4, 4])
    assert pair.tolist() == [[0, 1]]
    # a negative class on both sides is no class
    assert len(ref.adjacency_of_edges(labels, edges, value, [0, -1, -1, 0, 0])[0]) == 0
    # a NaN voxel on the only bridge: no row - and hill_climb itself leaves it out
    nan = np.asarray([1.0, 3.0, np.nan, 5.0, 4.0])
    labels0 = href.hill_climb_of_edges(voxels, edges, nan, "highest")[0]
    assert labels0.tolist() == [0, 0, -1, 1, 1]
    assert len(ref.adjacency_of_edges(labels0, edges, nan)[0]) == 0
    assert len(ref.adjacency_of_edges([0, 0, 1, 1, 1], edges, nan)[0]) == 0
    # labels with -1: the voxel is in no segment
    assert len(ref.adjacency_of_edges([0, 0, -1, 1, 1], edges, value)[0]) == 0
    pair, links, saddle = ref.adjacency_of_edges([2, -1, 7, 7, 0], edges, value)
    assert pair.tolist() == [[0, 7]] and links.tolist() == [1] and saddle.tolist() == [4.0]
    # without values: no saddle, the same rows
    pair, links, saddle = ref.adjacency_of_edges(labels, edges)
    assert pair.tolist() == [[0, 1]] and links.tolist() == [1] and saddle is None
    # one label for all: nothing crosses
    assert len(ref.adjacency_of_edges(np.zeros(5, dtype=np.int64), edges, value)[0]) == 0


def test_a_pair_joined_by_several_edges():
    # a row of four at two edges: {0,1} {0,2} {1,2} {1,3} {2,3}; labels 0 0 1 1: three edges cross, met in the order
    # {0,2}, {1,2}, {1,3} with the passes 1, 2, 4: the saddle is the maximum, not the first
    voxels = ref.centres(ref.row_cells(4))
    edges = cref.edges(voxels, 2 * E)
    assert len(edges[0]) == 5
    pair, links, saddle = ref.adjacency_of_edges([0, 0, 1, 1], edges, [1.0, 5.0, 2.0, 4.0])
    assert pair.tolist() == [[0, 1]] and links.tolist() == [3] and saddle.tolist() == [4.0]
    # the pair is unordered: labels the other way round are the same row
    pair, links, saddle = ref.adjacency_of_edges([1, 1, 0, 0], edges, [1.0, 5.0, 2.0, 4.0])
    assert pair.tolist() == [[0, 1]] and links.tolist() == [3] and saddle.tolist() == [4.0]
    # three labels: rows ascend by (a, b)
    pair, links, saddle = ref.adjacency_of_edges([5, 0, 5, 3], edges, [1.0, 5.0, 2.0, 4.0])
    assert pair.tolist() == [[0, 3], [0, 5], [3, 5]] and links.tolist() == [1, 2, 1]
    assert saddle.tolist() == [4.0, 2.0, 2.0]


def test_min_size_acts_after_the_merge():
    voxels, edges = row(5)
    value = np.asarray(ref.LINE_VALUES)
    # hill_climb alone drops the small peak
    labels, sizes, peaks, _, _ = href.hill_climb_of_edges(voxels, edges, value, "highest", min_size=3)
    assert labels.tolist() == [-1, -1, 0, 0, 0] and sizes.tolist() == [3]
    # merged into the big one it lives on inside it
    labels, sizes, peaks, prom = peaks_on_row(ref.LINE_VALUES, 2.0, min_size=3)
    assert labels.tolist() == [0] * 5 and sizes.tolist() == [5] and peaks.tolist() == [3]
    # not merged it is dropped as before, and the numbering closes up
    labels, sizes, peaks, prom = peaks_on_row(ref.LINE_VALUES, 0.5, min_size=3)
    assert labels.tolist() == [-1, -1, 0, 0, 0] and sizes.tolist() == [3] and peaks.tolist() == [3]
    assert prom.tolist() == [INF]
    # weights: sizes are their sums
    labels, sizes, peaks, prom = peaks_on_row(ref.LINE_VALUES, 0.5, voxel_weight=[4, 4, 1, 1, 1], min_size=4)
    assert labels.tolist() == [0, 0, -1, -1, -1] and sizes.tolist() == [8] and prom.tolist() == [1.0]


def test_partitions():
    assert ref.same_partition([0, 0, 1, -1], [3, 3, 0, -1])
    assert not ref.same_partition([0, 0, 1, -1], [3, 3, 3, -1])
    assert not ref.same_partition([0, 0, 1, -1], [0, 1, 2, -1])
    assert not ref.same_partition([0, 0, 1, -1], [0, 0, 1, 1])


# ---- the host merge of the library ------------------------------------------------------------------------------------------

def test_the_host_merge_on_random_graphs():
    rng = np.random.default_rng(5)
    merged = 0
    for trial in range(300):
        n_seg = int(rng.integers(1, 13))
        p, pair, saddle = ref.random_segment_graph(rng, n_seg)
        for tau in (0.0, 1.0, 2.0, 3.5, INF):
            root, prom = merge(p, pair, saddle, tau)
            merged += int((root != np.arange(n_seg)).sum())
            if tau == 0.0:
                assert np.array_equal(root, np.arange(n_seg))
    assert merged > 1000
    # the rows in any order give the same result: the function orders them itself
    p, pair, saddle = ref.random_segment_graph(rng, 12)
    shuffle = rng.permutation(len(pair))
    want = ref.merge_by_prominence(p, pair, saddle, 2.0)
    rc, root, prom = c_merge(p, pair[shuffle], saddle[shuffle], 2.0)
    assert rc == _ffi.NM_OK and np.array_equal(root, want[0]) and np.array_equal(prom, want[1])


def test_the_host_merge_checks_its_arguments():
    p, pair, saddle = [3.0, 2.0], [[0, 1]], [1.0]
    assert c_merge(p, pair, saddle, 1.0)[0] == _ffi.NM_OK
    for tau in (-1.0, float("nan"), -INF):
        rc, root, prom = c_merge(p, pair, saddle, tau)
        assert rc == _ffi.NM_ERR_INVALID and (root == -7).all() and (prom == -7.0).all()
    for bad_pair in ([[1, 0]], [[0, 0]], [[0, 2]], [[-1, 1]]):
        assert c_merge(p, bad_pair, saddle, 1.0)[0] == _ffi.NM_ERR_INVALID
    assert c_merge(p, pair, [float("nan")], 1.0)[0] == _ffi.NM_ERR_INVALID
    assert c_merge([3.0, float("nan")], pair, saddle, 1.0)[0] == _ffi.NM_ERR_INVALID
    # no segments, no rows
    rc, root, prom = c_merge([], np.zeros((0, 2)), [], 1.0)
    assert rc == _ffi.NM_OK and len(root) == 0
    rc, root, prom = c_merge([1.0, 2.0, 3.0], np.zeros((0, 2)), [], INF)
    assert rc == _ffi.NM_OK and root.tolist() == [0, 1, 2] and (prom == INF).all()


def test_workspace_query_needs_no_gpu():
    lib = _ffi.load()
    query = lib.nm_neighbor_index_adjacency_workspace_bytes
    assert 0 < query(0, 0) <= query(1000, 0) < query(100000, 0) < query(100000, 10000000)
    assert query(0, 0) == query(1, 1)
    assert query(-1, 0) == 0 and query(0, -1) == 0 and query(1 << 31, 0) == 0 and query(0, 1 << 31) == 0
