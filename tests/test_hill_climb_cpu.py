"""
CPU tests for NeighborIndex.hill_climb: they pin the yardstick the GPU tests (test_hill_climb_gpu.py) are measured
against - the numpy reference of tests/hill_climb_reference.py - to graphs labelled by hand (a ramp, two bumps and a
saddle, plateaus, a case where the two modes differ, voxels out of the graph, min_size), check that the inputs of the
GPU tests are not trivial, and that the library declares, binds and exports the new symbols under ABI 7.
"""

import ctypes
import os

import numpy as np
import pytest

import components_reference as cref
import dbscan_reference as dref
import hill_climb_reference as ref
import regions_reference as rref
from nimrud_amd import _ffi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nimrud_hip.h")
SYMBOLS = ("nm_neighbor_index_hill_climb", "nm_neighbor_index_hill_climb_workspace_bytes")
E = ref.EDGE


# ---- 1. graphs labelled by hand -------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ref.MODES)
def test_a_ramp_is_one_segment_and_every_link_points_to_the_next_voxel(mode):
    row = ref.centres(ref.row_cells(7))
    labels, sizes, peaks, link = ref.hill_climb(row, E, ref.RAMP_VALUES, mode)
    assert labels.tolist() == [0] * 7 and sizes.tolist() == [7] and peaks.tolist() == [6]
    assert link.tolist() == [1, 2, 3, 4, 5, 6, 6]
    # downhill: the peak is position 0 and the links run the other way
    labels, sizes, peaks, link = ref.hill_climb(row, E, ref.RAMP_VALUES[::-1], mode)
    assert peaks.tolist() == [0] and link.tolist() == [0, 0, 1, 2, 3, 4, 5]
    # at three edges "highest" jumps three voxels at a time, "nearest" still steps to the next one
    labels, sizes, peaks, link = ref.hill_climb(row, 3 * E, ref.RAMP_VALUES, mode)
    assert link.tolist() == ([3, 4, 5, 6, 6, 6, 6] if mode == "highest" else [1, 2, 3, 4, 5, 6, 6])
    assert labels.tolist() == [0] * 7 and peaks.tolist() == [6]


@pytest.mark.parametrize("mode", ref.MODES)
def test_two_bumps_joined_by_a_saddle_are_one_component_and_two_segments(mode):
    row = ref.centres(ref.row_cells(7))
    assert cref.components(row, E)[1].tolist() == [7]                     # connectivity welds them
    labels, sizes, peaks, link = ref.hill_climb(row, E, ref.BUMPS_VALUES, mode)
    # the saddle (3) sees the slopes 2 and 4: equal value, equal d2 - the smaller position in both modes
    assert link.tolist() == ref.BUMPS_LINK_1 and labels.tolist() == ref.BUMPS_LABELS_1
    assert sizes.tolist() == [4, 3] and peaks.tolist() == [1, 5]
    # at two edges it sees both peaks: "highest" takes the higher one, "nearest" keeps the slope
    labels, sizes, peaks, link = ref.hill_climb(row, 2 * E, ref.BUMPS_VALUES, mode)
    assert link.tolist() == ref.BUMPS_LINK_2[mode] and labels.tolist() == ref.BUMPS_LABELS_2[mode]
    assert peaks.tolist() == [1, 5] and sizes.sum() == 7
    # mirrored values mirror the tie: the saddle still goes to the smaller POSITION, now the other bump
    labels, sizes, peaks, link = ref.hill_climb(row, E, ref.BUMPS_VALUES[::-1], mode)
    assert link.tolist() == [1, 1, 1, 2, 5, 5, 5] and labels.tolist() == [0, 0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("mode", ref.MODES)
def test_a_plateau_climbs_to_its_smallest_position_and_may_split_where_it_is_not_convex(mode):
    ell = ref.centres(ref.plateau_cells())
    flat = np.full(len(ell), 2.5)
    for rho in (1.0, 2.0):
        labels, sizes, peaks, link = ref.hill_climb(ell, rho * E, flat, mode)
        assert labels.tolist() == [0] * 9 and sizes.tolist() == [9] and peaks.tolist() == [0]
    labels, sizes, peaks, link = ref.hill_climb(ell, E, flat, mode)
    assert link.tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7]
    # -0 and +0 are equal: still one plateau
    zeros = np.where(np.arange(9) % 2 == 0, 0.0, -0.0)
    assert ref.hill_climb(ell, E, zeros, mode)[3].tolist() == link.tolist()
    # a U is one component and one plateau, and two segments: documented, not a defect
    u = ref.centres(ref.u_cells())
    assert cref.components(u, E)[1].tolist() == [13]
    labels, sizes, peaks, link = ref.hill_climb(u, E, np.zeros(13), mode)
    assert labels.tolist() == ref.U_LABELS and peaks.tolist() == ref.U_PEAKS and sizes.tolist() == [9, 4]
    assert link[12] == 7                                                  # (4, 3) and (3, 4) tie: the smaller position


def test_highest_and_nearest_give_different_links():
    row = ref.centres(ref.row_cells(3))
    for mode in ref.MODES:
        labels, sizes, peaks, link = ref.hill_climb(row, 2 * E, ref.DIFFER_VALUES, mode)
        assert link.tolist() == ref.DIFFER_LINK[mode] and labels.tolist() == [0, 0, 0] and peaks.tolist() == [2]
    # "highest": among equal values the smaller d2; "nearest": among equal d2 the larger value
    row = ref.centres(ref.row_cells(5))
    assert ref.hill_climb(row, 2 * E, [9.0, 0.0, 0.0, 9.0, 9.0], "highest")[3].tolist() == [0, 0, 3, 3, 3]
    assert ref.hill_climb(row, 2 * E, [5.0, 0.0, 1.0, 0.0, 7.0], "nearest")[3].tolist() == [0, 0, 4, 4, 4]
    assert ref.hill_climb(row, E, [5.0, 0.0, 1.0, 0.0, 7.0], "nearest")[3].tolist() == [0, 0, 2, 4, 4]


@pytest.mark.parametrize("mode", ref.MODES)
def test_nan_values_and_negative_classes_are_out_of_the_graph(mode):
    row = ref.centres(ref.row_cells(7))
    nan = float("nan")
    # a NaN in the ramp: nobody's candidate, no label, no link - the ramp breaks in two at one edge
    labels, sizes, peaks, link = ref.hill_climb(row, E, [0.0, 1.0, 2.0, nan, 4.0, 5.0, 6.0], mode)
    assert labels.tolist() == [0, 0, 0, -1, 1, 1, 1] and link.tolist() == [1, 2, 2, -1, 5, 6, 6]
    assert sizes.tolist() == [3, 3] and peaks.tolist() == [2, 6]
    # a negative class does the same; other classes link among themselves only
    labels, sizes, peaks, link = ref.hill_climb(row, E, ref.RAMP_VALUES, mode, voxel_class=[0, 0, 0, -1, 0, 0, 0])
    assert labels.tolist() == [0, 0, 0, -1, 1, 1, 1] and link.tolist() == [1, 2, 2, -1, 5, 6, 6]
    labels, sizes, peaks, link = ref.hill_climb(row, 2 * E, ref.RAMP_VALUES, mode, voxel_class=[0, 1, 0, 1, 0, 1, 0])
    assert link.tolist() == [2, 3, 4, 5, 6, 5, 6] and labels.tolist() == [1, 0, 1, 0, 1, 0, 1]
    assert peaks.tolist() == [5, 6] and sizes.tolist() == [3, 4]
    # infinities are values like any other
    labels, sizes, peaks, link = ref.hill_climb(row, E, [-np.inf, -np.inf, 0.0, np.inf, np.inf, 1.0, 2.0], mode)
    assert link.tolist() == [0, 2, 3, 3, 3, 4, 6] and peaks.tolist() == [0, 3, 6]


@pytest.mark.parametrize("mode", ref.MODES)
def test_min_size_drops_a_segment_and_renumbers(mode):
    row = ref.centres(ref.row_cells(7))
    weight = [1, 1, 1, 1, 5, 5, 5]
    labels, sizes, peaks, link, total = ref.hill_climb_of_edges(row, cref.edges(row, E), ref.BUMPS_VALUES, mode,
                                                                voxel_weight=weight, min_size=5)
    assert labels.tolist() == [-1, -1, -1, -1, 0, 0, 0] and sizes.tolist() == [15] and peaks.tolist() == [5]
    assert total == 2 and link.tolist() == ref.BUMPS_LINK_1                # the links do not depend on min_size
    labels, sizes, peaks, link, total = ref.hill_climb_of_edges(row, cref.edges(row, E), ref.BUMPS_VALUES, mode,
                                                                voxel_weight=weight, min_size=16)
    assert (labels == -1).all() and len(sizes) == 0 and len(peaks) == 0 and total == 2


# ---- 2. the inputs of the GPU tests are not trivial ----------------------------------------------------------------------

def test_the_lattice_inputs_exercise_ties_chains_and_more_than_one_peak():
    voxels = cref.voxels_of(rref.lattice_cloud("thin"), E)
    assert len(voxels) == 9481
    pairs = cref.edges(voxels, 1.5 * E)
    m = len(voxels)
    smooth, levels = ref.smooth_values(voxels), ref.quantised_values(voxels)
    assert sorted(set(levels.tolist())) == [0.0, 1.0, 2.0, 3.0]
    out = {}
    for name, value in (("smooth", smooth), ("levels", levels)):
        for mode in ref.MODES:
            labels, sizes, peaks, link, total = ref.hill_climb_of_edges(voxels, pairs, value, mode)
            assert (labels >= 0).all() and sizes.sum() == m and total == len(sizes) > 1
            assert (np.diff(peaks) > 0).all() and (link[peaks] == peaks).all()
            out[name, mode] = link
    # the modes disagree on both value sets, and on the levels most links stay on a plateau: ties decide them
    for name in ("smooth", "levels"):
        assert (out[name, "highest"] != out[name, "nearest"]).any(), name
    for mode in ref.MODES:
        link = out["levels", mode]
        assert (levels[link] == levels).sum() > m // 2
    # value = x, "nearest", three edges (the gaps of the lattice are bridged): a chain along the whole lattice
    labels, sizes, peaks, link, total = ref.hill_climb_of_edges(voxels, cref.edges(voxels, 3.0 * E), voxels[:, 0].copy(),
                                                                "nearest")
    steps, at = 0, np.arange(m)
    while (link[at] != at).any():
        at = link[at]
        steps += 1
    print("value = x, nearest, 3 edges: %d peaks, the longest chain has %d links" % (total, steps))
    assert steps >= 700 and total == 2


def test_a_monotone_map_of_the_values_changes_nothing():
    voxels = cref.voxels_of(rref.lattice_cloud("random"), E)[:3000]
    pairs = cref.edges(voxels, 1.5 * E)
    levels = ref.quantised_values(voxels)
    cls = ref.case_classes(len(voxels))
    weight = dref.case_weights(len(voxels))
    for mode in ref.MODES:
        a = ref.hill_climb_of_edges(voxels, pairs, levels, mode, cls, weight, 9)
        b = ref.hill_climb_of_edges(voxels, pairs, 2.0 * levels + 1.0, mode, cls, weight, 9)
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
        assert (a[0][cls < 0] == -1).all() and (a[3][cls < 0] == -1).all() and len(a[1]) < a[4]
        # every segment inside one component of the same graph
        comp = cref.components_of_edges(len(voxels), pairs, cls)[0]
        inside = a[3] >= 0
        assert np.array_equal(comp[a[3][inside]], comp[inside])


# ---- 3. the ABI ---------------------------------------------------------------------------------------------------------

def test_both_symbols_are_declared_bound_and_exported():
    with open(HEADER) as f:
        header = f.read()
    exported = ctypes.CDLL(_ffi.LIBRARY_PATH)
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(exported, name), name
    restype, argtypes = _ffi.SIGNATURES["nm_neighbor_index_hill_climb"]
    assert restype is ctypes.c_int and len(argtypes) == 18
    assert "enum { NM_CLIMB_HIGHEST = 0, NM_CLIMB_NEAREST = 1 };" in header
    assert _ffi.NM_CLIMB == {"highest": 0, "nearest": 1}
    assert "value[u] > value[v] || (value[u] == value[v] && u < v)" in header
    assert _ffi.load().nm_abi_version() == 7 == _ffi.ABI_VERSION


def test_workspace_query_is_a_host_function_that_grows_with_m():
    lib = _ffi.load()
    bytes_for = lib.nm_neighbor_index_hill_climb_workspace_bytes
    assert bytes_for(-1) == 0 and bytes_for(-(1 << 40)) == 0 and bytes_for(1 << 31) == 0
    counts = (0, 1, 4095, 4096, 4097, 18000, 10 ** 6, 10 ** 6 + 1, 10 ** 8, (1 << 31) - 1)
    sizes = [bytes_for(n) for n in counts]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert all(s % 16 == 0 for s in sizes)
    # the scratch of components: the forest is its parent[] array, nothing more is needed
    assert sizes == [lib.nm_neighbor_index_components_workspace_bytes(n) for n in counts]
