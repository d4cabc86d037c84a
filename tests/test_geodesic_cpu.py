"""
CPU tests for NeighborIndex.geodesic: they pin the yardstick the GPU tests (test_geodesic_gpu.py) are measured against -
the numpy reference of tests/geodesic_reference.py - to scipy's Dijkstra on the fp64 bits and to graphs worked by hand
(a row, a horseshoe, a staircase, two seeds with a tie, classes, a limit, sizes), and check that the library declares,
binds and exports the new symbols under ABI 7 and answers what needs no device.
"""

import ctypes
import math
import os

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import dijkstra

import components_reference as cref
import geodesic_reference as ref
import regions_reference as rref
from nimrud_amd import _ffi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nimrud_hip.h")
SYMBOLS = ("nm_neighbor_index_geodesic_workspace_bytes", "nm_neighbor_index_geodesic_relax",
           "nm_neighbor_index_geodesic_finish")
E = ref.EDGE
INF = ref.INF


def scipy_distances(m, edges, voxel_seed, voxel_class=None):
    """scipy.sparse.csgraph.dijkstra from all seeds of the graph at once, on the reference's directed edges"""
    src, dst, w = edges
    seeds = np.nonzero(ref.start(m, voxel_seed, voxel_class) == 0.0)[0]
    if len(seeds) == 0:
        return np.full(m, INF)
    graph = coo_matrix((w, (src, dst)), shape=(m, m)).tocsr()
    return dijkstra(graph, directed=True, indices=seeds, min_only=True)


@pytest.fixture(scope="module")
def lattice():
    voxels = cref.voxels_of(rref.lattice_cloud("random"), E)
    assert len(voxels) == 17991
    return voxels, {rho: cref.edges(voxels, rho * E) for rho in (1.0, 2.0, 3.0)}


# ---- 1. the fixpoint is Dijkstra's answer, bit for bit ----------------------------------------------------------------

def test_the_fixpoint_is_scipys_dijkstra_on_the_shared_cases(lattice):
    voxels, pairs = lattice
    m = len(voxels)
    for rho, seeds, classes, limited in ref.LATTICE_CASES:
        seed = ref.case_seeds(m, seeds)
        cls = ref.case_classes(m) if classes else None
        edges = ref.directed_edges(voxels, pairs[rho], cls)
        # w is symmetric bit for bit and one edge long or more (up to the rounding of the centres): never 0
        src, dst, w = edges
        back = np.lexsort((dst, src))
        assert np.array_equal(src[back], dst) and np.array_equal(ref.bits(w[back]), ref.bits(w))
        assert (w >= E * (1.0 - 1e-12)).all()
        dist, sweeps = ref.distances(m, edges, seed, cls)
        want = scipy_distances(m, edges, seed, cls)
        assert np.array_equal(ref.bits(dist), ref.bits(want)), (rho, seeds, classes)
        reached = int((dist < INF).sum())
        print("r = %g edges, %d seeds, classes %s: %d of %d reached in %d sweeps" % (rho, seeds, classes, reached, m,
                                                                                  sweeps))
        assert reached >= seeds - (0 if cls is None else int((cls[seed] < 0).sum()))
        if limited:
            # a limit cuts the unlimited answer off and changes nothing below it: every prefix of a path is shorter
            limit = ref.median_distance(dist)
            cut, _ = ref.distances(m, edges, seed, cls, limit)
            assert np.array_equal(ref.bits(cut), ref.bits(np.where(dist <= limit, dist, INF)))
            assert (cut == limit).any()
    # the cases are not trivial: at two and three edges a single seed reaches most of the lattice over many sweeps
    dist, sweeps = ref.distances(m, ref.directed_edges(voxels, pairs[2.0]), ref.case_seeds(m, 1))
    assert (dist < INF).sum() > m // 2 and sweeps > 20


def test_links_segments_and_sources_on_a_lattice_case(lattice):
    voxels, pairs = lattice
    m = len(voxels)
    seed, cls = ref.case_seeds(m, 200), ref.case_classes(m)
    weight = np.random.default_rng(3).integers(1, 6, m)
    dist, labels, sizes, sources, link, total, _ = ref.geodesic_of_edges(voxels, pairs[2.0], seed, voxel_class=cls,
                                                                        voxel_weight=weight, min_size=40)
    in_graph = cls >= 0
    assert total == (seed & in_graph).sum() and 0 < len(sizes) < total
    assert np.array_equal(np.nonzero(link == np.arange(m))[0], np.nonzero(seed & in_graph)[0])
    assert np.array_equal(link >= 0, dist < INF) and (dist[~in_graph] == INF).all()
    # links strictly descend the order, stay in the class, and a voxel shares its link's segment
    at = np.nonzero((link >= 0) & (link != np.arange(m)))[0]
    up = link[at]
    assert ((dist[up] < dist[at]) | ((dist[up] == dist[at]) & (up < at))).all()
    assert np.array_equal(cls[up], cls[at]) and np.array_equal(labels[up], labels[at])
    assert (np.diff(sources) > 0).all() and np.array_equal(labels[sources], np.arange(len(sources)))
    assert sizes.min() >= 40 and np.array_equal(np.bincount(labels[labels >= 0], weights=weight[labels >= 0]), sizes)
    # labels >= 0 (before min_size) exactly on the components that hold a seed
    labels1 = ref.segments(dist, link)[0]
    comp = cref.components_of_edges(m, pairs[2.0], cls)[0]
    seeded = np.zeros(comp.max() + 1, dtype=bool)
    seeded[comp[seed & in_graph]] = True
    assert np.array_equal(labels1 >= 0, in_graph & seeded[np.maximum(comp, 0)])


# ---- 2. graphs worked by hand ---------------------------------------------------------------------------------------------

def running_sum(voxels, path):
    """the left-to-right rounded length of a path of positions"""
    total, out = 0.0, [0.0]
    for a, b in zip(path[:-1], path[1:]):
        dx, dy, dz = voxels[b] - voxels[a]
        total = total + math.sqrt((dx * dx + dy * dy) + dz * dz)
        out.append(total)
    return out


def test_a_row():
    row = ref.centres(ref.row_cells(6))
    seed = [1, 0, 0, 0, 0, 0]
    dist, labels, sizes, sources, link = ref.geodesic(row, E, seed)
    assert dist.tolist() == running_sum(row, range(6)) == [0.0, E, 2 * E, 3 * E, 4 * E, 5 * E]
    assert link.tolist() == [0, 0, 1, 2, 3, 4] and labels.tolist() == [0] * 6
    assert sizes.tolist() == [6] and sources.tolist() == [0]
    # from the other end the links run the other way
    dist, labels, sizes, sources, link = ref.geodesic(row, E, seed[::-1])
    assert link.tolist() == [1, 2, 3, 4, 5, 5] and sources.tolist() == [5] and dist[0] == 5 * E
    # at two edges every second voxel is one step: the same distances, over fewer links
    dist, labels, sizes, sources, link = ref.geodesic(row, 2 * E, seed)
    assert dist.tolist() == [0.0, E, 2 * E, 3 * E, 4 * E, 5 * E] and link.tolist() == [0, 0, 0, 1, 2, 3]


def test_a_horseshoe_is_walked_round_and_a_larger_radius_jumps_the_gap():
    u = ref.centres(ref.horseshoe_cells())
    seed = [1, 0, 0, 0, 0, 0, 0]
    dist, labels, sizes, sources, link = ref.geodesic(u, E, seed)
    assert link.tolist() == ref.HORSESHOE_LINK_1
    assert dist[1] == 6 * E and np.linalg.norm(u[1] - u[0]) == 2 * E     # round the bend, not across
    assert dist.tolist() == [0.0, 6 * E, E, 5 * E, 2 * E, 3 * E, 4 * E]
    dist, labels, sizes, sources, link = ref.geodesic(u, 2 * E, seed)
    assert link.tolist() == ref.HORSESHOE_LINK_2 and dist[1] == 2 * E
    assert dist[5] == E + math.sqrt(2 * E * E) and dist[6] == dist[5] + E and dist[3] == 3 * E


def test_a_staircase_takes_the_diagonal():
    steps = ref.centres(ref.staircase_cells())
    dist, labels, sizes, sources, link = ref.geodesic(steps, 1.5 * E, [1, 0, 0, 0, 0])
    diagonal = math.sqrt(2 * E * E)
    assert dist.tolist() == [0.0, E, diagonal, E + diagonal, diagonal + diagonal] and diagonal < 2 * E
    assert E + diagonal == diagonal + E and link.tolist() == ref.STAIRCASE_LINK
    # at one edge there is no diagonal
    dist, labels, sizes, sources, link = ref.geodesic(steps, E, [1, 0, 0, 0, 0])
    assert dist.tolist() == [0.0, E, 2 * E, 3 * E, 4 * E] and link.tolist() == [0, 0, 1, 2, 3]


def test_two_seeds_a_tie_goes_to_the_smaller_position():
    row = ref.centres(ref.row_cells(7))
    dist, labels, sizes, sources, link = ref.geodesic(row, E, [1, 0, 0, 0, 0, 0, 1])
    # the middle voxel is three steps from either seed, bit for bit: its candidates 2 and 4 tie, 2 is taken
    assert ref.bits(dist[2] + E) == ref.bits(dist[4] + E) == ref.bits(dist[3]) and dist[2] == dist[4]
    assert link.tolist() == [0, 0, 1, 2, 5, 6, 6] and labels.tolist() == [0, 0, 0, 0, 1, 1, 1]
    assert sizes.tolist() == [4, 3] and sources.tolist() == [0, 6]
    # an even row, the seeds off-centre: the split is where the distances say
    row = ref.centres(ref.row_cells(8))
    dist, labels, sizes, sources, link = ref.geodesic(row, E, [1, 0, 0, 0, 0, 1, 0, 0])
    assert labels.tolist() == [0, 0, 0, 1, 1, 1, 1, 1] and link.tolist() == [0, 0, 1, 4, 5, 5, 5, 6]
    assert dist.tolist() == [0.0, E, 2 * E, 2 * E, E, 0.0, E, 2 * E]


def test_classes_seeds_and_islands():
    row = ref.centres(ref.row_cells(7))
    seed = [1, 0, 0, 0, 0, 0, 0]
    # a class wall blocks the path; a negative class is out of the graph
    for wall in (1, -1):
        dist, labels, sizes, sources, link = ref.geodesic(row, E, seed, voxel_class=[0, 0, 0, wall, 0, 0, 0])
        assert dist.tolist() == [0.0, E, 2 * E, INF, INF, INF, INF]
        assert labels.tolist() == [0, 0, 0, -1, -1, -1, -1] and link.tolist() == [0, 0, 1, -1, -1, -1, -1]
    # at two edges the wall is stepped over, and the wall's own class has no seed
    dist, labels, sizes, sources, link = ref.geodesic(row, 2 * E, seed, voxel_class=[0, 0, 0, 1, 0, 0, 0])
    assert dist.tolist() == [0.0, E, 2 * E, INF, 4 * E, 5 * E, 6 * E] and link.tolist() == [0, 0, 0, -1, 2, 4, 4]
    # a seed of negative class is ignored
    dist, labels, sizes, sources, link = ref.geodesic(row, E, [1, 0, 0, 0, 0, 0, 1], voxel_class=[0] * 6 + [-1])
    assert dist.tolist() == [0.0, E, 2 * E, 3 * E, 4 * E, 5 * E, INF] and sources.tolist() == [0]
    # an island without a seed, no seed at all, every voxel a seed
    gap = ref.centres([(0, 0, 0), (1, 0, 0), (3, 0, 0), (4, 0, 0)])
    dist, labels, sizes, sources, link = ref.geodesic(gap, E, [1, 0, 0, 0])
    assert dist.tolist() == [0.0, E, INF, INF] and labels.tolist() == [0, 0, -1, -1] and link.tolist() == [0, 0, -1, -1]
    dist, labels, sizes, sources, link = ref.geodesic(gap, E, [0, 0, 0, 0])
    assert (dist == INF).all() and (labels == -1).all() and (link == -1).all() and len(sizes) == len(sources) == 0
    dist, labels, sizes, sources, link = ref.geodesic(gap, E, [1, 2, 255, 1])
    assert (dist == 0.0).all() and labels.tolist() == link.tolist() == sources.tolist() == [0, 1, 2, 3]


def test_max_distance_is_inclusive_and_nothing_is_reached_through_what_lies_beyond():
    row = ref.centres(ref.row_cells(7))
    seed = [1, 0, 0, 0, 0, 0, 0]
    dist, labels, sizes, sources, link = ref.geodesic(row, E, seed, max_distance=3 * E)
    assert dist.tolist() == [0.0, E, 2 * E, 3 * E, INF, INF, INF] and labels.tolist() == [0, 0, 0, 0, -1, -1, -1]
    assert link.tolist() == [0, 0, 1, 2, -1, -1, -1] and sizes.tolist() == [4]
    dist = ref.geodesic(row, E, seed, max_distance=np.nextafter(3 * E, 0.0))[0]
    assert dist.tolist() == [0.0, E, 2 * E, INF, INF, INF, INF]
    assert ref.geodesic(row, E, seed, max_distance=0.0)[0].tolist() == [0.0] + [INF] * 6
    assert ref.geodesic(row, E, seed, max_distance=INF)[0][6] == 6 * E


def test_sizes_are_weight_sums_and_min_size_drops_segments_only():
    row = ref.centres(ref.row_cells(7))
    seed = [1, 0, 0, 0, 0, 0, 1]
    weight = [1, 1, 1, 1, 5, 5, 5]
    edges = cref.edges(row, E)
    dist, labels, sizes, sources, link, total, _ = ref.geodesic_of_edges(row, edges, seed, voxel_weight=weight)
    assert sizes.tolist() == [4, 15] and total == 2
    dist2, labels, sizes, sources, link2, total, _ = ref.geodesic_of_edges(row, edges, seed, voxel_weight=weight,
                                                                           min_size=5)
    assert labels.tolist() == [-1, -1, -1, -1, 0, 0, 0] and sizes.tolist() == [15] and sources.tolist() == [6]
    assert total == 2 and np.array_equal(ref.bits(dist2), ref.bits(dist)) and np.array_equal(link2, link)


def test_links_before_the_fixpoint_have_orphans_and_no_cycle():
    cells = ref.serpentine_cells()
    assert len(cells) == 2049
    voxels = ref.centres(ref.in_position_order([tuple(c) for c in cells]))
    pairs = cref.edges(voxels, E)
    assert len(pairs[0]) == len(cells) - 1                                # the graph is the path
    edges = ref.directed_edges(voxels, pairs)
    seed = np.zeros(len(voxels), dtype=bool)
    seed[0] = True
    full, sweeps = ref.distances(len(voxels), edges, seed)
    assert sweeps == len(cells) - 1 and full.max() == (len(cells) - 1) * E
    # the kernel's order of relaxation is not the reference's: take ANY dist between the start and the fixpoint, e.g.
    # the fixpoint with a stretch of the path reset to +inf and its end kept
    dist = full.copy()
    on_path = np.argsort(full)
    dist[on_path[100:200]] = INF
    link, orphans = ref.links(dist, edges)
    assert orphans == 1 and link[on_path[200]] == -1 and link[on_path[201]] == on_path[200]
    labels, sizes, sources, total = ref.segments(dist, link)
    assert sizes.tolist() == [100] and (labels[on_path[100:]] == -1).all() and (labels[on_path[:100]] == 0).all()
    assert not ((labels >= 0) & (link < 0)).any()


# ---- 3. the ABI ---------------------------------------------------------------------------------------------------------

def test_the_symbols_are_declared_bound_and_exported():
    with open(HEADER) as f:
        header = f.read()
    exported = ctypes.CDLL(_ffi.LIBRARY_PATH)
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(exported, name), name
    restype, argtypes = _ffi.SIGNATURES["nm_neighbor_index_geodesic_relax"]
    assert restype is ctypes.c_int and len(argtypes) == 15
    restype, argtypes = _ffi.SIGNATURES["nm_neighbor_index_geodesic_finish"]
    assert restype is ctypes.c_int and len(argtypes) == 17
    assert "dist[u] < dist[v] || (dist[u] == dist[v] && u < v)" in header
    assert _ffi.load().nm_abi_version() == 7 == _ffi.ABI_VERSION


def test_workspace_query_is_a_host_function_that_grows_with_m():
    lib = _ffi.load()
    bytes_for = lib.nm_neighbor_index_geodesic_workspace_bytes
    assert bytes_for(-1) == 0 and bytes_for(-(1 << 40)) == 0 and bytes_for(1 << 31) == 0 and bytes_for(1 << 40) == 0
    counts = (0, 1, 4095, 4096, 4097, 18000, 10 ** 6, 10 ** 6 + 1, 10 ** 8, (1 << 31) - 1)
    sizes = [bytes_for(n) for n in counts]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert all(s % 16 == 0 for s in sizes)
    assert all(s >= lib.nm_neighbor_index_components_workspace_bytes(n) for s, n in zip(sizes, counts))


def test_argument_errors_that_need_no_device():
    # without a context nothing is looked at and nothing is queued: NM_ERR_INVALID from both entry points
    lib = _ffi.load()
    lat = _ffi.NmLattice()
    assert lib.nm_neighbor_index_geodesic_relax(None, ctypes.byref(lat), E, None, 0, None, None, INF, 1, 1, None, None,
                                                None, 0, None) == _ffi.NM_ERR_INVALID
    assert lib.nm_neighbor_index_geodesic_finish(None, ctypes.byref(lat), E, None, 0, None, None, 1, None, None, None,
                                                 None, None, None, None, 0, None) == _ffi.NM_ERR_INVALID
