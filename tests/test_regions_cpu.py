"""
CPU tests for NeighborIndex.regions: they pin the yardstick the GPU tests (test_regions_gpu.py) are measured against -
the numpy reference of tests/regions_reference.py - to graphs labelled by hand, to the inclusive limits of its two
tests, and to components_reference / dbscan_reference through the two identities of the contract; they check that the
random inputs of the GPU tests are not trivial, and that the library declares, binds and exports the new symbols under
ABI 7.
"""

import ctypes
import math
import os

import numpy as np
import pytest

import components_reference as cref
import dbscan_reference as dref
import regions_reference as ref
from nimrud_amd import _ffi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nimrud_hip.h")
SYMBOLS = ("nm_neighbor_index_regions", "nm_neighbor_index_regions_workspace_bytes")
E = ref.EDGE


def centres(cells):
    return (np.asarray(cells, dtype=np.float64) + 0.5) * E


@pytest.fixture(scope="module")
def lattices():
    """name -> (the voxels of the GPU tests' cloud, weights, edges at 1.5 edges), made once and never changed"""
    out = {}
    for name, m in (("random", 17991), ("thin", 9481)):
        voxels = cref.voxels_of(ref.lattice_cloud(name), E)
        assert len(voxels) == m
        voxels.setflags(write=False)
        pairs = cref.edges(voxels, 1.5 * E)
        for a in pairs:
            a.setflags(write=False)
        out[name] = (voxels, dref.case_weights(m), pairs)
    return out


# ---- 1. graphs labelled by hand -------------------------------------------------------------------------------------

def test_the_roof_two_faces_and_a_ridge_shared_out_by_the_tie_rule():
    cells = ref.roof_cells()
    assert len(cells) == 42
    voxels = centres(cells)
    normal, seed = ref.roof_inputs(cells)
    assert seed.sum() == 36 and (~seed).sum() == 6
    r = ref.ROOF_RADIUS_IN_EDGES * E
    # a ridge voxel is exactly one edge from a seed of either face
    ridge = np.nonzero(~seed)[0]
    d2 = ((voxels[ridge][:, None, :] - voxels[None, :, :]) ** 2).sum(axis=2)
    assert ((d2 == E * E) & seed[None, :]).sum(axis=1).tolist() == [2] * 6
    labels, sizes, got_seed = ref.regions(voxels, r, voxel_normal=normal, min_cos=ref.min_cos_of(0.5), voxel_seed=seed)
    assert labels.tolist() == ref.ROOF_LABELS and sizes.tolist() == ref.ROOF_SIZES
    assert np.array_equal(got_seed, seed)
    # unsigned directions: flipping the wall's normals changes nothing
    flipped = np.where(cells[:, 2:3] < 3, -normal, normal)
    again = ref.regions(voxels, r, voxel_normal=flipped, min_cos=ref.min_cos_of(0.5), voxel_seed=seed)
    assert again[0].tolist() == ref.ROOF_LABELS
    # a right angle lets perpendicular normals link: one region
    labels, sizes, _ = ref.regions(voxels, r, voxel_normal=normal, min_cos=ref.min_cos_of(math.pi / 2),
                                   voxel_seed=seed)
    assert labels.tolist() == [0] * 42 and sizes.tolist() == [42]
    assert ref.min_cos_of(math.pi / 2) == 0.0 and ref.min_cos_of(0.5) == math.cos(0.5) and ref.min_cos_of(2.0) == 0.0
    # at one edge the seeds of the two faces are no neighbors (sqrt 2 apart): two regions whatever the angle
    labels, sizes, _ = ref.regions(voxels, E, voxel_normal=normal, min_cos=0.0, voxel_seed=seed)
    assert sizes.tolist() == ref.ROOF_SIZES and labels.tolist() == ref.ROOF_LABELS


def test_the_valley_the_tie_goes_to_the_plane():
    cells = ref.roof_cells(valley=True)
    normal, seed = ref.roof_inputs(cells)
    labels, sizes, _ = ref.regions(centres(cells), ref.ROOF_RADIUS_IN_EDGES * E, voxel_normal=normal,
                                   min_cos=ref.min_cos_of(0.5), voxel_seed=seed)
    assert labels.tolist() == ref.VALLEY_LABELS and sizes.tolist() == ref.VALLEY_SIZES


def test_a_voxel_that_is_no_seed_does_not_link_and_one_without_a_seed_neighbor_is_out():
    # a bar of seven voxels, the middle three no seeds: 3 attaches to nobody (its neighbors 2 and 4 are no seeds)
    bar = centres([(x, 0, 0) for x in range(7)])
    seed = np.array([1, 1, 0, 0, 0, 1, 1], dtype=bool)
    labels, sizes, got = ref.regions(bar, E, voxel_seed=seed)
    assert labels.tolist() == [0, 0, 0, -1, 1, 1, 1] and sizes.tolist() == [3, 3] and np.array_equal(got, seed)
    labels, sizes, got = ref.regions(bar, E, voxel_seed=seed, voxel_weight=[2, 2, 5, 9, 1, 1, 1], min_size=4)
    assert labels.tolist() == [0, 0, 0, -1, -1, -1, -1] and sizes.tolist() == [9]
    labels, sizes, got = ref.regions(bar, E, voxel_seed=seed, voxel_class=[0, 0, 0, 0, 1, 0, 0])
    assert labels.tolist() == [0, 0, 0, -1, -1, 1, 1] and got.tolist() == seed.tolist()
    labels, sizes, got = ref.regions(bar, E, voxel_seed=seed, voxel_class=[0, -1, 0, 0, 0, 0, 0])
    assert labels.tolist() == [0, -1, -1, -1, 1, 1, 1] and got.tolist() == [True, False, False, False, False, True, True]


# ---- 2. the limits are inclusive, NaN is false ------------------------------------------------------------------------

def test_the_value_limit_is_inclusive():
    row = centres([(x, 0, 0) for x in range(3)])
    value = np.array([0.0, 0.25, 0.5])
    assert ref.regions(row, E, voxel_value=value, max_step=0.25)[0].tolist() == [0, 0, 0]
    assert ref.regions(row, E, voxel_value=value, max_step=0.2499)[0].tolist() == [0, 1, 2]
    # per column: the second column cuts the second edge
    two = np.column_stack((value, [0.0, 0.0, 1.0]))
    assert ref.regions(row, E, voxel_value=two, max_step=[0.25, 0.5])[0].tolist() == [0, 0, 1]
    # NaN is false
    value = np.array([0.0, np.nan, 0.0])
    assert ref.regions(row, E, voxel_value=value, max_step=1e300)[0].tolist() == [0, 1, 2]


def test_the_normal_limit_is_inclusive():
    row = centres([(x, 0, 0) for x in range(2)])
    normal = np.array([(1.0, 0.0, 0.0), (0.5, 0.0, math.sqrt(0.75))])
    assert (normal[0, 0] * normal[1, 0] + normal[0, 1] * normal[1, 1]) + normal[0, 2] * normal[1, 2] == 0.5
    assert ref.regions(row, E, voxel_normal=normal, min_cos=0.5)[0].tolist() == [0, 0]
    assert ref.regions(row, E, voxel_normal=normal, min_cos=np.nextafter(0.5, 1.0))[0].tolist() == [0, 1]
    assert ref.regions(row, E, voxel_normal=-normal, min_cos=0.5)[0].tolist() == [0, 0]
    # a zero normal links only where min_cos <= 0, a NaN normal never
    zero = np.array([(1.0, 0.0, 0.0), (0.0, 0.0, 0.0)])
    assert ref.regions(row, E, voxel_normal=zero, min_cos=1e-300)[0].tolist() == [0, 1]
    assert ref.regions(row, E, voxel_normal=zero, min_cos=0.0)[0].tolist() == [0, 0]
    nan = np.array([(1.0, 0.0, 0.0), (np.nan, 0.0, 0.0)])
    assert ref.regions(row, E, voxel_normal=nan, min_cos=-1.0)[0].tolist() == [0, 1]


# ---- 3. the two identities ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["random", "thin"])
def test_without_seeds_and_rules_it_is_components(lattices, name):
    voxels, weight, pairs = lattices[name]
    m = len(voxels)
    cls = np.random.default_rng(5).integers(-1, 3, m)
    for voxel_class, voxel_weight, min_size in ((None, None, 1), (cls, weight, 1), (cls, weight, 9)):
        got = ref.regions_of_edges(voxels, pairs, voxel_class=voxel_class, voxel_weight=voxel_weight, min_size=min_size)
        want = cref.components_of_edges(m, pairs, voxel_class, voxel_weight, min_size)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[3] == want[2]
        assert np.array_equal(got[2], np.ones(m, dtype=bool) if voxel_class is None else cls >= 0)
        assert len(want[1]) > 1


@pytest.mark.parametrize("name", ["random", "thin"])
def test_with_the_core_of_a_dbscan_run_as_seeds_it_is_that_run(lattices, name):
    voxels, weight, pairs = lattices[name]
    m = len(voxels)
    cls = np.random.default_rng(5).integers(-1, 3, m)
    for voxel_class, min_weight, min_size in ((None, 12, 1), (cls, 7, 1), (cls, 7, 15)):
        labels, sizes, core, _, total = dref.dbscan_of_edges(voxels, pairs, min_weight, weight, voxel_class, min_size)
        assert core.any() and (~core & (labels >= 0)).any() and len(sizes) > 1
        got = ref.regions_of_edges(voxels, pairs, voxel_seed=core, voxel_class=voxel_class, voxel_weight=weight,
                                   min_size=min_size)
        assert np.array_equal(got[0], labels) and np.array_equal(got[1], sizes) and got[3] == total
        assert np.array_equal(got[2], core)


# ---- 4. the random inputs of the GPU tests are not trivial ----------------------------------------------------------------

def test_the_random_inputs_exercise_every_part_of_the_contract(lattices):
    voxels, weight, pairs = lattices["random"]
    m = len(voxels)
    normal, value, seed, cls = ref.case_inputs(voxels)
    assert (cls < 0).sum() == 1456 and sorted(set(cls.tolist())) == [-1, 0, 1, 2]
    assert (np.abs(normal).sum(axis=1) == 0).sum() == 931 and seed.sum() == 12658
    kwargs = ref.mode_arguments("both2", normal, value)
    _, alive, in_graph, _, (si, sj), normal_ok, value_ok = ref.seed_edges(m, pairs, voxel_seed=seed, voxel_class=cls,
                                                                         **kwargs)
    # both passing and failing edges among the seed-seed pairs, and each test cuts edges the other lets through
    counts = [len(si), int((normal_ok & value_ok).sum()), int((normal_ok & ~value_ok).sum()),
              int((~normal_ok & value_ok).sum()), int((~normal_ok & ~value_ok).sum())]
    print("seed-seed edges, pass, normal only, value only, neither:", counts)
    assert counts == [12491, 6332, 2712, 2413, 1034]
    labels, sizes, got_seed, total = ref.regions_of_edges(voxels, pairs, voxel_seed=seed, voxel_class=cls,
                                                          voxel_weight=weight, **kwargs)
    assert np.array_equal(got_seed, in_graph) and np.array_equal(in_graph, seed & (cls >= 0))
    border = (labels >= 0) & ~got_seed
    left = (labels < 0) & alive
    print("regions %d, border %d, left at -1 inside the graph %d" % (total, border.sum(), left.sum()))
    assert (total, len(sizes), int(border.sum()), int(left.sum())) == (6224, 6224, 4369, 498)
    assert sizes.sum() == weight[labels >= 0].sum() and (labels[~alive] == -1).all()
    # numbered by smallest seed
    first = np.full(len(sizes), m)
    np.minimum.at(first, labels[got_seed], np.nonzero(got_seed)[0])
    assert (np.diff(first) > 0).all()
    # min_size 20 drops some regions and not all
    kept = ref.regions_of_edges(voxels, pairs, voxel_seed=seed, voxel_class=cls, voxel_weight=weight, min_size=20,
                                **kwargs)
    assert len(kept[1]) == 423 and np.array_equal(kept[1], sizes[sizes >= 20])
    # every mode cuts the graph its own way
    totals = {mode: ref.regions_of_edges(voxels, pairs, voxel_seed=seed, voxel_class=cls,
                                         **ref.mode_arguments(mode, normal, value))[3] for mode in ref.MODES}
    print(totals)
    assert len(set(totals.values())) == len(ref.MODES)


# ---- 5. the ABI ---------------------------------------------------------------------------------------------------------

def test_both_symbols_are_declared_bound_and_exported():
    with open(HEADER) as f:
        header = f.read()
    exported = ctypes.CDLL(_ffi.LIBRARY_PATH)
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(exported, name), name
    restype, argtypes = _ffi.SIGNATURES["nm_neighbor_index_regions"]
    assert restype is ctypes.c_int and len(argtypes) == 22
    assert "#define NM_REGION_MAX_DIMS 4" in header and _ffi.NM_REGION_MAX_DIMS == 4
    assert "from its smaller end" in header
    assert _ffi.load().nm_abi_version() == 7 == _ffi.ABI_VERSION


def test_workspace_query_is_a_host_function_that_grows_with_m():
    lib = _ffi.load()
    bytes_for = lib.nm_neighbor_index_regions_workspace_bytes
    assert bytes_for(-1) == 0 and bytes_for(-(1 << 40)) == 0 and bytes_for(1 << 31) == 0
    counts = (0, 1, 4095, 4096, 4097, 18000, 10 ** 6, 10 ** 6 + 1, 10 ** 8, (1 << 31) - 1)
    sizes = [bytes_for(n) for n in counts]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert all(s % 16 == 0 for s in sizes)
    # the scratch of dbscan: the components scratch and the effective class of every voxel
    assert sizes == [lib.nm_neighbor_index_dbscan_workspace_bytes(n) for n in counts]
