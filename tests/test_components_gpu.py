"""
GPU tests of NeighborIndex.components / multiscale.cluster_cloud (nm_neighbors.hip: k_cc_init, k_cc_link, k_cc_flatten,
k_cc_mark, k_cc_label) against the numpy + scipy reference of tests/components_reference.py, which
test_components_cpu.py pins on graphs labelled by hand.  every comparison is array_equal on int64.

the reference runs on the handle's own voxels: each case first holds index.voxels() to nearest_reference.voxels_of.
edges are found once per (case, radius) and shared, never changed.
"""

import ctypes

import numpy as np
import pytest
import torch

import components_reference as ref
import nearest_reference
from nimrud_amd import _ffi
from nimrud_amd import device as _device
from nimrud_amd.minimal import multiscale

pytestmark = pytest.mark.gpu

E = ref.EDGE


class Graph(object):
    """a cloud, its handle, its voxels and the reference's edges per radius (made once, never changed)"""

    def __init__(self, cloud, edge=E):
        self.cloud, self.edge = cloud, edge
        self.index = multiscale.NeighborIndex(cloud, edge, method="index")
        self.voxels = ref.voxels_of(cloud, edge)
        self.voxels.setflags(write=False)
        self.m = len(self.voxels)
        assert self.index.n_voxels == self.m and np.array_equal(self.index.voxels(), self.voxels)
        self._edges = {}

    def edges(self, radius):
        if radius not in self._edges:
            pair = ref.edges(self.voxels, radius)
            for a in pair:
                a.setflags(write=False)
            self._edges[radius] = pair
        return self._edges[radius]

    def want(self, radius, voxel_class=None, voxel_weight=None, min_size=1):
        return ref.components_of_edges(self.m, self.edges(radius), voxel_class, voxel_weight, min_size)

    def check(self, radius, voxel_class=None, voxel_weight=None, min_size=1):
        labels, sizes = self.index.components(radius, voxel_class, voxel_weight, min_size)
        want_labels, want_sizes, _ = self.want(radius, voxel_class, voxel_weight, min_size)
        print("M = %d, r = %g: %d components, %d voxels unlabelled" % (self.m, radius, len(want_sizes),
                                                                       (want_labels < 0).sum()))
        assert labels.dtype == np.int64 and sizes.dtype == np.int64
        assert labels.shape == (self.m,) and sizes.shape == want_sizes.shape
        assert np.array_equal(labels, want_labels)
        assert np.array_equal(sizes, want_sizes)
        return labels, sizes


@pytest.fixture(scope="module")
def lattice():
    """the random sparse lattice: 20 000 cells drawn in 96 x 40 x 24, one point somewhere inside each"""
    g = Graph(ref.cells_cloud(ref.random_lattice_cells(), seed=41))
    assert 17000 < g.m < 18500 and g.m > 4 * 4096              # several scan tiles
    return g


@pytest.fixture(scope="module")
def snake():
    cells = ref.snake_cells()
    order = np.lexsort((cells[:, 0], cells[:, 1], cells[:, 2]))
    g = Graph(ref.cells_cloud(cells))
    g.path_step = np.argsort(order)          # path_step[i]: the position of the path's i-th cell
    assert g.m == len(cells) >= 4096
    assert [int(w) for w in g.index.filter.widths] == [6, 6, 4]          # 2 x 8 x 2 superblocks
    return g


@pytest.fixture(scope="module")
def scene():
    return Graph(nearest_reference.scene_cloud()[0], nearest_reference.SCENE_EDGE)


# ---- 1. the random sparse lattice ----------------------------------------------------------------------------------

@pytest.mark.parametrize("edges_of_radius", [1.0, 1.5, 2.2])
def test_random_lattice(lattice, edges_of_radius):
    labels, sizes = lattice.check(edges_of_radius * E)
    assert 1 < len(sizes) < lattice.m and sizes.sum() == lattice.m and (labels >= 0).all()
    # numbered by smallest member
    first = np.full(len(sizes), lattice.m)
    np.minimum.at(first, labels, np.arange(lattice.m))
    assert (np.diff(first) > 0).all()


# ---- 2. the inclusive limit, exactly ---------------------------------------------------------------------------------

def test_checkerboard_at_one_edge_leaves_every_voxel_alone():
    g = Graph(ref.cells_cloud(ref.checkerboard_cells()))
    d2 = nearest_reference.all_d2(g.voxels[:200], g.voxels)
    assert np.sort(d2, axis=1)[:, 1].min() == 2.0 * E * E         # the nearest others: sqrt(2) edges, exactly
    labels, sizes = g.check(E)
    assert np.array_equal(labels, np.arange(g.m)) and (sizes == 1).all()
    # the smallest radius whose fp64 square reaches 2 e^2 joins everything, the number below it nothing
    r = np.sqrt(2.0) * E
    while r * r < 2.0 * E * E:
        r = np.nextafter(r, 1.0)
    while np.nextafter(r, 0.0) ** 2 >= 2.0 * E * E:
        r = np.nextafter(r, 0.0)
    labels, sizes = g.check(r)
    assert sizes.tolist() == [g.m]
    labels, sizes = g.check(np.nextafter(r, 0.0))
    assert np.array_equal(labels, np.arange(g.m))


def test_filled_block_at_one_edge_is_one_component():
    g = Graph(ref.cells_cloud(ref.block_cells()))
    assert g.m == 12 * 10 * 9
    labels, sizes = g.check(E)                                     # face neighbors sit exactly at the limit
    assert (labels == 0).all() and sizes.tolist() == [g.m]
    labels, sizes = g.check(np.nextafter(E, 0.0))
    assert np.array_equal(labels, np.arange(g.m))


# ---- 3. deep trees ---------------------------------------------------------------------------------------------------

def test_snake_is_one_component(snake):
    labels, sizes = snake.check(E)
    assert (labels == 0).all() and sizes.tolist() == [snake.m]


@pytest.mark.parametrize("step", [1, 1500, 4000])
def test_snake_cut_by_one_removed_voxel_is_two(snake, step):
    cls = np.zeros(snake.m, dtype=np.int64)
    cls[snake.path_step[step]] = -1
    labels, sizes = snake.check(E, voxel_class=cls)
    assert sorted(sizes.tolist()) == sorted([step, snake.m - step - 1])
    assert labels[snake.path_step[step]] == -1 and (labels == -1).sum() == 1
    assert len(set(labels[snake.path_step[:step]])) == 1 and len(set(labels[snake.path_step[step + 1:]])) == 1


# ---- 4. other lattices and radii -------------------------------------------------------------------------------------

def test_long_thin_lattice_with_rows_in_pieces():
    g = Graph(ref.cells_cloud(ref.thin_cells(), seed=5))
    assert int(g.index.filter.widths[0]) == 10                     # 1024 cells = 32 leaves along x: two pieces a row
    for r in (1.0, 1.5):
        labels, sizes = g.check(r * E)
        assert len(sizes) > 1


def test_radius_of_3_2_edges_on_the_scene(scene):
    assert scene.m == 884
    scene.check(3.2 * scene.edge)
    scene.check(1.2 * scene.edge)


def test_a_single_voxel():
    g = Graph(np.array([[0.0, 0.0, 0.0], [0.01, 0.01, 0.01]]))
    assert g.m == 1
    for r in (0.0, E, 3.0 * E):
        labels, sizes = g.check(r)
        assert labels.tolist() == [0] and sizes.tolist() == [1]
    labels, sizes = g.check(E, voxel_class=np.array([-1]))
    assert labels.tolist() == [-1] and sizes.shape == (0,)
    labels, sizes = g.check(E, voxel_weight=np.array([2]), min_size=3)
    assert labels.tolist() == [-1] and sizes.shape == (0,)


def test_radius_zero_joins_nothing(scene):
    labels, sizes = scene.check(0.0)
    assert np.array_equal(labels, np.arange(scene.m))


# ---- 5. classes, weights, min_size -----------------------------------------------------------------------------------

def test_voxel_classes_are_segmented_in_one_call(lattice):
    cls = np.random.default_rng(3).integers(-1, 3, lattice.m)
    r = 1.5 * E
    labels, sizes = lattice.check(r, voxel_class=cls)
    assert np.array_equal(labels < 0, cls < 0)
    offset = 0
    for c in (0, 1, 2):
        # class c alone: the same partition of its voxels, and, numbers apart, in the same order
        alone, alone_sizes, _ = lattice.want(r, voxel_class=np.where(cls == c, 0, -1))
        mine = cls == c
        ids = np.unique(labels[mine])
        assert len(ids) == len(alone_sizes)
        assert np.array_equal(np.searchsorted(ids, labels[mine]), alone[mine])
        assert np.array_equal(sizes[ids], alone_sizes)
        offset += len(ids)
    assert offset == len(sizes)


def test_point_count_weights_and_min_size(lattice):
    weight = lattice.index.point_counts()
    assert weight.sum() == len(lattice.cloud) and weight.max() > 1
    r = E
    all_labels, all_sizes, total = lattice.want(r, voxel_weight=weight)
    assert all_sizes.min() < 3 <= all_sizes.max()                   # min_size = 3 drops some and not all
    labels, sizes = lattice.check(r, voxel_weight=weight, min_size=3)
    assert 0 < len(sizes) < total
    assert sizes.sum() == weight[labels >= 0].sum()
    # the survivors keep their order: they are the unfiltered components of size >= 3, renumbered in place
    keep = np.nonzero(all_sizes >= 3)[0]
    assert np.array_equal(sizes, all_sizes[keep])
    renumber = np.full(len(all_sizes) + 1, -1)
    renumber[keep] = np.arange(len(keep))
    assert np.array_equal(labels, renumber[all_labels])


# ---- 6. the existing API and purity ----------------------------------------------------------------------------------

@pytest.mark.parametrize("edges_of_radius", [1.0, 2.2])
def test_components_of_the_handles_own_lists(lattice, edges_of_radius):
    r = edges_of_radius * E
    offsets, index = lattice.index.lists(lattice.index.voxels(), r)
    rows = np.repeat(np.arange(lattice.m), np.diff(offsets))
    want_labels, want_sizes, _ = ref.components_of_edges(lattice.m, (rows, index))
    labels, sizes = lattice.index.components(r)
    assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes)


def test_two_runs_are_bit_identical_and_torch_stays_torch(lattice):
    cloud = torch.from_numpy(lattice.cloud).cuda()
    index = multiscale.NeighborIndex(cloud, E, method="index")
    cls = torch.from_numpy(np.random.default_rng(3).integers(-1, 3, lattice.m)).cuda()
    weight = index.point_counts()
    for r in (1.0 * E, 2.2 * E):
        a = index.components(r, voxel_class=cls, voxel_weight=weight, min_size=2)
        b = index.components(r, voxel_class=cls, voxel_weight=weight, min_size=2)
        assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 for t in a + b)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        want = lattice.want(r, cls.cpu().numpy(), weight.cpu().numpy(), 2)
        assert np.array_equal(a[0].cpu().numpy(), want[0]) and np.array_equal(a[1].cpu().numpy(), want[1])


def test_numpy_in_numpy_out_and_any_integer_dtype(scene):
    r = 1.2 * scene.edge
    cls = np.random.default_rng(9).integers(-1, 2, scene.m)
    want = scene.want(r, voxel_class=cls)
    for dtype in (np.int8, np.int32, np.int64):
        labels, sizes = scene.index.components(r, voxel_class=cls.astype(dtype))
        assert isinstance(labels, np.ndarray) and isinstance(sizes, np.ndarray)
        assert np.array_equal(labels, want[0]) and np.array_equal(sizes, want[1])
    labels, sizes = scene.index.components(r, voxel_class=torch.from_numpy(cls.astype(np.int32)))
    assert isinstance(labels, np.ndarray) and np.array_equal(labels, want[0])       # the handle follows its cloud


# ---- 7. cluster_cloud ------------------------------------------------------------------------------------------------

def point_level(cloud, edge, radius, point_class, min_points):
    """what cluster_cloud promises, from the reference: (point labels, sizes)"""
    lat = nearest_reference.oracle.Lattice(cloud, edge)
    addr = lat.coordinate_to_address(cloud)
    unique, inverse, counts = np.unique(addr, return_inverse=True, return_counts=True)
    voxel_class = None
    if point_class is not None:
        voxel_class = np.full(len(unique), np.iinfo(np.int64).max)
        np.minimum.at(voxel_class, inverse, point_class)
    labels, sizes = ref.components(lat.address_to_coordinate(unique), radius, voxel_class, counts, min_points)
    return labels[inverse], sizes


def test_cluster_cloud_on_the_island():
    cloud = nearest_reference.island_cloud()
    e = nearest_reference.ISLAND_EDGE
    got = multiscale.cluster_cloud(cloud, e, e)                    # every step exactly at the limit
    want = point_level(cloud, e, e, None, 1)
    assert isinstance(got[0], np.ndarray) and got[0].dtype == np.int64 and got[0].shape == (len(cloud),)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(want[1]) > 1
    cls = np.random.default_rng(2).integers(-1, 2, len(cloud))
    got = multiscale.cluster_cloud(cloud, e, e, point_class=cls, min_points=2)
    want = point_level(cloud, e, e, cls, 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (want[0] == -1).any() and len(want[1]) > 1


def test_cluster_cloud_counts_points_and_takes_the_minimum_class(scene):
    cloud, e = scene.cloud, scene.edge
    cls = np.random.default_rng(4).integers(-1, 3, len(cloud))
    r = 1.2 * e
    for point_class, min_points in ((None, 1), (None, 40), (cls, 1), (cls, 5)):
        want = point_level(cloud, e, r, point_class, min_points)
        got = multiscale.cluster_cloud(cloud, e, r, point_class=point_class, min_points=min_points)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), min_points
        assert np.array_equal(np.bincount(got[0][got[0] >= 0], minlength=len(got[1])), got[1])     # sizes count points
    tensors = multiscale.cluster_cloud(torch.from_numpy(cloud).cuda(), e, r, torch.from_numpy(cls).cuda(), 5)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors)
    assert np.array_equal(tensors[0].cpu().numpy(), want[0]) and np.array_equal(tensors[1].cpu().numpy(), want[1])


# ---- 8. errors -------------------------------------------------------------------------------------------------------

def c_components(index, radius, label, size, count, tmp="auto", lattice="own", cls=None, weight=None, min_size=1):
    """nm_neighbor_index_components itself: (status, message)"""
    rt = index._rt
    if isinstance(tmp, str):
        nbytes = rt.lib.nm_neighbor_index_components_workspace_bytes(index.n_voxels)
        tmp = torch.empty(nbytes, dtype=torch.uint8, device=rt.device)
    lat = index.filter.nm_lattice if isinstance(lattice, str) else lattice
    rc = rt.lib.nm_neighbor_index_components(
        rt.ctx, ctypes.byref(lat) if lat is not None else None, radius, _device.ptr(index._work), index._work.numel(),
        _device.ptr(cls), _device.ptr(weight), min_size, _device.ptr(label), _device.ptr(size), _device.ptr(count),
        _device.ptr(tmp), tmp.numel() if tmp is not None else 0, rt.stream())
    torch.cuda.synchronize()
    msg = rt.lib.nm_last_error(rt.ctx)
    return rc, (msg.decode("utf-8", "replace") if msg else "")


def test_argument_errors_through_the_c_entry_point(lattice):
    index, m = lattice.index, lattice.m
    rt = index._rt
    label = torch.full((m,), -7, dtype=torch.int64, device="cuda")
    size = torch.full((m,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    short = torch.empty(64, dtype=torch.uint8, device="cuda")
    cases = [
        (dict(tmp=short), _ffi.NM_ERR_WORKSPACE),
        (dict(tmp=None), _ffi.NM_ERR_WORKSPACE),
        (dict(radius=float("nan")), _ffi.NM_ERR_RADIUS),
        (dict(radius=-0.01), _ffi.NM_ERR_RADIUS),
        (dict(radius=1e6), _ffi.NM_ERR_RADIUS),
        (dict(label=None), _ffi.NM_ERR_INVALID),
        (dict(size=None), _ffi.NM_ERR_INVALID),
        (dict(count=None), _ffi.NM_ERR_INVALID),
        (dict(lattice=None), _ffi.NM_ERR_INVALID),
    ]
    for change, status in cases:
        args = dict(radius=E, label=label, size=size, count=count)
        args.update(change)
        rc, msg = c_components(index, **args)
        assert rc == status and msg, (change, rc, msg)
        assert (label == -7).all() and (size == -7).all() and (count == -7).all(), change
    rt.check_async(wait=True)                # nothing sticky: the context is as usable as before
    # a scratch that takes the minimum but not this index's M: refused on the device, nothing labelled
    least = torch.empty(rt.lib.nm_neighbor_index_components_workspace_bytes(0), dtype=torch.uint8, device="cuda")
    rc, msg = c_components(index, E, label, size, count, tmp=least)
    assert rc == _ffi.NM_OK and count.tolist() == [-1, -1] and (label == -7).all() and (size == -7).all()
    # and the call itself: both counts, labels and sizes
    rc, msg = c_components(index, E, label, size, count)
    want_labels, want_sizes, total = lattice.want(E)
    assert rc == _ffi.NM_OK, msg
    assert count.tolist() == [len(want_sizes), total]
    assert np.array_equal(label.cpu().numpy(), want_labels)
    assert np.array_equal(size[:len(want_sizes)].cpu().numpy(), want_sizes) and (size[len(want_sizes):] == -7).all()
    weight = torch.from_numpy(index.point_counts()).cuda()
    rc, msg = c_components(index, E, label, size, count, weight=weight, min_size=3)
    want_labels, want_sizes, total = lattice.want(E, voxel_weight=weight.cpu().numpy(), min_size=3)
    assert rc == _ffi.NM_OK and count.tolist() == [len(want_sizes), total] and len(want_sizes) < total
    assert np.array_equal(label.cpu().numpy(), want_labels)


def test_argument_errors_in_python(scene):
    index, m = scene.index, scene.m
    for bad in (float("nan"), -1.0, 1e6):
        with pytest.raises(ValueError):
            index.components(bad)
    for name in ("voxel_class", "voxel_weight"):
        for bad in (np.zeros(m - 1, dtype=np.int64), np.zeros((m, 1), dtype=np.int64), np.zeros(m),
                    np.zeros(m, dtype=bool), torch.zeros(m, dtype=torch.float32)):
            with pytest.raises(ValueError):
                index.components(scene.edge, **{name: bad})
    for bad in (1.5, "2", None, True):
        with pytest.raises(ValueError):
            index.components(scene.edge, min_size=bad)
    searching = multiscale.NeighborIndex(scene.cloud, scene.edge, method="search")
    with pytest.raises(ValueError, match="index form"):
        searching.components(scene.edge)
    with pytest.raises(ValueError):
        multiscale.cluster_cloud(scene.cloud, scene.edge, scene.edge, point_class=np.zeros(len(scene.cloud)))
    with pytest.raises(ValueError):
        multiscale.cluster_cloud(scene.cloud, scene.edge, scene.edge, point_class=np.zeros(5, dtype=np.int64))
