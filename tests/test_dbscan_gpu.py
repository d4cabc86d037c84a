"""
GPU tests of NeighborIndex.dbscan / multiscale.dbscan_cloud (nm_neighbors.hip: k_db_density, k_db_border around the
union-find kernels of components()) against the numpy reference of tests/dbscan_reference.py, which test_dbscan_cpu.py
pins to sklearn.cluster.DBSCAN and to graphs labelled by hand.  every comparison is array_equal: labels, sizes and
density on int64, core on bool.

the reference runs on the handle's own voxels; edges are found once per (case, radius) and shared, never changed.
"""

import ctypes

import numpy as np
import pytest
import torch

import components_reference as cref
import dbscan_reference as ref
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
        self.voxels = cref.voxels_of(cloud, edge)
        self.voxels.setflags(write=False)
        self.m = len(self.voxels)
        assert self.index.n_voxels == self.m and np.array_equal(self.index.voxels(), self.voxels)
        self._edges = {}

    def edges(self, radius):
        if radius not in self._edges:
            pair = cref.edges(self.voxels, radius)
            for a in pair:
                a.setflags(write=False)
            self._edges[radius] = pair
        return self._edges[radius]

    def want(self, radius, min_weight, voxel_weight=None, voxel_class=None, min_size=1):
        return ref.dbscan_of_edges(self.voxels, self.edges(radius), min_weight, voxel_weight, voxel_class, min_size)

    def check(self, radius, min_weight, voxel_weight=None, voxel_class=None, min_size=1):
        labels, sizes, core, density = self.index.dbscan(radius, min_weight, voxel_weight, voxel_class, min_size,
                                                         return_density=True)
        want_labels, want_sizes, want_core, want_density, _ = self.want(radius, min_weight, voxel_weight, voxel_class,
                                                                        min_size)
        print("M = %d, r = %g, min_weight %d: %d clusters, %d core, %d border, %d unlabelled" % (
            self.m, radius, min_weight, len(want_sizes), want_core.sum(), ((want_labels >= 0) & ~want_core).sum(),
            (want_labels < 0).sum()))
        assert labels.dtype == np.int64 and sizes.dtype == np.int64 and density.dtype == np.int64
        assert core.dtype == np.bool_
        assert labels.shape == core.shape == density.shape == (self.m,) and sizes.shape == want_sizes.shape
        assert np.array_equal(density, want_density)
        assert np.array_equal(core, want_core)
        assert np.array_equal(labels, want_labels)
        assert np.array_equal(sizes, want_sizes)
        return labels, sizes, core, density


@pytest.fixture(scope="module")
def lattice():
    """the random sparse lattice of the components tests: 17 991 voxels, five scan tiles"""
    g = Graph(cref.cells_cloud(cref.random_lattice_cells(), seed=41))
    assert g.m == 17991
    return g


@pytest.fixture(scope="module")
def thin():
    """700 x 6 x 5 cells: clusters that cross superblock borders and the pieces of a row"""
    g = Graph(cref.cells_cloud(cref.thin_cells(), seed=5))
    assert g.m == 9481 and int(g.index.filter.widths[0]) == 10
    return g


@pytest.fixture(scope="module")
def scene():
    return Graph(nearest_reference.scene_cloud()[0], nearest_reference.SCENE_EDGE)


# ---- 1. the cases the reference is tied to sklearn on ---------------------------------------------------------------

@pytest.mark.parametrize("name,rho,min_weight", ref.CASES)
def test_the_sklearn_cases(lattice, thin, name, rho, min_weight):
    g = {"random": lattice, "thin": thin}[name]
    labels, sizes, core, density = g.check(rho * E, min_weight, ref.case_weights(g.m))
    if (name, rho, min_weight) == ("random", 2.2, 60):
        assert not core.any() and (labels == -1).all() and sizes.shape == (0,)
    else:
        assert core.any() and (~core & (labels >= 0)).any() and (labels < 0).any() and len(sizes) > 1
        # numbered by smallest core member
        first = np.full(len(sizes), g.m)
        np.minimum.at(first, labels[core], np.nonzero(core)[0])
        assert (np.diff(first) > 0).all()


# ---- 2. what single linkage cannot do, and the tie rule ---------------------------------------------------------------

def test_two_blocks_and_a_bridge():
    g = Graph(cref.cells_cloud(ref.bridge_cells()))
    assert g.m == 2 * 216 + 10
    assert g.index.components(E)[1].tolist() == [g.m]                   # one chain of voxels welds the blocks
    labels, sizes, core, density = g.check(E, 5)
    assert sizes.tolist() == [217, 217]
    x = np.rint(g.voxels[:, 0] / E - 0.5).astype(np.int64)
    on_bridge = (x >= 6) & (x < 16)
    assert on_bridge.sum() == 10 and not core[on_bridge].any()
    assert labels[x == 6].tolist() == [0] and labels[x == 15].tolist() == [1]      # the ends: border of their block
    assert (labels[(x > 6) & (x < 15)] == -1).all()                                # the middle: noise
    assert (labels[x < 6] == 0).all() and (labels[x >= 16] == 1).all()
    assert (~core[~on_bridge]).sum() == 16                                         # the corners are border


def test_a_tie_between_two_clusters_goes_to_the_smaller_position():
    g = Graph(cref.cells_cloud(ref.TIE_CELLS))
    assert g.m == len(ref.TIE_CELLS)
    d2 = nearest_reference.all_d2(g.voxels, g.voxels[5:6])[0]
    assert d2[1] == d2[8] == E * E                                      # equidistant, exactly
    labels, sizes, core, density = g.check(E, ref.TIE_MIN_WEIGHT, ref.TIE_WEIGHTS)
    assert density.tolist() == ref.TIE_DENSITY and not core[5] and core.sum() == 8
    assert labels.tolist() == ref.TIE_LABELS and sizes.tolist() == ref.TIE_SIZES
    assert labels[5] == labels[1] == 1 and labels[8] == 0


# ---- 3. the generalisation: min_weight <= 1 is components() --------------------------------------------------------------

@pytest.mark.parametrize("with_classes", [False, True])
def test_min_weight_one_is_components(lattice, with_classes):
    cls = np.random.default_rng(3).integers(-1, 3, lattice.m) if with_classes else None
    for rho, min_weight, min_size in ((1.0, 1, 1), (1.5, 0, 3), (2.2, -5, 1)):
        want_labels, want_sizes = lattice.index.components(rho * E, cls, None, min_size)
        labels, sizes, core, density = lattice.index.dbscan(rho * E, min_weight, None, cls, min_size,
                                                            return_density=True)
        assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes)
        assert labels.dtype == want_labels.dtype and sizes.dtype == want_sizes.dtype
        assert np.array_equal(core, np.ones(lattice.m, dtype=bool) if cls is None else cls >= 0)
        assert (density[core] >= 1).all() and (density[~core] == 0).all()


# ---- 4. classes, weights, min_size -----------------------------------------------------------------------------------

def test_four_classes_and_removed_voxels_in_one_call(lattice):
    cls = np.random.default_rng(13).integers(-2, 4, lattice.m)
    weight = ref.case_weights(lattice.m)
    r = 2.2 * E
    labels, sizes, core, density = lattice.check(r, 14, weight, cls)
    assert (cls < 0).any() and (labels[cls < 0] == -1).all() and not core[cls < 0].any() and (density[cls < 0] == 0).all()
    assert len(sizes) > 4
    # the density counts the own class only: it is that of the class alone
    for c in range(4):
        alone = lattice.want(r, 14, weight, np.where(cls == c, 0, -1))
        assert np.array_equal(density[cls == c], alone[3][cls == c])
        assert np.array_equal(core[cls == c], alone[2][cls == c])
        assert len(set(labels[(cls == c) & (labels >= 0)])) == len(alone[1])
    assert len(set(cls[labels == labels[core][0]])) == 1                 # no cluster holds two classes


def test_point_count_weights_and_min_size(lattice):
    weight = lattice.index.point_counts()
    assert weight.sum() == len(lattice.cloud) and weight.max() > 1
    r, min_weight, min_size = 1.5 * E, 7, 12
    all_labels, all_sizes, all_core, _, total = lattice.want(r, min_weight, weight)
    assert all_sizes.min() < min_size <= all_sizes.max()                 # min_size drops some and not all
    labels, sizes, core, density = lattice.check(r, min_weight, weight, None, min_size)
    assert 0 < len(sizes) < total
    assert sizes.sum() == weight[labels >= 0].sum()
    assert np.array_equal(core, all_core)                                # core is not changed by min_size
    dropped = np.isin(all_labels, np.nonzero(all_sizes < min_size)[0])
    assert (dropped & ~all_core).any() and (dropped & all_core).any()    # border and core voxels among the dropped
    assert (labels[dropped] == -1).all() and core[dropped].any()
    keep = np.nonzero(all_sizes >= min_size)[0]
    assert np.array_equal(sizes, all_sizes[keep])


# ---- 5. small and special ---------------------------------------------------------------------------------------------

def test_a_single_voxel():
    g = Graph(np.array([[0.0, 0.0, 0.0], [0.01, 0.01, 0.01]]))
    assert g.m == 1
    for r in (0.0, E, 3.0 * E):
        labels, sizes, core, density = g.check(r, 1)
        assert labels.tolist() == [0] and sizes.tolist() == [1] and core.tolist() == [True] and density.tolist() == [1]
        labels, sizes, core, density = g.check(r, 2)
        assert labels.tolist() == [-1] and sizes.shape == (0,) and core.tolist() == [False] and density.tolist() == [1]
    labels, sizes, core, density = g.check(E, 2, g.index.point_counts())
    assert labels.tolist() == [0] and sizes.tolist() == [2] and density.tolist() == [2]
    labels, sizes, core, density = g.check(E, 0, None, np.array([-1]))
    assert labels.tolist() == [-1] and core.tolist() == [False] and density.tolist() == [0]


def test_radius_zero_the_density_is_the_own_weight(scene):
    weight = ref.case_weights(scene.m)
    labels, sizes, core, density = scene.check(0.0, 3, weight)
    assert np.array_equal(density, weight) and np.array_equal(core, weight >= 3)
    assert np.array_equal(labels[core], np.arange(core.sum())) and (labels[~core] == -1).all()
    assert np.array_equal(sizes, weight[core])


def test_radius_of_3_2_edges_on_the_scene(scene):
    assert scene.m == 884
    weight = scene.index.point_counts()
    labels, sizes, core, density = scene.check(3.2 * scene.edge, 60, weight)
    assert core.any() and (~core).any()
    scene.check(1.2 * scene.edge, 4)


def test_the_thin_lattice_at_one_edge(thin):
    labels, sizes, core, density = thin.check(E, 4)
    assert len(sizes) > 1 and (labels < 0).any()
    thin.check(1.5 * E, 9, ref.case_weights(thin.m), np.random.default_rng(2).integers(-1, 2, thin.m), 20)


# ---- 6. purity and the forms of the arguments ---------------------------------------------------------------------------

def test_two_runs_are_bit_identical_and_torch_stays_torch(lattice):
    cloud = torch.from_numpy(lattice.cloud).cuda()
    index = multiscale.NeighborIndex(cloud, E, method="index")
    cls = torch.from_numpy(np.random.default_rng(3).integers(-1, 3, lattice.m)).cuda()
    weight = index.point_counts()
    for r, min_weight in ((1.0 * E, 3), (2.2 * E, 12)):
        a = index.dbscan(r, min_weight, weight, cls, 2, return_density=True)
        b = index.dbscan(r, min_weight, weight, cls, 2, return_density=True)
        assert len(a) == 4 and all(isinstance(t, torch.Tensor) and t.is_cuda for t in a + b)
        assert [t.dtype for t in a] == [torch.int64, torch.int64, torch.bool, torch.int64]
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        want = lattice.want(r, min_weight, weight.cpu().numpy(), cls.cpu().numpy(), 2)
        assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(a, want[:4]))
    assert len(index.dbscan(E, 3)) == 3


def test_numpy_in_numpy_out_and_any_integer_dtype(scene):
    r = 1.2 * scene.edge
    cls = np.random.default_rng(9).integers(-1, 2, scene.m)
    weight = np.random.default_rng(10).integers(0, 4, scene.m)
    want = scene.want(r, 5, weight, cls)
    for cls_dtype, weight_dtype in ((np.int8, np.uint8), (np.int32, np.int32), (np.int64, np.uint16)):
        got = scene.index.dbscan(r, 5, weight.astype(weight_dtype), cls.astype(cls_dtype))
        assert len(got) == 3 and all(isinstance(t, np.ndarray) for t in got)
        assert all(np.array_equal(x, y) for x, y in zip(got, want[:3]))
    got = scene.index.dbscan(r, np.int32(5), torch.from_numpy(weight.astype(np.uint8)),
                             torch.from_numpy(cls.astype(np.int32)))
    assert isinstance(got[0], np.ndarray) and all(np.array_equal(x, y) for x, y in zip(got, want[:3]))


# ---- 7. dbscan_cloud ---------------------------------------------------------------------------------------------------

def point_level(cloud, edge, radius, min_points, point_class, min_cluster_points):
    """what dbscan_cloud promises, from the reference: (point labels, sizes, point core)"""
    lat = nearest_reference.oracle.Lattice(cloud, edge)
    addr = lat.coordinate_to_address(cloud)
    unique, inverse, counts = np.unique(addr, return_inverse=True, return_counts=True)
    voxel_class = None
    if point_class is not None:
        voxel_class = np.full(len(unique), np.iinfo(np.int64).max)
        np.minimum.at(voxel_class, inverse, point_class)
    labels, sizes, core, _ = ref.dbscan(lat.address_to_coordinate(unique), radius, min_points, counts, voxel_class,
                                        min_cluster_points)
    return labels[inverse], sizes, core[inverse]


def test_dbscan_cloud_on_the_scene(scene):
    cloud, e = scene.cloud, scene.edge
    cls = np.random.default_rng(4).integers(-1, 3, len(cloud))
    r = 1.2 * e
    for point_class, min_points, min_cluster in ((None, 20, 1), (None, 20, 200), (cls, 6, 1), (cls, 6, 15)):
        want = point_level(cloud, e, r, min_points, point_class, min_cluster)
        got = multiscale.dbscan_cloud(cloud, e, r, min_points, point_class=point_class,
                                      min_cluster_points=min_cluster)
        assert len(got) == 3 and all(isinstance(t, np.ndarray) for t in got)
        assert got[0].dtype == np.int64 and got[0].shape == (len(cloud),) and got[2].dtype == np.bool_
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), (min_points, min_cluster)
        assert np.array_equal(np.bincount(got[0][got[0] >= 0], minlength=len(got[1])), got[1])     # sizes count points
        assert want[2].any() and (~want[2]).any() and len(want[1]) >= 1
    tensors = multiscale.dbscan_cloud(torch.from_numpy(cloud).cuda(), e, r, 6, torch.from_numpy(cls).cuda(), 15)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors) and tensors[2].dtype == torch.bool
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(tensors, want))


# ---- 8. errors -------------------------------------------------------------------------------------------------------

def c_dbscan(index, radius, label, size, core, count, min_weight=3, density=None, tmp="auto", lattice="own", cls=None,
             weight=None, min_size=1):
    """nm_neighbor_index_dbscan itself: (status, message)"""
    rt = index._rt
    if isinstance(tmp, str):
        nbytes = rt.lib.nm_neighbor_index_dbscan_workspace_bytes(index.n_voxels)
        tmp = torch.empty(nbytes, dtype=torch.uint8, device=rt.device)
    lat = index.filter.nm_lattice if isinstance(lattice, str) else lattice
    rc = rt.lib.nm_neighbor_index_dbscan(
        rt.ctx, ctypes.byref(lat) if lat is not None else None, radius, min_weight, _device.ptr(index._work),
        index._work.numel(), _device.ptr(cls), _device.ptr(weight), min_size, _device.ptr(label), _device.ptr(size),
        _device.ptr(core), _device.ptr(density), _device.ptr(count), _device.ptr(tmp),
        tmp.numel() if tmp is not None else 0, rt.stream())
    torch.cuda.synchronize()
    msg = rt.lib.nm_last_error(rt.ctx)
    return rc, (msg.decode("utf-8", "replace") if msg else "")


def test_argument_errors_through_the_c_entry_point(lattice):
    index, m = lattice.index, lattice.m
    rt = index._rt
    label = torch.full((m,), -7, dtype=torch.int64, device="cuda")
    size = torch.full((m,), -7, dtype=torch.int64, device="cuda")
    density = torch.full((m,), -7, dtype=torch.int64, device="cuda")
    core = torch.full((m,), 7, dtype=torch.uint8, device="cuda")
    count = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    short = torch.empty(64, dtype=torch.uint8, device="cuda")

    def untouched():
        return bool((label == -7).all() and (size == -7).all() and (density == -7).all() and (core == 7).all())

    cases = [
        (dict(tmp=short), _ffi.NM_ERR_WORKSPACE),
        (dict(tmp=None), _ffi.NM_ERR_WORKSPACE),
        (dict(radius=float("nan")), _ffi.NM_ERR_INVALID),
        (dict(radius=-0.01), _ffi.NM_ERR_INVALID),
        (dict(radius=1e6), _ffi.NM_ERR_RADIUS),
        (dict(label=None), _ffi.NM_ERR_INVALID),
        (dict(size=None), _ffi.NM_ERR_INVALID),
        (dict(core=None), _ffi.NM_ERR_INVALID),
        (dict(count=None), _ffi.NM_ERR_INVALID),
        (dict(lattice=None), _ffi.NM_ERR_INVALID),
    ]
    for change, status in cases:
        args = dict(radius=E, label=label, size=size, core=core, count=count, density=density)
        args.update(change)
        rc, msg = c_dbscan(index, **args)
        assert rc == status and msg, (change, rc, msg)
        assert untouched() and (count == -7).all(), change
    rt.check_async(wait=True)                # nothing sticky: the context is as usable as before
    # a scratch that takes the minimum but not this index's M: refused on the device, nothing labelled
    least = torch.empty(rt.lib.nm_neighbor_index_dbscan_workspace_bytes(0), dtype=torch.uint8, device="cuda")
    rc, msg = c_dbscan(index, E, label, size, core, count, density=density, tmp=least)
    assert rc == _ffi.NM_OK and count.tolist() == [-1, -1, -1] and untouched()
    # the scratch of components() is 8 bytes per voxel short of this one: it has room for three of the five tiles
    rc, msg = c_dbscan(index, E, label, size, core, count, density=density, tmp=torch.empty(
        rt.lib.nm_neighbor_index_components_workspace_bytes(m), dtype=torch.uint8, device="cuda"))
    assert rc == _ffi.NM_OK and count.tolist() == [-1, -1, -1] and untouched()
    # and the call itself: the three counts, labels, sizes, core, density; then without the density
    weight = torch.from_numpy(ref.case_weights(m)).cuda()
    want_labels, want_sizes, want_core, want_density, total = lattice.want(1.5 * E, 12, weight.cpu().numpy(), None, 9)
    for d in (density, None):
        rc, msg = c_dbscan(index, 1.5 * E, label, size, core, count, min_weight=12, density=d, weight=weight,
                           min_size=9)
        assert rc == _ffi.NM_OK, msg
        assert count.tolist() == [len(want_sizes), total, int(want_core.sum())] and len(want_sizes) < total
        assert np.array_equal(label.cpu().numpy(), want_labels)
        assert np.array_equal(core.cpu().numpy(), want_core.astype(np.uint8))
        assert np.array_equal(density.cpu().numpy(), want_density)
        assert np.array_equal(size[:len(want_sizes)].cpu().numpy(), want_sizes)
        assert (size[len(want_sizes):] == -7).all()


def test_argument_errors_in_python(scene):
    index, m = scene.index, scene.m
    for bad in (float("nan"), -1.0, 1e6):
        with pytest.raises(ValueError):
            index.dbscan(bad, 3)
    for name in ("voxel_class", "voxel_weight"):
        for bad in (np.zeros(m - 1, dtype=np.int64), np.zeros((m, 1), dtype=np.int64), np.zeros(m),
                    np.zeros(m, dtype=bool), torch.zeros(m, dtype=torch.float32)):
            with pytest.raises(ValueError):
                index.dbscan(scene.edge, 3, **{name: bad})
    negative = np.ones(m, dtype=np.int64)
    negative[m // 2] = -1
    with pytest.raises(ValueError, match="negative"):
        index.dbscan(scene.edge, 3, voxel_weight=negative)
    for name in ("min_weight", "min_size"):
        for bad in (1.5, "2", None, True):
            args = dict(min_weight=3)
            args[name] = bad
            with pytest.raises(ValueError):
                index.dbscan(scene.edge, **args)
    searching = multiscale.NeighborIndex(scene.cloud, scene.edge, method="search")
    with pytest.raises(ValueError, match="index form"):
        searching.dbscan(scene.edge, 3)
    with pytest.raises(ValueError):
        multiscale.dbscan_cloud(scene.cloud, scene.edge, scene.edge, 5, point_class=np.zeros(len(scene.cloud)))
    with pytest.raises(ValueError):
        multiscale.dbscan_cloud(scene.cloud, scene.edge, scene.edge, 5, point_class=np.zeros(5, dtype=np.int64))
    for bad in (2.5, None, True):
        with pytest.raises(ValueError):
            multiscale.dbscan_cloud(scene.cloud, scene.edge, scene.edge, bad)
    with pytest.raises(ValueError):
        multiscale.dbscan_cloud(scene.cloud, scene.edge, -1.0, 5)
    rt = index._rt
    rt.check_async(wait=True)
