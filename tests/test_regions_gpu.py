"""
GPU tests of NeighborIndex.regions / multiscale.smooth_regions (nm_neighbors.hip: k_rg_seed, k_rg_link around the
union-find kernels of components() and the border walk of dbscan()) against the numpy reference of
tests/regions_reference.py, which test_regions_cpu.py pins to graphs labelled by hand and to the references of
components() and dbscan().  every comparison is array_equal: labels and sizes on int64, seeds on bool.

the reference runs on the handle's own voxels; edges are found once per (case, radius) and shared, never changed.
"""

import ctypes
import math

import numpy as np
import pytest
import torch

import components_reference as cref
import dbscan_reference as dref
import nearest_reference
import regions_reference as ref
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

    def want(self, radius, max_angle=None, **kwargs):
        """the reference's (labels, sizes, seed, total) for the keyword arguments of regions()"""
        if max_angle is not None:
            kwargs["min_cos"] = ref.min_cos_of(max_angle)
        return ref.regions_of_edges(self.voxels, self.edges(radius), **kwargs)

    def check(self, radius, **kwargs):
        labels, sizes, seed = self.index.regions(radius, **kwargs)
        want_labels, want_sizes, want_seed, total = self.want(radius, **kwargs)
        print("M = %d, r = %g: %d regions of %d, %d seeds, %d attached, %d unlabelled" % (
            self.m, radius, len(want_sizes), total, want_seed.sum(), ((want_labels >= 0) & ~want_seed).sum(),
            (want_labels < 0).sum()))
        assert labels.dtype == np.int64 and sizes.dtype == np.int64 and seed.dtype == np.bool_
        assert labels.shape == seed.shape == (self.m,) and sizes.shape == want_sizes.shape
        assert np.array_equal(seed, want_seed)
        assert np.array_equal(labels, want_labels)
        assert np.array_equal(sizes, want_sizes)
        return labels, sizes, seed


def mode_kwargs(mode, normal, value):
    """the keyword arguments of regions() for a mode of the reference"""
    with_normal, dims = ref.MODES[mode]
    out = {}
    if with_normal:
        out.update(voxel_normal=normal, max_angle=ref.MAX_ANGLE)
    if dims:
        out.update(voxel_value=value[:, 0] if dims == 1 else value[:, :dims],
                   max_step=ref.MAX_STEP[0] if dims == 1 else list(ref.MAX_STEP[:dims]))
    return out


@pytest.fixture(scope="module")
def lattice():
    """the random sparse lattice of the components tests: 17 991 voxels, five scan tiles"""
    g = Graph(ref.lattice_cloud("random"))
    assert g.m == 17991
    g.inputs = ref.case_inputs(g.voxels)
    g.weight = dref.case_weights(g.m)
    return g


@pytest.fixture(scope="module")
def thin():
    """700 x 6 x 5 cells: regions that cross superblock borders and the pieces of a row"""
    g = Graph(ref.lattice_cloud("thin"))
    assert g.m == 9481 and int(g.index.filter.widths[0]) == 10
    g.inputs = ref.case_inputs(g.voxels)
    g.weight = dref.case_weights(g.m)
    return g


@pytest.fixture(scope="module")
def scene():
    return Graph(nearest_reference.scene_cloud()[0], nearest_reference.SCENE_EDGE)


# ---- 1. the graphs labelled by hand and the two limits --------------------------------------------------------------

def test_the_roof():
    cells = ref.roof_cells()
    g = Graph(cref.cells_cloud(cells))
    assert g.m == 42 and np.array_equal(np.rint((g.voxels - g.voxels.min(axis=0)) / E), cells - cells.min(axis=0))
    normal, seed = ref.roof_inputs(cells)
    r = ref.ROOF_RADIUS_IN_EDGES * E
    labels, sizes, got = g.check(r, voxel_normal=normal, max_angle=0.5, voxel_seed=seed)
    assert labels.tolist() == ref.ROOF_LABELS and sizes.tolist() == ref.ROOF_SIZES and np.array_equal(got, seed)
    labels, sizes, _ = g.check(r, voxel_normal=normal, max_angle=math.pi / 2, voxel_seed=seed)
    assert labels.tolist() == [0] * 42 and sizes.tolist() == [42]
    labels, sizes, _ = g.check(E, voxel_normal=normal, max_angle=math.pi / 2, voxel_seed=seed)
    assert labels.tolist() == ref.ROOF_LABELS
    # the valley: the tie goes the other way
    cells = ref.roof_cells(valley=True)
    g = Graph(cref.cells_cloud(cells))
    normal, seed = ref.roof_inputs(cells)
    labels, sizes, _ = g.check(r, voxel_normal=normal, max_angle=0.5, voxel_seed=seed.astype(np.uint8))
    assert labels.tolist() == ref.VALLEY_LABELS and sizes.tolist() == ref.VALLEY_SIZES


def test_the_value_limit_is_inclusive():
    g = Graph(cref.cells_cloud([(x, 0, 0) for x in range(3)] + [(0, 2, 2)]))
    assert g.m == 4
    value = np.array([0.0, 0.25, 0.5, 9.0])
    assert g.check(E, voxel_value=value, max_step=0.25)[0].tolist() == [0, 0, 0, 1]
    assert g.check(E, voxel_value=value, max_step=0.2499)[0].tolist() == [0, 1, 2, 3]
    two = np.column_stack((value, [0.0, 0.0, 1.0, 0.0]))
    assert g.check(E, voxel_value=two, max_step=[0.25, 0.5])[0].tolist() == [0, 0, 1, 2]
    assert g.check(E, voxel_value=np.array([0.0, np.nan, 0.0, 0.0]), max_step=1e300)[0].tolist() == [0, 1, 2, 3]


def c_regions(index, radius, label, size, count, cls=None, weight=None, seed=None, normal=None, normal_stride=3,
              min_cos=0.0, value=None, value_stride=0, dims=0, max_step=(), min_size=1, tmp="auto", lattice="own"):
    """nm_neighbor_index_regions itself: (status, message)"""
    rt = index._rt
    if isinstance(tmp, str):
        nbytes = rt.lib.nm_neighbor_index_regions_workspace_bytes(index.n_voxels)
        tmp = torch.empty(nbytes, dtype=torch.uint8, device=rt.device)
    lat = index.filter.nm_lattice if isinstance(lattice, str) else lattice
    steps = None if max_step is None else (ctypes.c_double * max(len(max_step), 1))(*max_step)
    rc = rt.lib.nm_neighbor_index_regions(
        rt.ctx, ctypes.byref(lat) if lat is not None else None, radius, _device.ptr(index._work),
        index._work.numel(), _device.ptr(cls), _device.ptr(weight), _device.ptr(seed), _device.ptr(normal),
        normal_stride, min_cos, _device.ptr(value), value_stride, dims, steps, min_size, _device.ptr(label),
        _device.ptr(size), _device.ptr(count), _device.ptr(tmp), tmp.numel() if tmp is not None else 0, rt.stream())
    torch.cuda.synchronize()
    msg = rt.lib.nm_last_error(rt.ctx)
    return rc, (msg.decode("utf-8", "replace") if msg else "")


def test_the_normal_limit_is_inclusive():
    g = Graph(cref.cells_cloud([(0, 0, 0), (1, 0, 0), (0, 2, 2)]))
    assert g.m == 3
    normal = np.array([(1.0, 0.0, 0.0), (0.5, 0.0, math.sqrt(0.75)), (0.0, 0.0, 1.0)])
    label = torch.empty(3, dtype=torch.int64, device="cuda")
    size = torch.empty(3, dtype=torch.int64, device="cuda")
    count = torch.empty(3, dtype=torch.int64, device="cuda")
    for n, min_cos, want in ((normal, 0.5, [0, 0, 1]), (-normal, 0.5, [0, 0, 1]),
                             (normal, float(np.nextafter(0.5, 1.0)), [0, 1, 2])):
        rc, msg = c_regions(g.index, E, label, size, count, normal=torch.from_numpy(n).cuda(), min_cos=min_cos)
        assert rc == _ffi.NM_OK, msg
        assert label.tolist() == want == ref.regions(g.voxels, E, voxel_normal=n, min_cos=min_cos)[0].tolist()
        assert count.tolist() == [max(want) + 1, max(want) + 1, 3]
    # a zero normal links only where min_cos <= 0, a NaN normal never
    zero = np.array([(1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)])
    nan = np.array([(1.0, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.0, 0.0, 1.0)])
    for n, min_cos, want in ((zero, 1e-300, [0, 1, 2]), (zero, 0.0, [0, 0, 1]), (nan, -1.0, [0, 1, 2])):
        rc, msg = c_regions(g.index, E, label, size, count, normal=torch.from_numpy(n).cuda(), min_cos=min_cos)
        assert rc == _ffi.NM_OK and label.tolist() == want, (min_cos, msg)


# ---- 2. the random lattice: every instance of the link kernel ------------------------------------------------------------

@pytest.mark.parametrize("rho,mode,min_size", [
    (1.0, "normal", 1), (1.0, "value1", 20), (1.0, "value4", 1), (1.0, "both2", 20),
    (1.5, "normal", 20), (1.5, "value1", 1), (1.5, "value4", 20), (1.5, "both2", 1),
    (2.2, "normal", 1), (2.2, "value1", 20), (2.2, "value4", 1), (2.2, "both2", 20),
    (1.5, "value2", 1), (1.5, "value3", 20), (1.5, "both1", 1), (1.5, "both3", 20), (1.5, "both4", 1)])
def test_the_random_lattice(lattice, rho, mode, min_size):
    normal, value, seed, cls = lattice.inputs
    labels, sizes, got = lattice.check(rho * E, voxel_seed=seed, voxel_class=cls, voxel_weight=lattice.weight,
                                       min_size=min_size, **mode_kwargs(mode, normal, value))
    assert len(sizes) > 1 and (labels < 0).any() and ((labels >= 0) & ~got).any()
    assert (labels[cls < 0] == -1).all() and not got[cls < 0].any()
    assert sizes.min() >= min_size and sizes.sum() == lattice.weight[labels >= 0].sum()
    # numbered by smallest seed
    kept = got & (labels >= 0)
    first = np.full(len(sizes), lattice.m)
    np.minimum.at(first, labels[kept], np.nonzero(kept)[0])
    assert (np.diff(first) > 0).all()


def test_every_voxel_a_seed_and_no_weights(lattice):
    normal, value, _, cls = lattice.inputs
    labels, sizes, got = lattice.check(1.5 * E, voxel_normal=normal, max_angle=ref.MAX_ANGLE, voxel_value=value[:, :2],
                                       max_step=list(ref.MAX_STEP[:2]))
    assert got.all() and (labels >= 0).all() and sizes.sum() == lattice.m


def test_the_thin_lattice(thin):
    normal, value, seed, cls = thin.inputs
    for rho, mode, min_size in ((1.0, "both2", 1), (1.5, "normal", 20), (2.2, "value4", 1)):
        labels, sizes, got = thin.check(rho * E, voxel_seed=seed, voxel_class=cls, voxel_weight=thin.weight,
                                        min_size=min_size, **mode_kwargs(mode, normal, value))
        assert len(sizes) > 1 and (labels < 0).any()


# ---- 3. the two identities, against the live calls of the same handle ----------------------------------------------------

@pytest.mark.parametrize("with_classes", [False, True])
def test_without_seeds_and_rules_it_is_components(lattice, with_classes):
    cls = np.random.default_rng(3).integers(-1, 3, lattice.m) if with_classes else None
    weight = lattice.weight if with_classes else None
    for rho, min_size in ((1.0, 1), (1.5, 3), (2.2, 1)):
        want_labels, want_sizes = lattice.index.components(rho * E, cls, weight, min_size)
        labels, sizes, seed = lattice.index.regions(rho * E, voxel_class=cls, voxel_weight=weight, min_size=min_size)
        assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes)
        assert labels.dtype == want_labels.dtype and sizes.dtype == want_sizes.dtype
        assert np.array_equal(seed, np.ones(lattice.m, dtype=bool) if cls is None else cls >= 0)
    # the counts too, through the C entry points
    index, rt = lattice.index, lattice.index._rt
    label = torch.empty(lattice.m, dtype=torch.int64, device="cuda")
    size = torch.empty(lattice.m, dtype=torch.int64, device="cuda")
    count = torch.empty(3, dtype=torch.int64, device="cuda")
    dev_cls = None if cls is None else torch.from_numpy(cls).cuda()
    rc, msg = c_regions(index, 1.5 * E, label, size, count, cls=dev_cls, min_size=3)
    assert rc == _ffi.NM_OK, msg
    cc_count = torch.empty(2, dtype=torch.int64, device="cuda")
    nbytes = rt.lib.nm_neighbor_index_components_workspace_bytes(lattice.m)
    tmp = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rt.check(rt.lib.nm_neighbor_index_components(
        rt.ctx, ctypes.byref(index.filter.nm_lattice), 1.5 * E, _device.ptr(index._work), index._work.numel(),
        _device.ptr(dev_cls), None, 3, _device.ptr(label), _device.ptr(size), _device.ptr(cc_count), _device.ptr(tmp),
        nbytes, rt.stream()))
    assert count[:2].tolist() == cc_count.tolist() and count[0] < count[1]
    assert count[2] == (lattice.m if cls is None else int((cls >= 0).sum()))


@pytest.mark.parametrize("with_classes", [False, True])
def test_with_the_core_of_a_dbscan_run_as_seeds_it_is_that_run(lattice, thin, with_classes):
    mixed = 0
    for g in (lattice, thin):
        cls = np.random.default_rng(3).integers(-1, 3, g.m) if with_classes else None
        for rho, min_weight, min_size in ((1.0, 4, 1), (1.5, 12, 9), (2.2, 40, 1)):
            want_labels, want_sizes, core = g.index.dbscan(rho * E, min_weight, g.weight, cls, min_size)
            mixed += bool(core.any() and not core.all() and ((want_labels >= 0) & ~core).any())
            labels, sizes, seed = g.index.regions(rho * E, voxel_seed=core, voxel_class=cls, voxel_weight=g.weight,
                                                  min_size=min_size)
            assert np.array_equal(labels, want_labels) and np.array_equal(sizes, want_sizes)
            assert np.array_equal(seed, core)
    assert mixed >= 3                        # core, border and other voxels in at least half of the runs


# ---- 4. purity and the forms of the arguments ---------------------------------------------------------------------------

def test_two_runs_are_bit_identical_and_torch_stays_torch(lattice):
    normal, value, seed, cls = lattice.inputs
    cloud = torch.from_numpy(lattice.cloud).cuda()
    index = multiscale.NeighborIndex(cloud, E, method="index")
    args = dict(voxel_normal=torch.from_numpy(normal).cuda(), max_angle=ref.MAX_ANGLE,
                voxel_value=torch.from_numpy(value[:, :2].copy()).cuda(), max_step=torch.tensor(ref.MAX_STEP[:2]),
                voxel_seed=torch.from_numpy(seed).cuda(), voxel_class=torch.from_numpy(cls).cuda(),
                voxel_weight=index.point_counts(), min_size=2)
    for rho in (1.0, 2.2):
        a = index.regions(rho * E, **args)
        b = index.regions(rho * E, **args)
        assert len(a) == 3 and all(isinstance(t, torch.Tensor) and t.is_cuda for t in a + b)
        assert [t.dtype for t in a] == [torch.int64, torch.int64, torch.bool]
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        want = lattice.want(rho * E, voxel_normal=normal, max_angle=ref.MAX_ANGLE, voxel_value=value[:, :2],
                            max_step=np.asarray(ref.MAX_STEP[:2]), voxel_seed=seed, voxel_class=cls,
                            voxel_weight=index.point_counts().cpu().numpy(), min_size=2)
        assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(a, want[:3]))


def test_tables_with_a_row_stride_and_other_dtypes(lattice):
    normal, value, seed, cls = lattice.inputs
    r = 1.5 * E
    want = lattice.want(r, voxel_normal=normal, max_angle=ref.MAX_ANGLE, voxel_value=value[:, 1:3],
                        max_step=np.asarray(ref.MAX_STEP[1:3]), voxel_seed=seed, voxel_class=cls)
    wide = np.full((lattice.m, 7), np.nan)
    wide[:, 2:5] = normal
    strided = wide[:, 2:5]
    assert not strided.flags["C_CONTIGUOUS"]
    got = lattice.index.regions(r, voxel_normal=strided, max_angle=ref.MAX_ANGLE, voxel_value=value[:, 1:3],
                                max_step=ref.MAX_STEP[1:3], voxel_seed=seed, voxel_class=cls)
    assert all(np.array_equal(x, y) for x, y in zip(got, want[:3]))
    # the same on the device: the view is handed over as it is, 7 doubles a row
    dev = torch.from_numpy(wide).cuda()[:, 2:5]
    assert dev.stride(0) == 7 and lattice.index._voxel_rows(dev, "voxel_normal", 3).data_ptr() == dev.data_ptr()
    got = lattice.index.regions(r, voxel_normal=dev, max_angle=ref.MAX_ANGLE,
                                voxel_value=torch.from_numpy(value).cuda()[:, 1:3], max_step=np.asarray(ref.MAX_STEP[1:3]),
                                voxel_seed=seed.astype(np.int32), voxel_class=cls.astype(np.int8))
    assert all(isinstance(t, np.ndarray) for t in got) and all(np.array_equal(x, y) for x, y in zip(got, want[:3]))
    # fp32 tables are promoted
    got = lattice.index.regions(r, voxel_normal=normal.astype(np.float32), max_angle=ref.MAX_ANGLE, voxel_seed=seed,
                                voxel_class=cls)
    want = lattice.want(r, voxel_normal=normal.astype(np.float32).astype(np.float64), max_angle=ref.MAX_ANGLE,
                        voxel_seed=seed, voxel_class=cls)
    assert all(np.array_equal(x, y) for x, y in zip(got, want[:3]))


# ---- 5. smooth_regions ---------------------------------------------------------------------------------------------------

def test_smooth_regions_on_the_scene(scene):
    cloud, e = scene.cloud, scene.edge
    r, max_angle = 1.5 * e, 0.3
    lat = nearest_reference.oracle.Lattice(cloud, e)
    unique, inverse, counts = np.unique(lat.coordinate_to_address(cloud), return_inverse=True, return_counts=True)
    for max_curvature, min_points in ((None, 1), (0.05, 25)):
        # the normals and seeds it used, downloaded: the link rule is tested, not the eigen-solver
        normals, seed = multiscale.voxel_normals(scene.index, 2.0 * r, max_curvature)
        normals, seed = normals.cpu().numpy(), seed.cpu().numpy()
        assert seed.any() and (max_curvature is None or (~seed).any()) and np.array_equal(seed & (np.abs(normals).sum(axis=1) > 0), seed)
        want_labels, want_sizes, _, _ = scene.want(r, voxel_normal=normals, max_angle=max_angle, voxel_seed=seed,
                                                   voxel_weight=counts, min_size=min_points)
        point_labels, sizes, table = multiscale.smooth_regions(cloud, e, r, max_angle, normal_radius=2.0 * r,
                                                               max_curvature=max_curvature, min_points=min_points)
        assert all(isinstance(t, np.ndarray) for t in (point_labels, sizes, table))
        assert point_labels.dtype == np.int64 and point_labels.shape == (len(cloud),) and table.shape == (len(sizes), 25)
        assert np.array_equal(point_labels, want_labels[inverse]) and np.array_equal(sizes, want_sizes)
        assert np.array_equal(table[:, 0], sizes.astype(np.float64)) and len(sizes) > 1
        assert np.array_equal(np.bincount(point_labels[point_labels >= 0], minlength=len(sizes)), sizes)
        # the largest region is the ground, and its fitted normal is the ground's: (0, 0, 1) within max_angle
        ground = int(np.argmax(sizes))
        n = table[ground, multiscale.SEGMENT_COLUMNS["normal"]]
        print("ground: %d of %d points, normal %s" % (sizes[ground], len(cloud), n))
        assert abs(n[2]) >= math.cos(max_angle)
        assert (point_labels[:1800] == ground).mean() > 0.5             # (the plane's points come first in the cloud)
    tensors = multiscale.smooth_regions(torch.from_numpy(cloud).cuda(), e, r, max_angle, normal_radius=2.0 * r,
                                        max_curvature=0.05, min_points=25)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors)
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(tensors, (point_labels, sizes, table)))


# ---- 6. errors -------------------------------------------------------------------------------------------------------

def test_argument_errors_through_the_c_entry_point(lattice):
    index, m = lattice.index, lattice.m
    rt = index._rt
    normal, value, seed, cls = lattice.inputs
    dev_normal = torch.from_numpy(normal).cuda()
    dev_value = torch.from_numpy(value).cuda()
    label = torch.full((m,), -7, dtype=torch.int64, device="cuda")
    size = torch.full((m,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    short = torch.empty(64, dtype=torch.uint8, device="cuda")

    def untouched():
        return bool((label == -7).all() and (size == -7).all())

    values = dict(value=dev_value, value_stride=4)
    cases = [
        (dict(dims=5, max_step=(1.0,) * 5, **values), _ffi.NM_ERR_INVALID),
        (dict(dims=-1, **values), _ffi.NM_ERR_INVALID),
        (dict(normal=dev_normal, normal_stride=2), _ffi.NM_ERR_INVALID),
        (dict(normal=dev_normal, min_cos=float("nan")), _ffi.NM_ERR_INVALID),
        (dict(dims=2, max_step=(0.5, -0.5), **values), _ffi.NM_ERR_INVALID),
        (dict(dims=2, max_step=(float("nan"), 0.5), **values), _ffi.NM_ERR_INVALID),
        (dict(dims=2, max_step=None, **values), _ffi.NM_ERR_INVALID),
        (dict(dims=2, max_step=(0.5, 0.5), value=None, value_stride=4), _ffi.NM_ERR_INVALID),
        (dict(dims=4, max_step=(0.5,) * 4, value=dev_value, value_stride=3), _ffi.NM_ERR_INVALID),
        (dict(label=None), _ffi.NM_ERR_INVALID),
        (dict(size=None), _ffi.NM_ERR_INVALID),
        (dict(count=None), _ffi.NM_ERR_INVALID),
        (dict(lattice=None), _ffi.NM_ERR_INVALID),
        (dict(radius=float("nan")), _ffi.NM_ERR_INVALID),
        (dict(radius=-0.01), _ffi.NM_ERR_INVALID),
        (dict(radius=1e6), _ffi.NM_ERR_RADIUS),
        (dict(tmp=short), _ffi.NM_ERR_WORKSPACE),
        (dict(tmp=None), _ffi.NM_ERR_WORKSPACE),
    ]
    for change, status in cases:
        args = dict(radius=E, label=label, size=size, count=count)
        args.update(change)
        rc, msg = c_regions(index, **args)
        assert rc == status and msg, (change, rc, msg)
        assert untouched() and (count == -7).all(), change
    rt.check_async(wait=True)                # nothing sticky: the context is as usable as before
    # a scratch that takes the minimum but not this index's M: refused on the device, nothing labelled
    least = torch.empty(rt.lib.nm_neighbor_index_regions_workspace_bytes(0), dtype=torch.uint8, device="cuda")
    rc, msg = c_regions(index, E, label, size, count, normal=dev_normal, min_cos=0.9, tmp=least)
    assert rc == _ffi.NM_OK and count.tolist() == [-1, -1, -1] and untouched()
    # and the call itself: the three counts, labels and sizes
    want_labels, want_sizes, want_seed, total = lattice.want(
        1.5 * E, voxel_normal=normal, max_angle=ref.MAX_ANGLE, voxel_value=value, max_step=np.asarray(ref.MAX_STEP),
        voxel_seed=seed, voxel_class=cls, voxel_weight=lattice.weight, min_size=9)
    rc, msg = c_regions(index, 1.5 * E, label, size, count, cls=torch.from_numpy(cls).cuda(),
                        weight=torch.from_numpy(lattice.weight).cuda(),
                        seed=torch.from_numpy(seed.astype(np.uint8) * 3).cuda(), normal=dev_normal,
                        min_cos=ref.min_cos_of(ref.MAX_ANGLE), value=dev_value, value_stride=4, dims=4,
                        max_step=ref.MAX_STEP, min_size=9)
    assert rc == _ffi.NM_OK, msg
    assert count.tolist() == [len(want_sizes), total, int(want_seed.sum())] and len(want_sizes) < total
    assert np.array_equal(label.cpu().numpy(), want_labels)
    assert np.array_equal(size[:len(want_sizes)].cpu().numpy(), want_sizes)
    assert (size[len(want_sizes):] == -7).all()


def test_argument_errors_in_python(scene):
    index, m = scene.index, scene.m
    normal = np.tile((0.0, 0.0, 1.0), (m, 1))
    value = np.zeros((m, 2))
    for kwargs in (dict(voxel_normal=normal), dict(max_angle=0.3), dict(voxel_value=value), dict(max_step=0.5)):
        with pytest.raises(ValueError, match="go together"):
            index.regions(scene.edge, **kwargs)
    for bad in (float("nan"), -1.0, 1e6):
        with pytest.raises(ValueError):
            index.regions(bad)
    for bad in (normal[:-1], normal[:, :2], np.zeros((m, 4)), np.zeros(m), normal.astype(np.int64)):
        with pytest.raises(ValueError):
            index.regions(scene.edge, voxel_normal=bad, max_angle=0.3)
    with pytest.raises(ValueError):
        index.regions(scene.edge, voxel_normal=normal, max_angle=float("nan"))
    for bad in (value[:-1], np.zeros((m, 5)), np.zeros((m, 2, 1)), np.zeros((m, 2), dtype=np.int32)):
        with pytest.raises(ValueError):
            index.regions(scene.edge, voxel_value=bad, max_step=0.5)
    for bad in (-0.5, float("nan"), [0.5], [0.5, 0.5, 0.5], [0.5, -0.5]):
        with pytest.raises(ValueError):
            index.regions(scene.edge, voxel_value=value, max_step=bad)
    for name in ("voxel_seed", "voxel_class", "voxel_weight"):
        for bad in (np.zeros(m - 1, dtype=np.int64), np.zeros((m, 1), dtype=np.int64), np.zeros(m),
                    torch.zeros(m, dtype=torch.float32)):
            with pytest.raises(ValueError):
                index.regions(scene.edge, **{name: bad})
    for bad in (1.5, "2", None, True):
        with pytest.raises(ValueError):
            index.regions(scene.edge, min_size=bad)
    searching = multiscale.NeighborIndex(scene.cloud, scene.edge, method="search")
    with pytest.raises(ValueError, match="index form"):
        searching.regions(scene.edge)
    with pytest.raises(ValueError):
        multiscale.smooth_regions(scene.cloud, scene.edge, -1.0, 0.3)
    with pytest.raises(ValueError):
        multiscale.smooth_regions(scene.cloud, scene.edge, scene.edge, float("nan"))
    with pytest.raises(ValueError):
        multiscale.smooth_regions(scene.cloud, scene.edge, scene.edge, 0.3, max_curvature=-1.0)
    with pytest.raises(ValueError):
        multiscale.smooth_regions(scene.cloud, scene.edge, scene.edge, 0.3, min_points=2.5)
    with pytest.raises(ValueError):
        multiscale.smooth_regions(scene.cloud, scene.edge, scene.edge, 0.3, point_class=np.zeros(len(scene.cloud)))
    index._rt.check_async(wait=True)
