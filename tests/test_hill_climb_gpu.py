"""
GPU tests of NeighborIndex.hill_climb / multiscale.peak_segments (nm_neighbors.hip: k_hc_parent and k_hc_peaks around the
flatten, mark, scan and label kernels of components()) against the numpy reference of tests/hill_climb_reference.py,
which test_hill_climb_cpu.py pins to graphs labelled by hand.  every comparison is array_equal: labels, sizes, peaks and
links on int64.

the reference runs on the handle's own voxels; edges are found once per (case, radius) and shared, never changed.  the
voxels of the lattices are cell centres, so equal squared distances are everywhere: every case leans on the tiebreaks.
"""

import ctypes

import numpy as np
import pytest
import torch

import components_reference as cref
import dbscan_reference as dref
import hill_climb_reference as ref
import nearest_reference
import regions_reference as rref
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

    def want(self, radius, value, mode, **kwargs):
        """the reference's (labels, sizes, peaks, link, total)"""
        return ref.hill_climb_of_edges(self.voxels, self.edges(radius), value, mode, **kwargs)

    def check(self, radius, value, mode, **kwargs):
        got = self.index.hill_climb(radius, value, link=mode, return_link=True, **kwargs)
        want = self.want(radius, value, mode, **kwargs)
        print("M = %d, r = %g, %s: %d segments of %d, %d voxels outside" % (
            self.m, radius, mode, len(want[1]), want[4], (want[3] < 0).sum()))
        assert len(got) == 4 and all(a.dtype == np.int64 for a in got)
        assert got[0].shape == got[3].shape == (self.m,) and got[1].shape == got[2].shape == want[1].shape
        assert np.array_equal(got[3], want[3])                      # link
        assert np.array_equal(got[0], want[0])                      # labels
        assert np.array_equal(got[1], want[1])                      # sizes
        assert np.array_equal(got[2], want[2])                      # peaks
        return got


ANCHOR = (0, 4, 4)


def cells_graph(cells):
    """a Graph of one point per cell, the cells listed in position order, and the ANCHOR behind them: a lattice needs
    an extent on every axis.  the anchor is the last position and more than three edges from every other cell"""
    cells = np.asarray(list(cells) + [ANCHOR], dtype=np.int64)
    g = Graph(cref.cells_cloud(cells))
    assert g.m == len(cells)
    assert np.array_equal(np.rint((g.voxels - g.voxels.min(axis=0)) / E), cells - cells.min(axis=0))
    return g


def hand(g, radius, value, mode, voxel_class=None, voxel_weight=None, min_size=1):
    """g.check with the anchor's entries added to the arguments (value 0, class 0, weight 1) and taken off the results:
    it is a segment of its own, the last one"""
    n = g.m - 1
    kwargs = dict(min_size=min_size)
    if voxel_class is not None:
        kwargs["voxel_class"] = np.append(voxel_class, 0)
    if voxel_weight is not None:
        kwargs["voxel_weight"] = np.append(voxel_weight, 1)
    labels, sizes, peaks, link = g.check(radius, np.append(np.asarray(value, dtype=np.float64), 0.0), mode, **kwargs)
    assert link[n] == n and (link[:n] != n).all()
    if min_size <= 1:
        assert labels[n] == len(sizes) - 1 and (labels[:n] != labels[n]).all() and sizes[-1] == 1 and peaks[-1] == n
        sizes, peaks = sizes[:-1], peaks[:-1]
    else:
        assert labels[n] == -1
    return labels[:n], sizes, peaks, link[:n]


@pytest.fixture(scope="module")
def lattice():
    """the random sparse lattice of the components tests: 17 991 voxels, five scan tiles"""
    g = Graph(rref.lattice_cloud("random"))
    assert g.m == 17991
    return g


@pytest.fixture(scope="module")
def thin():
    """700 x 6 x 5 cells: segments that cross superblock borders and the pieces of a row"""
    g = Graph(rref.lattice_cloud("thin"))
    assert g.m == 9481 and int(g.index.filter.widths[0]) == 10
    return g


@pytest.fixture(scope="module")
def scene():
    return Graph(nearest_reference.scene_cloud()[0], nearest_reference.SCENE_EDGE)


VALUES = {"smooth": ref.smooth_values, "levels": ref.quantised_values, "x": lambda voxels: voxels[:, 0].copy()}


# ---- 1. the graphs labelled by hand, on the device ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", ref.MODES)
def test_the_hand_graphs(mode):
    row = cells_graph(ref.row_cells(7))
    labels, sizes, peaks, link = hand(row, E, ref.RAMP_VALUES, mode)
    assert link.tolist() == [1, 2, 3, 4, 5, 6, 6] and labels.tolist() == [0] * 7 and peaks.tolist() == [6]
    labels, sizes, peaks, link = hand(row, 3 * E, ref.RAMP_VALUES, mode)
    assert link.tolist() == ([3, 4, 5, 6, 6, 6, 6] if mode == "highest" else [1, 2, 3, 4, 5, 6, 6])
    # two bumps and a saddle: one component (and the anchor), two segments, the saddle by the tiebreak
    assert row.index.components(E)[1].tolist() == [7, 1]
    labels, sizes, peaks, link = hand(row, E, ref.BUMPS_VALUES, mode)
    assert link.tolist() == ref.BUMPS_LINK_1 and labels.tolist() == ref.BUMPS_LABELS_1
    assert sizes.tolist() == [4, 3] and peaks.tolist() == [1, 5]
    labels, sizes, peaks, link = hand(row, 2 * E, ref.BUMPS_VALUES, mode)
    assert link.tolist() == ref.BUMPS_LINK_2[mode] and labels.tolist() == ref.BUMPS_LABELS_2[mode]
    # min_size drops the first bump (and the anchor) and renumbers; the links stay
    labels, sizes, peaks, link = hand(row, E, ref.BUMPS_VALUES, mode, voxel_weight=[1, 1, 1, 1, 5, 5, 5], min_size=5)
    assert labels.tolist() == [-1, -1, -1, -1, 0, 0, 0] and sizes.tolist() == [15] and peaks.tolist() == [5]
    assert link.tolist() == ref.BUMPS_LINK_1
    # NaN and negative classes are out of the graph; infinities are values
    labels, sizes, peaks, link = hand(row, E, [0.0, 1.0, 2.0, float("nan"), 4.0, 5.0, 6.0], mode)
    assert labels.tolist() == [0, 0, 0, -1, 1, 1, 1] and link.tolist() == [1, 2, 2, -1, 5, 6, 6]
    labels, sizes, peaks, link = hand(row, 2 * E, ref.RAMP_VALUES, mode, voxel_class=[0, 1, 0, 1, 0, 1, 0])
    assert link.tolist() == [2, 3, 4, 5, 6, 5, 6] and labels.tolist() == [1, 0, 1, 0, 1, 0, 1]
    labels, sizes, peaks, link = hand(row, E, ref.RAMP_VALUES, mode, voxel_class=[0, 0, 0, -1, 0, 0, 0])
    assert labels.tolist() == [0, 0, 0, -1, 1, 1, 1] and link.tolist() == [1, 2, 2, -1, 5, 6, 6]
    labels, sizes, peaks, link = hand(row, E, [-np.inf, -np.inf, 0.0, np.inf, np.inf, 1.0, 2.0], mode)
    assert link.tolist() == [0, 2, 3, 3, 3, 4, 6] and peaks.tolist() == [0, 3, 6]
    # the two modes differ
    three = cells_graph(ref.row_cells(3))
    assert hand(three, 2 * E, ref.DIFFER_VALUES, mode)[3].tolist() == ref.DIFFER_LINK[mode]
    # plateaus: -0 == +0, the smallest position is the peak, and a plateau that is not convex splits
    ell = cells_graph(ref.plateau_cells())
    for rho in (1.0, 2.0):
        labels, sizes, peaks, link = hand(ell, rho * E, np.where(np.arange(9) % 2 == 0, 0.0, -0.0), mode)
        assert labels.tolist() == [0] * 9 and peaks.tolist() == [0]
    u = cells_graph(ref.u_cells())
    labels, sizes, peaks, link = hand(u, E, np.zeros(13), mode)
    assert labels.tolist() == ref.U_LABELS and peaks.tolist() == ref.U_PEAKS and link[12] == 7


# ---- 2. the lattices against the reference ---------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("values", ["smooth", "levels"])
@pytest.mark.parametrize("rho", [1.0, 1.5, 3.0])
def test_the_random_lattice(lattice, rho, values, mode):
    labels, sizes, peaks, link = lattice.check(rho * E, VALUES[values](lattice.voxels), mode)
    assert (labels >= 0).all() and sizes.sum() == lattice.m and len(sizes) > 1


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("values", ["smooth", "levels"])
@pytest.mark.parametrize("rho", [1.0, 1.5, 3.0])
def test_the_thin_lattice(thin, rho, values, mode):
    labels, sizes, peaks, link = thin.check(rho * E, VALUES[values](thin.voxels), mode)
    assert (labels >= 0).all() and sizes.sum() == thin.m and len(sizes) > 1


@pytest.mark.parametrize("rho", [1.0, 1.5, 3.0])
def test_a_deep_chain_through_the_flatten_kernel(thin, rho):
    # value = x, "nearest": every voxel steps about one cell; at three edges the chain runs along the whole lattice
    labels, sizes, peaks, link = thin.check(rho * E, VALUES["x"](thin.voxels), "nearest")
    steps, at = 0, np.arange(thin.m)
    while (link[at] != at).any():
        at = link[at]
        steps += 1
    print("the longest chain has %d links" % steps)
    assert steps >= (700 if rho == 3.0 else 20)


@pytest.mark.parametrize("mode", ref.MODES)
def test_classes_weights_and_min_size(lattice, thin, mode):
    for g in (lattice, thin):
        cls, weight = ref.case_classes(g.m), dref.case_weights(g.m)
        value = ref.quantised_values(g.voxels)
        labels, sizes, peaks, link = g.check(1.5 * E, value, mode, voxel_class=cls, voxel_weight=weight, min_size=9)
        assert (labels[cls < 0] == -1).all() and (link[cls < 0] == -1).all() and (link[cls >= 0] >= 0).all()
        dropped = (labels < 0) & (cls >= 0)
        assert dropped.any() and sizes.min() >= 9 and sizes.sum() == weight[labels >= 0].sum()
        assert np.array_equal(cls[link[cls >= 0]], cls[cls >= 0])


@pytest.mark.parametrize("mode", ref.MODES)
def test_nan_values(lattice, mode):
    value = ref.smooth_values(lattice.voxels)
    value[::37] = np.nan
    labels, sizes, peaks, link = lattice.check(1.5 * E, value, mode, voxel_class=ref.case_classes(lattice.m, seed=8))
    assert (labels[::37] == -1).all() and (link[::37] == -1).all()
    assert not np.isin(link[link >= 0], np.arange(0, lattice.m, 37)).any()


# ---- 3. properties that need no reference ----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ref.MODES)
def test_properties_of_the_links_and_segments(lattice, mode):
    index, m, voxels = lattice.index, lattice.m, lattice.voxels
    cls = ref.case_classes(m)
    value = ref.quantised_values(voxels)
    r = 1.5 * E
    labels, sizes, peaks, link = index.hill_climb(r, value, link=mode, voxel_class=cls, return_link=True)
    inside = np.nonzero(link >= 0)[0]
    assert np.array_equal(link >= 0, cls >= 0)
    up = link[inside]
    climbs = up != inside
    # every link is higher, within the radius and of the same class
    assert ((value[up] > value[inside]) | ((value[up] == value[inside]) & (up < inside)))[climbs].all()
    d = voxels[inside] - voxels[up]
    assert ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r * r).all()
    assert np.array_equal(cls[up], cls[inside])
    # a voxel and its link share the segment, the peaks link to themselves and come in ascending order
    assert np.array_equal(labels[up], labels[inside]) and (labels[inside] >= 0).all()
    assert np.array_equal(link[peaks], peaks) and (np.diff(peaks) > 0).all()
    assert np.array_equal(np.nonzero(link == np.arange(m))[0], peaks)
    assert np.array_equal(labels[peaks], np.arange(len(peaks))) and np.array_equal(np.bincount(labels[inside]), sizes)
    # every segment lies inside one component of the same graph
    comp, comp_sizes = index.components(r, cls)
    assert np.array_equal(comp[peaks][labels[inside]], comp[inside]) and len(comp_sizes) < len(sizes)
    # a strictly increasing map of the values (exact in fp64: small integers) changes nothing
    again = index.hill_climb(r, 2.0 * value + 1.0, link=mode, voxel_class=cls, return_link=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (labels, sizes, peaks, link)))
    # two calls are bit-equal
    again = index.hill_climb(r, value, link=mode, voxel_class=cls, return_link=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (labels, sizes, peaks, link)))
    # below one edge every voxel of the graph is its own segment
    labels, sizes, peaks, link = index.hill_climb(0.99 * E, value, link=mode, voxel_class=cls, return_link=True)
    assert np.array_equal(peaks, np.nonzero(cls >= 0)[0]) and (sizes == 1).all()
    assert np.array_equal(link, np.where(cls >= 0, np.arange(m), -1))
    assert np.array_equal(labels[peaks], np.arange(len(peaks))) and (labels[cls < 0] == -1).all()
    # without return_link: three outputs, the same
    three = index.hill_climb(0.99 * E, value, link=mode, voxel_class=cls)
    assert len(three) == 3 and all(np.array_equal(a, b) for a, b in zip(three, (labels, sizes, peaks)))


def test_torch_stays_torch_and_other_dtypes(thin):
    cloud = torch.from_numpy(thin.cloud).cuda()
    index = multiscale.NeighborIndex(cloud, E, method="index")
    value = ref.smooth_values(thin.voxels).astype(np.float32)
    cls = ref.case_classes(thin.m)
    want = thin.want(1.5 * E, value.astype(np.float64), "nearest", voxel_class=cls,
                     voxel_weight=index.point_counts().cpu().numpy(), min_size=2)
    a = index.hill_climb(1.5 * E, torch.from_numpy(value).cuda(), link="nearest",
                         voxel_class=torch.from_numpy(cls.astype(np.int32)).cuda(), voxel_weight=index.point_counts(),
                         min_size=2, return_link=True)
    assert len(a) == 4 and all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 for t in a)
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(a, want[:4]))
    # a strided view of a table is taken, numpy in a torch handle too
    wide = np.zeros((thin.m, 3))
    wide[:, 1] = value
    b = index.hill_climb(1.5 * E, wide[:, 1], link="nearest", voxel_class=cls.astype(np.int8),
                         voxel_weight=index.point_counts(), min_size=2, return_link=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 4. the C entry point ----------------------------------------------------------------------------------------------------

def c_hill_climb(index, radius, value, label, size, peak, count, mode=0, link=None, cls=None, weight=None, min_size=1,
                 tmp="auto", lattice="own"):
    """nm_neighbor_index_hill_climb itself: (status, message)"""
    rt = index._rt
    if isinstance(tmp, str):
        nbytes = rt.lib.nm_neighbor_index_hill_climb_workspace_bytes(index.n_voxels)
        tmp = torch.empty(nbytes, dtype=torch.uint8, device=rt.device)
    lat = index.filter.nm_lattice if isinstance(lattice, str) else lattice
    rc = rt.lib.nm_neighbor_index_hill_climb(
        rt.ctx, ctypes.byref(lat) if lat is not None else None, radius, mode, _device.ptr(index._work),
        index._work.numel(), _device.ptr(value), _device.ptr(cls), _device.ptr(weight), min_size, _device.ptr(label),
        _device.ptr(size), _device.ptr(peak), _device.ptr(link), _device.ptr(count), _device.ptr(tmp),
        tmp.numel() if tmp is not None else 0, rt.stream())
    torch.cuda.synchronize()
    msg = rt.lib.nm_last_error(rt.ctx)
    return rc, (msg.decode("utf-8", "replace") if msg else "")


def test_the_c_entry_point(lattice):
    index, m = lattice.index, lattice.m
    rt = index._rt
    host_value = ref.quantised_values(lattice.voxels)
    cls, weight = ref.case_classes(m), dref.case_weights(m)
    value = torch.from_numpy(host_value).cuda()

    def filled(n):
        return torch.full((n,), -7, dtype=torch.int64, device="cuda")

    label, size, peak, link, count = filled(m), filled(m), filled(m), filled(m), filled(2)
    short = torch.empty(64, dtype=torch.uint8, device="cuda")

    def untouched():
        return bool((label == -7).all() and (size == -7).all() and (peak == -7).all() and (link == -7).all())

    cases = [
        (dict(value=None), _ffi.NM_ERR_INVALID),
        (dict(label=None), _ffi.NM_ERR_INVALID),
        (dict(size=None), _ffi.NM_ERR_INVALID),
        (dict(peak=None), _ffi.NM_ERR_INVALID),
        (dict(count=None), _ffi.NM_ERR_INVALID),
        (dict(lattice=None), _ffi.NM_ERR_INVALID),
        (dict(mode=2), _ffi.NM_ERR_INVALID),
        (dict(mode=-1), _ffi.NM_ERR_INVALID),
        (dict(radius=float("nan")), _ffi.NM_ERR_INVALID),
        (dict(radius=-0.01), _ffi.NM_ERR_INVALID),
        (dict(radius=1e6), _ffi.NM_ERR_RADIUS),
        (dict(tmp=short), _ffi.NM_ERR_WORKSPACE),
        (dict(tmp=None), _ffi.NM_ERR_WORKSPACE),
    ]
    for change, status in cases:
        args = dict(radius=E, value=value, label=label, size=size, peak=peak, count=count, link=link)
        args.update(change)
        rc, msg = c_hill_climb(index, **args)
        assert rc == status and msg, (change, rc, msg)
        assert untouched() and (count == -7).all(), change
    rt.check_async(wait=True)                # nothing sticky: the context is as usable as before
    # a scratch that takes the minimum but not this index's M: refused on the device, nothing written
    least = torch.empty(rt.lib.nm_neighbor_index_hill_climb_workspace_bytes(0), dtype=torch.uint8, device="cuda")
    rc, msg = c_hill_climb(index, E, value, label, size, peak, count, link=link, tmp=least)
    assert rc == _ffi.NM_OK and count.tolist() == [-1, -1] and untouched()
    # the call itself in both modes: counts, labels, sizes, peaks, links, and nothing behind the C entries
    for mode, name in ((_ffi.NM_CLIMB["highest"], "highest"), (_ffi.NM_CLIMB["nearest"], "nearest")):
        want_labels, want_sizes, want_peaks, want_link, total = lattice.want(
            1.5 * E, host_value, name, voxel_class=cls, voxel_weight=weight, min_size=9)
        rc, msg = c_hill_climb(index, 1.5 * E, value, label, size, peak, count, mode=mode, link=link,
                               cls=torch.from_numpy(cls).cuda(), weight=torch.from_numpy(weight).cuda(), min_size=9)
        assert rc == _ffi.NM_OK, msg
        kept = len(want_sizes)
        assert count.tolist() == [kept, total] and kept < total
        assert np.array_equal(label.cpu().numpy(), want_labels) and np.array_equal(link.cpu().numpy(), want_link)
        assert np.array_equal(size[:kept].cpu().numpy(), want_sizes)
        assert np.array_equal(peak[:kept].cpu().numpy(), want_peaks)
        assert (size[kept:] == -7).all() and (peak[kept:] == -7).all()
        # d_link NULL: the rest is the same
        label2, size2, peak2, count2 = filled(m), filled(m), filled(m), filled(2)
        rc, msg = c_hill_climb(index, 1.5 * E, value, label2, size2, peak2, count2, mode=mode,
                               cls=torch.from_numpy(cls).cuda(), weight=torch.from_numpy(weight).cuda(), min_size=9)
        assert rc == _ffi.NM_OK, msg
        assert torch.equal(label2, label) and torch.equal(size2, size) and torch.equal(peak2, peak)
        assert torch.equal(count2, count)


def test_argument_errors_in_python(scene):
    index, m = scene.index, scene.m
    value = np.zeros(m)
    for bad in (float("nan"), -1.0, 1e6):
        with pytest.raises(ValueError):
            index.hill_climb(bad, value)
    for bad in (value[:-1], np.zeros((m, 1)), np.zeros(m, dtype=np.int64), torch.zeros(m, dtype=torch.int32)):
        with pytest.raises(ValueError):
            index.hill_climb(scene.edge, bad)
    for bad in ("steepest", None, 0):
        with pytest.raises(ValueError, match="link must be"):
            index.hill_climb(scene.edge, value, link=bad)
    for name in ("voxel_class", "voxel_weight"):
        for bad in (np.zeros(m - 1, dtype=np.int64), np.zeros((m, 1), dtype=np.int64), np.zeros(m)):
            with pytest.raises(ValueError):
                index.hill_climb(scene.edge, value, **{name: bad})
    for bad in (1.5, "2", None, True):
        with pytest.raises(ValueError):
            index.hill_climb(scene.edge, value, min_size=bad)
    searching = multiscale.NeighborIndex(scene.cloud, scene.edge, method="search")
    with pytest.raises(ValueError, match="index form"):
        searching.hill_climb(scene.edge, value)
    with pytest.raises(ValueError):
        multiscale.peak_segments(scene.cloud, scene.edge, -1.0)
    with pytest.raises(ValueError, match="link must be"):
        multiscale.peak_segments(scene.cloud, scene.edge, scene.edge, link="up")
    with pytest.raises(ValueError):
        multiscale.peak_segments(scene.cloud, scene.edge, scene.edge, min_points=2.5)
    with pytest.raises(ValueError):
        multiscale.peak_segments(scene.cloud, scene.edge, scene.edge, point_value=np.zeros(len(scene.cloud) - 1))
    with pytest.raises(ValueError):
        multiscale.peak_segments(scene.cloud, scene.edge, scene.edge, point_value=np.zeros(len(scene.cloud), dtype=int))
    with pytest.raises(ValueError):
        multiscale.peak_segments(scene.cloud, scene.edge, scene.edge, point_class=np.zeros(len(scene.cloud)))
    index._rt.check_async(wait=True)


# ---- 5. peak_segments ------------------------------------------------------------------------------------------------------

def test_peak_segments_on_the_scene(scene):
    cloud, e = scene.cloud, scene.edge
    r = 1.5 * e
    lat = nearest_reference.oracle.Lattice(cloud, e)
    unique, inverse, counts = np.unique(lat.coordinate_to_address(cloud), return_inverse=True, return_counts=True)
    assert len(unique) == scene.m
    top = scene.index.voxel_table(cloud[:, 2].copy(), reduce="max")[:, 0]
    want_top = np.full(scene.m, -np.inf)
    np.maximum.at(want_top, inverse, cloud[:, 2])
    assert np.array_equal(top, want_top)
    other = np.cos(3.0 * cloud[:, 0]) + np.sin(2.0 * cloud[:, 1])
    other_top = np.full(scene.m, -np.inf)
    np.maximum.at(other_top, inverse, other)
    point_class = (np.arange(len(cloud)) % 11 == 0).astype(np.int64) - (np.arange(len(cloud)) % 97 == 0)
    voxel_class = np.full(scene.m, 1 << 40)
    np.minimum.at(voxel_class, inverse, point_class)
    runs = ((None, top, "highest", None, None, 1), (None, top, "nearest", None, None, 12),
            (other, other_top, "highest", point_class, voxel_class, 5))
    for point_value, value, mode, pcls, vcls, min_points in runs:
        want = scene.want(r, value, mode, voxel_class=vcls, voxel_weight=counts, min_size=min_points)
        got = multiscale.peak_segments(cloud, e, r, point_value=point_value, link=mode, point_class=pcls,
                                       min_points=min_points)
        point_labels, sizes, peak_xyz, peak_value = got
        assert all(isinstance(t, np.ndarray) for t in got)
        assert point_labels.dtype == np.int64 and point_labels.shape == (len(cloud),)
        assert peak_xyz.shape == (len(sizes), 3) and peak_value.shape == sizes.shape and len(sizes) > 1
        assert np.array_equal(point_labels, want[0][inverse]) and np.array_equal(sizes, want[1])
        assert np.array_equal(peak_xyz, scene.voxels[want[2]]) and np.array_equal(peak_value, value[want[2]])
        assert np.array_equal(np.bincount(point_labels[point_labels >= 0], minlength=len(sizes)), sizes)
        if vcls is not None:
            assert (point_labels[voxel_class[inverse] < 0] == -1).all()
        if point_value is None and min_points == 1:
            # the top of the pole is a peak: the highest voxel of the scene
            assert peak_value.max() == cloud[:, 2].max()
        tensors = multiscale.peak_segments(torch.from_numpy(cloud).cuda(), e, r, link=mode, min_points=min_points,
                                           point_value=None if point_value is None else torch.from_numpy(point_value),
                                           point_class=None if pcls is None else torch.from_numpy(pcls).cuda())
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors)
        assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(tensors, got))
