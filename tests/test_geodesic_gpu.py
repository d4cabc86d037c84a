"""
GPU tests of NeighborIndex.geodesic / multiscale.geodesic_segments (nm_neighbors.hip: k_geo_init, k_geo_sweep, k_geo_link
and k_geo_orphans around the flatten, mark, scan and label kernels of components()) against the numpy reference of
tests/geodesic_reference.py, which test_geodesic_cpu.py pins to scipy's Dijkstra and to graphs worked by hand.  every
comparison is array_equal: labels, sizes, sources and links on int64, distances on their int64 BIT PATTERNS, so that
+inf, -0 and a last bit cannot hide.

the reference runs on the handle's own voxels; edges are found once per (case, radius) and shared, never changed.  the
kernel relaxes in place, in whatever order its lanes run, the reference all edges at once: equal bits on every case are
the proof that the order does not matter.

one check differs from the issue's wording.  it asks that finish, called after a single sweep of the serpentine with
its seed at one end, report voxels without a candidate.  it cannot: on a path with one seed the first finite value a
voxel gets is its final one, so every reached voxel has its predecessor as a candidate whatever the sweep's order was
(no run has reported any).  the test keeps that call - it must return normally and agree with the reference's links
and segments ON THE DISTANCES IT LEFT, whatever they are - and shows d_count[2] > 0, orphans and all, on a dist[] that
is short of the fixpoint by construction.
"""

import ctypes

import numpy as np
import pytest
import torch

import components_reference as cref
import geodesic_reference as ref
import nearest_reference
import regions_reference as rref
from nimrud_amd import _ffi
from nimrud_amd import device as _device
from nimrud_amd.minimal import multiscale

pytestmark = pytest.mark.gpu

E = ref.EDGE
INF = ref.INF


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

    def want(self, radius, seed, **kwargs):
        """the reference's (dist, labels, sizes, sources, link, total, sweeps)"""
        return ref.geodesic_of_edges(self.voxels, self.edges(radius), seed, **kwargs)

    def check(self, radius, seed, **kwargs):
        got = self.index.geodesic(radius, seed, return_link=True, **kwargs)
        want = self.want(radius, seed, **kwargs)
        print("M = %d, r = %g: %d reached, %d segments of %d seeds, %d reference sweeps" % (
            self.m, radius, (want[0] < INF).sum(), len(want[2]), want[5], want[6]))
        dist, labels, sizes, sources, link = got
        assert len(got) == 5 and dist.dtype == np.float64 and all(a.dtype == np.int64 for a in got[1:])
        assert dist.shape == labels.shape == link.shape == (self.m,) and sizes.shape == sources.shape == want[2].shape
        assert np.array_equal(ref.bits(dist), ref.bits(want[0]))
        assert np.array_equal(link, want[4])
        assert np.array_equal(labels, want[1])
        assert np.array_equal(sizes, want[2])
        assert np.array_equal(sources, want[3])
        return got


ANCHOR = (0, 4, 4)


def cells_graph(cells, anchor=ANCHOR):
    """a Graph of one point per cell, the cells listed in position order, and the anchor behind them: a lattice needs
    an extent on every axis.  the anchor is the last position and more than three edges from every other cell"""
    cells = np.asarray(list(cells) + [anchor], dtype=np.int64)
    g = Graph(cref.cells_cloud(cells))
    assert g.m == len(cells)
    assert np.array_equal(np.rint((g.voxels - g.voxels.min(axis=0)) / E), cells - cells.min(axis=0))
    return g


def hand(g, radius, seed, max_distance=None, voxel_class=None, voxel_weight=None, min_size=1):
    """g.check with the anchor's entries added to the arguments (no seed, class 0, weight 1) and taken off the
    results: nothing reaches it"""
    n = g.m - 1
    kwargs = dict(min_size=min_size, max_distance=max_distance)
    if voxel_class is not None:
        kwargs["voxel_class"] = np.append(voxel_class, 0)
    if voxel_weight is not None:
        kwargs["voxel_weight"] = np.append(voxel_weight, 1)
    dist, labels, sizes, sources, link = g.check(radius, np.append(np.asarray(seed, dtype=np.int64), 0), **kwargs)
    assert dist[n] == INF and labels[n] == -1 and link[n] == -1 and (link[:n] != n).all() and (sources != n).all()
    return dist[:n], labels[:n], sizes, sources, link[:n]


@pytest.fixture(scope="module")
def lattice():
    """the random sparse lattice of the components tests: 17 991 voxels, five scan tiles"""
    g = Graph(rref.lattice_cloud("random"))
    assert g.m == 17991
    return g


@pytest.fixture(scope="module")
def serpentine():
    """2 049 cells in one layer; at one edge the graph is the path, and the seed is its first cell, position 0"""
    cells = ref.in_position_order([tuple(c) for c in ref.serpentine_cells()])
    g = cells_graph(cells, anchor=(0, 0, 4))
    assert g.m == 2050 and len(g.edges(E)[0]) == 2048
    return g


@pytest.fixture(scope="module")
def scene():
    return Graph(nearest_reference.scene_cloud()[0], nearest_reference.SCENE_EDGE)


# ---- 1. - 7. the graphs worked by hand, on the device ------------------------------------------------------------------

def test_a_row():
    row = cells_graph(ref.row_cells(6))
    dist, labels, sizes, sources, link = hand(row, E, [1, 0, 0, 0, 0, 0])
    assert link.tolist() == [0, 0, 1, 2, 3, 4] and labels.tolist() == [0] * 6 and sources.tolist() == [0]
    running = np.add.accumulate(np.append(0.0, np.sqrt(((row.voxels[1:6] - row.voxels[:5]) ** 2).sum(axis=1))))
    assert np.array_equal(ref.bits(dist), ref.bits(running)) and sizes.tolist() == [6]
    dist, labels, sizes, sources, link = hand(row, E, [0, 0, 0, 0, 0, 1])
    assert link.tolist() == [1, 2, 3, 4, 5, 5] and sources.tolist() == [5]


def test_a_horseshoe_is_walked_round_and_a_larger_radius_jumps_the_gap():
    u = cells_graph(ref.horseshoe_cells())
    seed = [1, 0, 0, 0, 0, 0, 0]
    dist, labels, sizes, sources, link = hand(u, E, seed)
    assert link.tolist() == ref.HORSESHOE_LINK_1 and labels.tolist() == [0] * 7
    across = float(np.sqrt(((u.voxels[1] - u.voxels[0]) ** 2).sum()))
    assert dist[1] > 2.9 * across and dist[1] == dist.max()             # six steps round, two cells across
    dist, labels, sizes, sources, link = hand(u, 2 * E, seed)
    assert link.tolist() == ref.HORSESHOE_LINK_2 and dist[1] == across


def test_a_staircase_takes_the_diagonal():
    steps = cells_graph(ref.staircase_cells())
    dist, labels, sizes, sources, link = hand(steps, 1.5 * E, [1, 0, 0, 0, 0])
    assert link.tolist() == ref.STAIRCASE_LINK and dist[1] < dist[2] < dist[1] + dist[1]
    dist, labels, sizes, sources, link = hand(steps, E, [1, 0, 0, 0, 0])
    assert link.tolist() == [0, 0, 1, 2, 3]


def test_two_seeds_a_tie_goes_to_the_smaller_position():
    row = cells_graph(ref.row_cells(7))
    dist, labels, sizes, sources, link = hand(row, E, [1, 0, 0, 0, 0, 0, 1])
    # the middle voxel's two candidates: bit-equal distances, bit-equal sums - the smaller position, and its seed
    w = np.sqrt(((row.voxels[3] - row.voxels[[2, 4]]) ** 2).sum(axis=1))
    assert ref.bits(dist[2]) == ref.bits(dist[4])
    assert ref.bits(dist[2] + w[0]) == ref.bits(dist[4] + w[1]) == ref.bits(dist[3])
    assert link.tolist() == [0, 0, 1, 2, 5, 6, 6] and labels.tolist() == [0, 0, 0, 0, 1, 1, 1]
    assert sizes.tolist() == [4, 3] and sources.tolist() == [0, 6]
    row = cells_graph(ref.row_cells(8))
    dist, labels, sizes, sources, link = hand(row, E, [1, 0, 0, 0, 0, 1, 0, 0])
    assert labels.tolist() == [0, 0, 0, 1, 1, 1, 1, 1] and link.tolist() == [0, 0, 1, 4, 5, 5, 5, 6]


def test_classes_seeds_and_islands():
    row = cells_graph(ref.row_cells(7))
    seed = [1, 0, 0, 0, 0, 0, 0]
    for wall in (1, -1):
        dist, labels, sizes, sources, link = hand(row, E, seed, voxel_class=[0, 0, 0, wall, 0, 0, 0])
        assert (dist[:3] < INF).all() and (dist[3:] == INF).all()
        assert labels.tolist() == [0, 0, 0, -1, -1, -1, -1] and link.tolist() == [0, 0, 1, -1, -1, -1, -1]
    dist, labels, sizes, sources, link = hand(row, 2 * E, seed, voxel_class=[0, 0, 0, 1, 0, 0, 0])
    assert link.tolist() == [0, 0, 0, -1, 2, 4, 4] and dist[3] == INF
    # a seed of negative class is ignored
    dist, labels, sizes, sources, link = hand(row, E, [1, 0, 0, 0, 0, 0, 1], voxel_class=[0] * 6 + [-1])
    assert sources.tolist() == [0] and dist[6] == INF and link[6] == -1 and labels.tolist() == [0] * 6 + [-1]
    # an island without a seed; no seed at all; every voxel a seed
    gap = cells_graph([(0, 0, 0), (1, 0, 0), (3, 0, 0), (4, 0, 0)])
    dist, labels, sizes, sources, link = hand(gap, E, [1, 0, 0, 0])
    assert (dist[2:] == INF).all() and labels.tolist() == [0, 0, -1, -1] and link.tolist() == [0, 0, -1, -1]
    dist, labels, sizes, sources, link = hand(gap, E, [0, 0, 0, 0])
    assert (dist == INF).all() and (labels == -1).all() and (link == -1).all() and len(sizes) == len(sources) == 0
    dist, labels, sizes, sources, link = gap.check(E, np.ones(gap.m, dtype=np.uint8))
    assert np.array_equal(ref.bits(dist), np.zeros(gap.m, dtype=np.int64))
    assert labels.tolist() == link.tolist() == sources.tolist() == list(range(gap.m)) and (sizes == 1).all()
    # bool seeds, and a one-voxel index
    again = gap.index.geodesic(E, np.ones(gap.m, dtype=bool), return_link=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (dist, labels, sizes, sources, link)))
    one = Graph(np.array([[0.0, 0.0, 0.0], [0.01, 0.01, 0.01]]))
    assert one.m == 1
    dist, labels, sizes, sources, link = one.check(E, [1])
    assert dist.tolist() == [0.0] and labels.tolist() == link.tolist() == sources.tolist() == [0]
    dist, labels, sizes, sources, link = one.check(E, [0])
    assert dist.tolist() == [INF] and labels.tolist() == link.tolist() == [-1] and len(sources) == 0


def test_max_distance_is_inclusive_and_nothing_is_reached_through_what_lies_beyond():
    row = cells_graph(ref.row_cells(7))
    seed = [1, 0, 0, 0, 0, 0, 0]
    full = hand(row, E, seed)[0]
    dist, labels, sizes, sources, link = hand(row, E, seed, max_distance=float(full[3]))
    assert np.array_equal(ref.bits(dist[:4]), ref.bits(full[:4])) and (dist[4:] == INF).all()
    assert labels.tolist() == [0, 0, 0, 0, -1, -1, -1] and link.tolist() == [0, 0, 1, 2, -1, -1, -1]
    dist, labels, sizes, sources, link = hand(row, E, seed, max_distance=float(np.nextafter(full[3], 0.0)))
    assert (dist[:3] < INF).all() and (dist[3:] == INF).all()
    # at two edges voxel 4 is within reach of voxel 2, but every way to it is too long: nothing beyond the limit
    dist, labels, sizes, sources, link = hand(row, 2 * E, seed, max_distance=3.5 * E)
    assert (dist[:4] < INF).all() and (dist[4:] == INF).all()
    assert (hand(row, E, seed, max_distance=0.0)[0][1:] == INF).all()


def test_sizes_are_weight_sums_and_min_size_drops_segments_only():
    row = cells_graph(ref.row_cells(7))
    seed, weight = [1, 0, 0, 0, 0, 0, 1], [1, 1, 1, 1, 5, 5, 5]
    dist, labels, sizes, sources, link = hand(row, E, seed, voxel_weight=weight)
    assert sizes.tolist() == [4, 15]
    dist2, labels, sizes, sources, link2 = hand(row, E, seed, voxel_weight=weight, min_size=5)
    assert labels.tolist() == [-1, -1, -1, -1, 0, 0, 0] and sizes.tolist() == [15] and sources.tolist() == [6]
    assert np.array_equal(ref.bits(dist2), ref.bits(dist)) and np.array_equal(link2, link)


# ---- 8. the random lattice against the reference ------------------------------------------------------------------------

@pytest.mark.parametrize("rho,seeds,classes,limited", ref.LATTICE_CASES)
def test_the_random_lattice(lattice, rho, seeds, classes, limited):
    m, r = lattice.m, rho * E
    seed = ref.case_seeds(m, seeds)
    cls = ref.case_classes(m) if classes else None
    kwargs = {} if cls is None else dict(voxel_class=cls)
    if limited:
        kwargs["max_distance"] = ref.median_distance(lattice.want(r, seed, **kwargs)[0])
    dist, labels, sizes, sources, link = lattice.check(r, seed, **kwargs)
    # two identical calls are bit-equal
    again = lattice.index.geodesic(r, seed, return_link=True, **kwargs)
    assert np.array_equal(ref.bits(again[0]), ref.bits(dist))
    assert all(np.array_equal(a, b) for a, b in zip(again[1:], (labels, sizes, sources, link)))
    assert len(lattice.index.geodesic(r, seed, **kwargs)) == 4
    if limited:
        assert dist[dist < INF].max() == kwargs["max_distance"]
        return
    # a label exactly on the voxels whose component of the same graph holds a seed
    comp = lattice.index.components(r, cls)[0]
    in_graph = np.ones(m, dtype=bool) if cls is None else cls >= 0
    seeded = np.zeros(comp.max() + 1, dtype=bool)
    seeded[comp[seed & in_graph]] = True
    assert np.array_equal(labels >= 0, in_graph & seeded[np.maximum(comp, 0)])


def test_weights_min_size_and_classes_on_the_lattice(lattice):
    m = lattice.m
    seed, cls = ref.case_seeds(m, 200), ref.case_classes(m)
    weight = np.random.default_rng(3).integers(1, 6, m)
    dist, labels, sizes, sources, link = lattice.check(2.0 * E, seed, voxel_class=cls, voxel_weight=weight, min_size=40)
    assert sizes.min() >= 40 and ((labels < 0) & (dist < INF)).any()
    assert (dist[cls < 0] == INF).all() and (link[cls < 0] == -1).all() and np.array_equal(link >= 0, dist < INF)


# ---- 9. a path as long as the index -------------------------------------------------------------------------------------

def test_the_serpentine(serpentine):
    g = serpentine
    seed = np.zeros(g.m, dtype=np.uint8)
    seed[0] = 1
    dist, labels, sizes, sources, link = g.check(E, seed)
    n = g.m - 1
    assert (dist[:n] < INF).all() and sizes.tolist() == [n] and sources.tolist() == [0]
    steps, at = 0, np.arange(n)
    while (link[at] != at).any():
        at = link[at]
        steps += 1
    print("the longest chain has %d links, the farthest voxel is %.17g away" % (steps, dist[:n].max()))
    assert steps == n - 1 == 2048


# ---- 10. the C entry points: any split into calls, and a dist[] short of the fixpoint ---------------------------------------

def c_relax(index, radius, seed, dist, count, first, sweeps, cls=None, max_distance=INF, tmp=None, lattice="own"):
    """nm_neighbor_index_geodesic_relax itself: (status, message)"""
    rt = index._rt
    lat = index.filter.nm_lattice if isinstance(lattice, str) else lattice
    rc = rt.lib.nm_neighbor_index_geodesic_relax(
        rt.ctx, ctypes.byref(lat) if lat is not None else None, radius, _device.ptr(index._work),
        index._work.numel(), _device.ptr(seed), _device.ptr(cls), max_distance, first, sweeps, _device.ptr(dist),
        _device.ptr(count), _device.ptr(tmp), tmp.numel() if tmp is not None else 0, rt.stream())
    torch.cuda.synchronize()
    msg = rt.lib.nm_last_error(rt.ctx)
    return rc, (msg.decode("utf-8", "replace") if msg else "")


def c_finish(index, radius, dist, label, size, source, count, link=None, cls=None, weight=None, min_size=1, tmp=None,
             lattice="own"):
    """nm_neighbor_index_geodesic_finish itself: (status, message)"""
    rt = index._rt
    lat = index.filter.nm_lattice if isinstance(lattice, str) else lattice
    rc = rt.lib.nm_neighbor_index_geodesic_finish(
        rt.ctx, ctypes.byref(lat) if lat is not None else None, radius, _device.ptr(index._work),
        index._work.numel(), _device.ptr(cls), _device.ptr(weight), min_size, _device.ptr(dist), _device.ptr(label),
        _device.ptr(size), _device.ptr(source), _device.ptr(link), _device.ptr(count), _device.ptr(tmp),
        tmp.numel() if tmp is not None else 0, rt.stream())
    torch.cuda.synchronize()
    msg = rt.lib.nm_last_error(rt.ctx)
    return rc, (msg.decode("utf-8", "replace") if msg else "")


def scratch(index, voxels=None):
    nbytes = index._rt.lib.nm_neighbor_index_geodesic_workspace_bytes(index.n_voxels if voxels is None else voxels)
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


def filled(n, dtype=torch.int64):
    return torch.full((n,), -7, dtype=dtype, device="cuda")


def test_any_split_into_calls_ends_at_the_same_bits(lattice):
    index, m = lattice.index, lattice.m
    r = 2.0 * E
    host_seed, cls = ref.case_seeds(m, 7), ref.case_classes(m)
    want = lattice.want(r, host_seed, voxel_class=cls)
    seed = torch.from_numpy(host_seed.astype(np.uint8)).cuda()
    d_cls = torch.from_numpy(cls).cuda()
    tmp = scratch(index)
    for sweeps in (1, 5, 64):
        dist, count = filled(m, torch.float64), filled(1)
        calls, first = 0, 1
        while True:
            rc, msg = c_relax(index, r, seed, dist, count, first, sweeps, cls=d_cls, tmp=tmp)
            assert rc == _ffi.NM_OK, msg
            calls, first = calls + 1, 0
            lowered = int(count[0])
            assert 0 <= lowered <= m
            if lowered == 0:
                break
            assert calls * sweeps <= m + 1
        print("%d sweeps per call: %d calls (the reference: %d sweeps)" % (sweeps, calls, want[6]))
        # in place a sweep is never slower than the reference's, which reads the values of the sweep before only
        assert calls * sweeps <= want[6] + sweeps
        assert np.array_equal(ref.bits(dist.cpu().numpy()), ref.bits(want[0]))
        # once more: nothing is lowered, nothing changes
        rc, msg = c_relax(index, r, seed, dist, count, 0, 3, cls=d_cls, tmp=tmp)
        assert rc == _ffi.NM_OK and count.tolist() == [0]
        assert np.array_equal(ref.bits(dist.cpu().numpy()), ref.bits(want[0]))
    # finish on those distances: the counts, and entries behind C untouched
    label, size, source, link, count = filled(m), filled(m), filled(m), filled(m), filled(3)
    rc, msg = c_finish(index, r, dist, label, size, source, count, link=link, cls=d_cls, tmp=scratch(index))
    assert rc == _ffi.NM_OK, msg
    kept = len(want[2])
    assert count.tolist() == [kept, want[5], 0]
    assert np.array_equal(label.cpu().numpy(), want[1]) and np.array_equal(link.cpu().numpy(), want[4])
    assert np.array_equal(size[:kept].cpu().numpy(), want[2]) and np.array_equal(source[:kept].cpu().numpy(), want[3])
    assert (size[kept:] == -7).all() and (source[kept:] == -7).all()
    # d_link NULL: the rest is the same
    label2, size2, source2, count2 = filled(m), filled(m), filled(m), filled(3)
    rc, msg = c_finish(index, r, dist, label2, size2, source2, count2, cls=d_cls, tmp=tmp)
    assert rc == _ffi.NM_OK, msg
    assert torch.equal(label2, label) and torch.equal(size2, size) and torch.equal(source2, source)
    assert torch.equal(count2, count)


def finish_against_the_reference(g, host_dist):
    """finish on ANY dist[]: returns normally, and its links, orphans, labels, sizes and sources are the reference's"""
    index, m = g.index, g.m
    edges = ref.directed_edges(g.voxels, g.edges(E))
    want_link, orphans = ref.links(host_dist, edges)
    want_labels, want_sizes, want_sources, total = ref.segments(host_dist, want_link)
    dist = torch.from_numpy(host_dist).cuda()
    label, size, source, link, count = filled(m), filled(m), filled(m), filled(m), filled(3)
    rc, msg = c_finish(index, E, dist, label, size, source, count, link=link, tmp=scratch(index))
    assert rc == _ffi.NM_OK, msg
    kept = len(want_sizes)
    assert count.tolist() == [kept, total, orphans]
    label, link = label.cpu().numpy(), link.cpu().numpy()
    assert np.array_equal(link, want_link) and np.array_equal(label, want_labels)
    assert np.array_equal(size[:kept].cpu().numpy(), want_sizes)
    assert np.array_equal(source[:kept].cpu().numpy(), want_sources)
    assert not ((label >= 0) & (link < 0)).any()                 # no voxel with a label and link -1
    return orphans, label, link


def test_finish_before_the_fixpoint_is_a_defined_result(serpentine):
    g = serpentine
    index, m = g.index, g.m
    seed = torch.zeros(m, dtype=torch.uint8, device="cuda")
    seed[0] = 1
    # a single sweep: some stretch of the path is reached (which, depends on the order the lanes ran in)
    dist, count = filled(m, torch.float64), filled(1)
    rc, msg = c_relax(index, E, seed, dist, count, 1, 1, tmp=scratch(index))
    assert rc == _ffi.NM_OK, msg
    after_one = dist.cpu().numpy()
    reached = int((after_one < INF).sum())
    print("one sweep reached %d of %d voxels and lowered %d" % (reached, m - 1, int(count[0])))
    assert 2 <= reached < m - 1 and int(count[0]) == reached - 1
    orphans, label, link = finish_against_the_reference(g, after_one)
    assert orphans == 0 and (label[after_one < INF] == 0).all()   # (one seed on a path: see the module's docstring)
    # short of the fixpoint by construction: a stretch of the path forgotten, what lies behind it kept
    full = g.want(E, seed.cpu().numpy())[0]
    on_path = np.argsort(full[:m - 1])
    broken = full.copy()
    broken[on_path[100:200]] = INF
    orphans, label, link = finish_against_the_reference(g, broken)
    assert orphans == 1 and link[on_path[200]] == -1 and (label[on_path[200:]] == -1).all()
    assert (label[on_path[:100]] == 0).all() and (link[on_path[201:]] >= 0).all()
    # several orphans, chains of every length below them, and a NaN
    broken = full.copy()
    broken[on_path[50::97]] = INF
    broken[on_path[31]] = float("nan")
    orphans, label, link = finish_against_the_reference(g, broken)
    assert orphans == len(on_path[50::97]) + 1 - (1 if (len(on_path) - 1 - 50) % 97 == 0 else 0)
    # the Python call refuses such distances only through finish's count: at the fixpoint there is none
    assert g.index.geodesic(E, seed.cpu().numpy())[1][:m - 1].min() == 0


# ---- 11. scratch and errors ------------------------------------------------------------------------------------------------

def test_a_scratch_without_room_and_the_error_statuses(lattice):
    index, m = lattice.index, lattice.m
    rt = index._rt
    seed = torch.from_numpy(ref.case_seeds(m, 7).astype(np.uint8)).cuda()
    dist, count1 = filled(m, torch.float64), filled(1)
    label, size, source, link, count3 = filled(m), filled(m), filled(m), filled(m), filled(3)
    good = scratch(index)
    short = torch.empty(64, dtype=torch.uint8, device="cuda")

    def untouched():
        return bool((dist == -7).all() and (label == -7).all() and (size == -7).all() and (source == -7).all() and
                    (link == -7).all())

    relax_cases = [
        (dict(seed=None), _ffi.NM_ERR_INVALID),
        (dict(dist=None), _ffi.NM_ERR_INVALID),
        (dict(count=None), _ffi.NM_ERR_INVALID),
        (dict(lattice=None), _ffi.NM_ERR_INVALID),
        (dict(radius=float("nan")), _ffi.NM_ERR_INVALID),
        (dict(radius=-0.01), _ffi.NM_ERR_INVALID),
        (dict(max_distance=float("nan")), _ffi.NM_ERR_INVALID),
        (dict(max_distance=-1.0), _ffi.NM_ERR_INVALID),
        (dict(sweeps=0), _ffi.NM_ERR_INVALID),
        (dict(sweeps=-3), _ffi.NM_ERR_INVALID),
        (dict(radius=1e6), _ffi.NM_ERR_RADIUS),
        (dict(tmp=short), _ffi.NM_ERR_WORKSPACE),
        (dict(tmp=None), _ffi.NM_ERR_WORKSPACE),
    ]
    for change, status in relax_cases:
        args = dict(radius=E, seed=seed, dist=dist, count=count1, first=1, sweeps=2, tmp=good)
        args.update(change)
        rc, msg = c_relax(index, **args)
        assert rc == status and msg, (change, rc, msg)
        assert untouched() and (count1 == -7).all(), change
    finish_cases = [
        (dict(dist=None), _ffi.NM_ERR_INVALID),
        (dict(label=None), _ffi.NM_ERR_INVALID),
        (dict(size=None), _ffi.NM_ERR_INVALID),
        (dict(source=None), _ffi.NM_ERR_INVALID),
        (dict(count=None), _ffi.NM_ERR_INVALID),
        (dict(lattice=None), _ffi.NM_ERR_INVALID),
        (dict(radius=float("nan")), _ffi.NM_ERR_INVALID),
        (dict(radius=-0.01), _ffi.NM_ERR_INVALID),
        (dict(radius=1e6), _ffi.NM_ERR_RADIUS),
        (dict(tmp=short), _ffi.NM_ERR_WORKSPACE),
        (dict(tmp=None), _ffi.NM_ERR_WORKSPACE),
    ]
    for change, status in finish_cases:
        args = dict(radius=E, dist=dist, label=label, size=size, source=source, count=count3, link=link, tmp=good)
        args.update(change)
        rc, msg = c_finish(index, **args)
        assert rc == status and msg, (change, rc, msg)
        assert untouched() and (count3 == -7).all(), change
    rt.check_async(wait=True)                # nothing sticky: the context is as usable as before
    # a scratch that takes the minimum but not this index's M: refused on the device, nothing written
    least = scratch(index, 0)
    assert least.numel() < good.numel()
    rc, msg = c_relax(index, E, seed, dist, count1, 1, 3, tmp=least)
    assert rc == _ffi.NM_OK and count1.tolist() == [-1] and untouched()
    rc, msg = c_relax(index, E, seed, dist, count1, 0, 1, tmp=least)
    assert rc == _ffi.NM_OK and count1.tolist() == [-1] and untouched()
    rc, msg = c_finish(index, E, dist, label, size, source, count3, link=link, tmp=least)
    assert rc == _ffi.NM_OK and count3.tolist() == [-1, -1, -1] and untouched()


def test_argument_errors_in_python(scene):
    index, m = scene.index, scene.m
    seed = np.zeros(m, dtype=np.uint8)
    seed[0] = 1
    for bad in (float("nan"), -1.0, 1e6):
        with pytest.raises(ValueError):
            index.geodesic(bad, seed)
    for bad in (seed[:-1], np.zeros((m, 1), dtype=np.uint8), np.zeros(m), torch.zeros(m, dtype=torch.float32)):
        with pytest.raises(ValueError):
            index.geodesic(scene.edge, bad)
    for bad in (float("nan"), -0.5, "far"):
        with pytest.raises(ValueError):
            index.geodesic(scene.edge, seed, max_distance=bad)
    for name in ("voxel_class", "voxel_weight"):
        for bad in (np.zeros(m - 1, dtype=np.int64), np.zeros((m, 1), dtype=np.int64), np.zeros(m)):
            with pytest.raises(ValueError):
                index.geodesic(scene.edge, seed, **{name: bad})
    for bad in (1.5, "2", None, True):
        with pytest.raises(ValueError):
            index.geodesic(scene.edge, seed, min_size=bad)
    searching = multiscale.NeighborIndex(scene.cloud, scene.edge, method="search")
    with pytest.raises(ValueError, match="index form"):
        searching.geodesic(scene.edge, seed)
    point_seed = np.zeros(len(scene.cloud), dtype=bool)
    with pytest.raises(ValueError):
        multiscale.geodesic_segments(scene.cloud, scene.edge, -1.0, point_seed)
    with pytest.raises(ValueError):
        multiscale.geodesic_segments(scene.cloud, scene.edge, scene.edge, point_seed[:-1])
    with pytest.raises(ValueError):
        multiscale.geodesic_segments(scene.cloud, scene.edge, scene.edge, point_seed, max_distance=-1.0)
    with pytest.raises(ValueError):
        multiscale.geodesic_segments(scene.cloud, scene.edge, scene.edge, point_seed, min_points=2.5)
    with pytest.raises(ValueError):
        multiscale.geodesic_segments(scene.cloud, scene.edge, scene.edge, point_seed,
                                     point_class=np.zeros(len(scene.cloud)))
    index._rt.check_async(wait=True)


def test_torch_stays_torch_and_other_dtypes(lattice):
    m = lattice.m
    cloud = torch.from_numpy(lattice.cloud).cuda()
    index = multiscale.NeighborIndex(cloud, E, method="index")
    host_seed, cls = ref.case_seeds(m, 7), ref.case_classes(m)
    want = lattice.want(2.0 * E, host_seed, voxel_class=cls, voxel_weight=index.point_counts().cpu().numpy(),
                        min_size=2)
    a = index.geodesic(2.0 * E, torch.from_numpy(host_seed).cuda(), voxel_class=torch.from_numpy(cls.astype(np.int32)),
                       voxel_weight=index.point_counts(), min_size=2, return_link=True)
    assert len(a) == 5 and all(isinstance(t, torch.Tensor) and t.is_cuda for t in a)
    assert a[0].dtype == torch.float64 and all(t.dtype == torch.int64 for t in a[1:])
    assert np.array_equal(ref.bits(a[0].cpu().numpy()), ref.bits(want[0]))
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(a[1:], (want[1], want[2], want[3], want[4])))
    b = index.geodesic(2.0 * E, host_seed.astype(np.int16) * 3, voxel_class=cls.astype(np.int8),
                       voxel_weight=index.point_counts(), min_size=2, return_link=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 12. geodesic_segments ----------------------------------------------------------------------------------------------------

def test_geodesic_segments_on_the_scene(scene):
    cloud, e = scene.cloud, scene.edge
    r = 1.5 * e
    lat = nearest_reference.oracle.Lattice(cloud, e)
    unique, inverse, counts = np.unique(lat.coordinate_to_address(cloud), return_inverse=True, return_counts=True)
    assert len(unique) == scene.m
    # seeds: a few points of the plane (the first 1800), a few of the blob (the last 800); the pole has none
    point_seed = np.zeros(len(cloud), dtype=bool)
    point_seed[[5, 700, 1500, 2300, 2900]] = True
    voxel_seed = np.zeros(scene.m, dtype=bool)
    voxel_seed[inverse[point_seed]] = True
    point_class = (np.arange(len(cloud)) % 11 == 0).astype(np.int64) - (np.arange(len(cloud)) % 97 == 0)
    voxel_class = np.full(scene.m, 1 << 40)
    np.minimum.at(voxel_class, inverse, point_class)
    runs = ((None, None, None, 1), (None, None, 2.0, 12), (point_class, voxel_class, None, 3))
    for pcls, vcls, limit, min_points in runs:
        want = scene.want(r, voxel_seed, max_distance=limit, voxel_class=vcls, voxel_weight=counts,
                          min_size=min_points)
        got = multiscale.geodesic_segments(cloud, e, r, point_seed, max_distance=limit, point_class=pcls,
                                           min_points=min_points)
        point_distance, point_labels, sizes, source_xyz = got
        assert all(isinstance(t, np.ndarray) for t in got)
        assert point_labels.dtype == np.int64 and point_labels.shape == point_distance.shape == (len(cloud),)
        assert source_xyz.shape == (len(sizes), 3) and len(sizes) >= 1
        assert np.array_equal(ref.bits(point_distance), ref.bits(want[0][inverse]))
        assert np.array_equal(point_labels, want[1][inverse]) and np.array_equal(sizes, want[2])
        assert np.array_equal(source_xyz, scene.voxels[want[3]])
        assert np.array_equal(np.bincount(point_labels[point_labels >= 0], minlength=len(sizes)), sizes)
        if limit is not None:
            assert point_distance[point_distance < INF].max() <= limit and (point_distance == INF).any()
        if vcls is not None:
            assert (point_labels[voxel_class[inverse] < 0] == -1).all()
        tensors = multiscale.geodesic_segments(torch.from_numpy(cloud).cuda(), e, r, torch.from_numpy(point_seed),
                                               max_distance=limit, min_points=min_points,
                                               point_class=None if pcls is None else torch.from_numpy(pcls).cuda())
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors)
        assert np.array_equal(ref.bits(tensors[0].cpu().numpy()), ref.bits(point_distance))
        assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(tensors[1:], got[1:]))
