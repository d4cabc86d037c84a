"""
GPU tests of NeighborIndex.adjacency / NeighborIndex.prominent_peaks / multiscale.prominent_segments (nm_neighbors.hip:
k_adj_walk, k_adj_heads, k_adj_reduce, k_adj_saddles; nm_api.hip: nm_merge_by_prominence) against the numpy reference
of tests/adjacency_reference.py, which test_adjacency_cpu.py pins to graphs worked out by hand.  every comparison is
array_equal, on the handle's own voxels; every call is made twice and the two results are the same bit for bit.

the reference's edges are found once per (graph, radius) and shared, never changed.
"""

import numpy as np
import pytest
import torch

import adjacency_reference as ref
import components_reference as cref
import hill_climb_reference as href
import nearest_reference
from nimrud_amd import synth
from nimrud_amd.minimal import multiscale

pytestmark = pytest.mark.gpu

E = ref.EDGE
INF = float("inf")


def bits(a):
    """an array as integers: equal bits, not equal numbers"""
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(x, y):
    return len(x) == len(y) and all(
        (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b)))
        for a, b in zip(x, y))


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

    def basins(self, radius, value, mode="highest", cls=None):
        """the reference's hill_climb labels"""
        return href.hill_climb_of_edges(self.voxels, self.edges(radius), value, mode, voxel_class=cls)[0]

    def check(self, radius, labels, value=None, cls=None):
        """adjacency on the device, twice, against the reference"""
        got = self.index.adjacency(radius, labels, voxel_value=value, voxel_class=cls)
        again = self.index.adjacency(radius, labels, voxel_value=value, voxel_class=cls)
        want = ref.adjacency_of_edges(labels, self.edges(radius), value, cls)
        pair, links, saddle = got
        print("M = %d, r = %g: %d rows, %d crossing edges of %d" % (
            self.m, radius, len(want[0]), want[1].sum(), len(self.edges(radius)[0])))
        assert same_bits(got, again)
        assert pair.dtype == np.int64 and links.dtype == np.int64 and pair.shape == (len(links), 2)
        assert np.array_equal(pair, want[0]) and np.array_equal(links, want[1])
        if value is None:
            assert saddle is None
        else:
            assert saddle.dtype == np.float64 and np.array_equal(saddle, want[2])
        return got

    def check_peaks(self, radius, value, tau, mode="highest", cls=None, weight=None, min_size=1):
        """prominent_peaks on the device, twice, against the reference"""
        kwargs = dict(link=mode, voxel_class=cls, voxel_weight=weight, min_size=min_size)
        got = self.index.prominent_peaks(radius, value, tau, **kwargs)
        again = self.index.prominent_peaks(radius, value, tau, **kwargs)
        want = ref.prominent_peaks_of_edges(self.voxels, self.edges(radius), value, tau, mode, voxel_class=cls,
                                            voxel_weight=weight, min_size=min_size)
        print("M = %d, r = %g, %s, min_prominence = %g: %d segments" % (self.m, radius, mode, tau, len(want[1])))
        assert same_bits(got, again)
        assert len(got) == 4 and [a.dtype for a in got] == [np.int64, np.int64, np.int64, np.float64]
        assert got[0].shape == (self.m,)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        return got


ANCHOR = (0, 4, 4)


def cells_graph(cells):
    """a Graph of one point per cell, the cells listed in position order, and the ANCHOR behind them: a lattice needs
    an extent on every axis.  the anchor is the last position and more than three edges from every other cell"""
    cells = np.asarray(list(cells) + [ANCHOR], dtype=np.int64)
    g = Graph(cref.cells_cloud(cells))
    assert g.m == len(cells)
    return g


def hand_rows(g, radius, labels, value=None, cls=None):
    """g.check with the anchor (label -1, value 0, class 0) behind the arguments; the results as lists"""
    labels = np.append(np.asarray(labels, dtype=np.int64), -1)
    value = None if value is None else np.append(np.asarray(value, dtype=np.float64), 0.0)
    cls = None if cls is None else np.append(np.asarray(cls, dtype=np.int64), 0)
    pair, links, saddle = g.check(radius, labels, value, cls)
    return pair.tolist(), links.tolist(), None if saddle is None else saddle.tolist()


def hand_peaks(g, radius, value, tau, **kwargs):
    """g.check_peaks with the anchor (value -1000: the lowest peak, alone, the last segment) taken off the results"""
    n = g.m - 1
    weight = kwargs.get("weight")
    kwargs["weight"] = np.append(np.ones(n, dtype=np.int64) if weight is None else weight, 1000)
    labels, sizes, peaks, prom = g.check_peaks(radius, np.append(np.asarray(value, dtype=np.float64), -1000.0), tau,
                                               **kwargs)
    assert peaks[-1] == n and labels[n] == len(sizes) - 1 and prom[-1] == INF
    return labels[:n].tolist(), sizes[:-1].tolist(), peaks[:-1].tolist(), prom[:-1].tolist()


@pytest.fixture(scope="module")
def uniform():
    """2 000 points, uniform in a 5 m cube, at an edge of 0.25: about 1 900 of the 8 000 cells are occupied"""
    g = Graph(np.random.default_rng(41).random((2000, 3)) * 5.0)
    assert 1700 < g.m <= 2000
    return g


@pytest.fixture(scope="module")
def sparse():
    """a plane and a pole, about 3 000 points in 8 m: most superblocks of the lattice are empty"""
    cloud, kind = synth.scene_cloud(4300, extent=8.0, n_poles=1, n_spheres=1, seed=9)
    cloud = np.ascontiguousarray(cloud[kind != 2])            # (the generator always makes a sphere: left out)
    assert 2900 < len(cloud) < 3100
    return Graph(cloud)


@pytest.fixture(scope="module")
def scene():
    return Graph(nearest_reference.scene_cloud()[0], nearest_reference.SCENE_EDGE)


RHOS = [1.0, 2.0 ** 0.5, 2.0, 3.0]


def random_values(m, seed=2):
    return np.random.default_rng(seed).random(m)


def scattered_labels(m, n_labels=60, seed=6):
    """`n_labels` labels scattered over the voxels, one in ten of them -1: almost every edge crosses"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, n_labels, m)
    labels[rng.random(m) < 0.1] = -1
    return labels


# ---- 1. the graphs worked out by hand, on the device -------------------------------------------------------------------

def test_the_hand_graphs():
    line = cells_graph(ref.row_cells(5))
    assert hand_rows(line, E, ref.LINE_LABELS, ref.LINE_VALUES) == ([[0, 1]], [1], [2.0])
    assert hand_rows(line, E, ref.LINE_LABELS) == ([[0, 1]], [1], None)
    assert hand_rows(line, E, [2, -1, 7, 7, 0], ref.LINE_VALUES) == ([[0, 7]], [1], [4.0])
    assert hand_rows(line, E, [0, 0, -1, 1, 1], ref.LINE_VALUES) == ([], [], [])
    # two classes side by side, a negative class, a NaN on the only bridge: no row
    for cls in ([0, 0, 1, 1, 1], [0, 0, -1, 1, 1], [0, -1, -1, 0, 0]):
        assert hand_rows(line, E, ref.LINE_LABELS, ref.LINE_VALUES, cls) == ([], [], [])
    assert hand_rows(line, E, ref.LINE_LABELS, [1.0, 3.0, float("nan"), 5.0, 4.0]) == ([], [], [])
    assert hand_rows(line, E, ref.LINE_LABELS, [1.0, float("nan"), 2.0, 5.0, 4.0]) == ([], [], [])
    # several edges between one pair: every edge once, the saddle the maximum and not the first
    four = cells_graph(ref.row_cells(4))
    assert hand_rows(four, 2 * E, [0, 0, 1, 1], [1.0, 5.0, 2.0, 4.0]) == ([[0, 1]], [3], [4.0])
    assert hand_rows(four, 2 * E, [1, 1, 0, 0], [1.0, 5.0, 2.0, 4.0]) == ([[0, 1]], [3], [4.0])
    assert hand_rows(four, 2 * E, [5, 0, 5, 3], [1.0, 5.0, 2.0, 4.0]) == ([[0, 3], [0, 5], [3, 5]], [1, 2, 1],
                                                                          [4.0, 2.0, 2.0])
    # -0 and +0 are one number
    pair, links, saddle = hand_rows(four, E, [0, 0, 1, 1], [1.0, -0.0, 0.0, 1.0])
    assert saddle == [0.0]
    # the line of five: the lower peak's prominence is exactly 1, and the test is strict
    for mode in href.MODES:
        assert hand_peaks(line, E, ref.LINE_VALUES, 1.0, mode=mode) == ([0, 0, 1, 1, 1], [2, 3], [1, 3], [1.0, INF])
        assert hand_peaks(line, E, ref.LINE_VALUES, np.nextafter(1.0, 2), mode=mode) == ([0] * 5, [5], [3], [INF])
        assert hand_peaks(line, E, ref.LINE_VALUES, INF, mode=mode) == ([0] * 5, [5], [3], [INF])
    # min_size acts after the merge
    assert hand_peaks(line, E, ref.LINE_VALUES, 2.0, min_size=3) == ([0] * 5, [5], [3], [INF])
    assert hand_peaks(line, E, ref.LINE_VALUES, 0.5, min_size=3) == ([-1, -1, 0, 0, 0], [3], [3], [INF])
    assert hand_peaks(line, E, ref.LINE_VALUES, 0.5, weight=[4, 4, 1, 1, 1], min_size=4) == (
        [0, 0, -1, -1, -1], [8], [1], [1.0])
    # three peaks in a chain
    seven = cells_graph(ref.row_cells(7))
    values = ref.chain_values(10.0, 8.0, 6.0, s_ab=4.0, s_bc=5.0)
    assert hand_peaks(seven, E, values, 2.0) == ([0, 0, 0, 1, 1, 1, 1], [3, 4], [1, 3], [INF, 4.0])
    assert hand_peaks(seven, E, values, 4.5) == ([0] * 7, [7], [1], [INF])
    assert hand_peaks(seven, E, values, 1.0)[3] == [INF, 4.0, 1.0]
    values = ref.chain_values(10.0, 6.0, 8.0, s_ab=5.5, s_bc=5.0)
    assert hand_peaks(seven, E, values, 1.0) == ([0, 0, 0, 0, 1, 1, 1], [4, 3], [1, 5], [INF, 3.0])
    # a plateau that splits: the pass lies at the peaks' own value
    u = cells_graph(href.u_cells())
    assert hand_peaks(u, E, np.zeros(13), 0.0) == (href.U_LABELS, [9, 4], [0, 8], [INF, 0.0])
    assert hand_peaks(u, E, np.zeros(13), 5e-324) == ([0] * 13, [13], [0], [INF])


# ---- 2. the uniform cloud against the reference ---------------------------------------------------------------------------

@pytest.mark.parametrize("levels", [0, 8])
@pytest.mark.parametrize("rho", RHOS)
def test_basins_of_the_uniform_cloud(uniform, rho, levels):
    value = random_values(uniform.m)
    if levels:
        value = ref.quantised(value, levels)
    labels = uniform.basins(rho * E, value)
    pair, links, saddle = uniform.check(rho * E, labels, value)
    assert len(pair) > 10


@pytest.mark.parametrize("rho", RHOS)
def test_labels_that_are_no_basins(uniform, rho):
    labels = scattered_labels(uniform.m)
    value = ref.quantised(random_values(uniform.m, seed=4), 8)
    pair, links, saddle = uniform.check(rho * E, labels, value)
    assert len(pair) <= 60 * 59 // 2
    if rho == 3.0:
        assert len(pair) > 1500 and links.max() > 15
    # three labels: three rows of many records each, at three edges runs that span waves and blocks
    pair, links, saddle = uniform.check(rho * E, scattered_labels(uniform.m, n_labels=3, seed=9), value)
    assert pair.tolist() == [[0, 1], [0, 2], [1, 2]]
    if rho == 3.0:
        assert links.min() > 256          # every row is more than a block of records


def test_labels_near_the_limit(uniform):
    top = (1 << 31) - 1
    labels = scattered_labels(uniform.m)
    high = np.where(labels >= 0, labels + (top - 59), -1)
    assert high.max() == top
    value = random_values(uniform.m, seed=4)
    low_rows = uniform.check(2 * E, labels, value)
    high_rows = uniform.check(2 * E, high, value)
    assert np.array_equal(high_rows[0], low_rows[0] + (top - 59)) and same_bits(high_rows[1:], low_rows[1:])
    # one label 0 among them: the pair's halves are as far apart as they get
    mixed = np.where(labels == 7, 0, high)
    uniform.check(2 * E, mixed, value)


@pytest.mark.parametrize("rho", [1.0, 3.0])
def test_classes_and_nan(uniform, rho):
    rng = np.random.default_rng(12)
    cls = rng.integers(-1, 2, uniform.m) * 5            # -5, 0, 5
    value = random_values(uniform.m, seed=8)
    value[rng.random(uniform.m) < 0.05] = np.nan
    uniform.check(rho * E, scattered_labels(uniform.m, n_labels=12), value, cls)
    labels = uniform.basins(rho * E, value, cls=cls)
    assert (labels[(cls < 0) | np.isnan(value)] == -1).all()
    uniform.check(rho * E, labels, value, cls)
    # the classes alone, the values alone
    uniform.check(rho * E, scattered_labels(uniform.m, n_labels=12), None, cls)
    uniform.check(rho * E, scattered_labels(uniform.m, n_labels=12), value, None)


def test_empty_and_trivial(uniform):
    value = random_values(uniform.m)
    labels = scattered_labels(uniform.m)
    for rows in (uniform.check(2 * E, np.zeros(uniform.m, dtype=np.int64), value),
                 uniform.check(2 * E, np.full(uniform.m, -1), value),
                 uniform.check(0.0, labels, value),
                 uniform.check(0.99 * E, labels, value)):
        assert rows[0].shape == (0, 2) and rows[1].shape == (0,) and rows[2].shape == (0,)
    rows = uniform.check(0.0, labels)
    assert rows[0].shape == (0, 2) and rows[1].shape == (0,) and rows[2] is None
    with_value = uniform.check(2 * E, labels, value)
    without = uniform.check(2 * E, labels)
    assert without[2] is None and same_bits(without[:2], with_value[:2])


@pytest.mark.parametrize("rho", [1.0, 3.0])
def test_sparse_structures(sparse, rho):
    value = sparse.voxels[:, 2] + 0.05 * random_values(sparse.m, seed=3)
    labels = sparse.basins(rho * E, value)
    pair, links, saddle = sparse.check(rho * E, labels, value)
    assert len(pair) > 10
    sparse.check(rho * E, scattered_labels(sparse.m), ref.quantised(value, 8))


# ---- 3. prominent_peaks -------------------------------------------------------------------------------------------------

def peaks_at_three_thresholds(g, radius, value, mode, cls=None):
    at_zero = g.check_peaks(radius, value, 0.0, mode, cls)
    climbed = g.index.hill_climb(radius, value, link=mode, voxel_class=cls)
    assert same_bits(at_zero[:3], climbed)
    finite = at_zero[3][np.isfinite(at_zero[3])]
    assert len(finite) > 4
    tau = float(np.median(finite))
    at_median = g.check_peaks(radius, value, tau, mode, cls)
    assert len(at_median[1]) <= len(at_zero[1])
    at_inf = g.check_peaks(radius, value, INF, mode, cls)
    graph_class = np.where(np.isnan(value), -1, 0 if cls is None else cls)
    pieces, piece_sizes = g.index.components(radius, voxel_class=graph_class)
    assert ref.same_partition(at_inf[0], pieces) and np.array_equal(np.sort(at_inf[1]), np.sort(piece_sizes))
    assert (at_inf[3] == INF).all()
    # with weights and a least size, at the median
    weight = np.random.default_rng(1).integers(1, 6, g.m)
    kept = g.check_peaks(radius, value, tau, mode, cls, weight=weight, min_size=12)
    assert len(kept[1]) <= len(at_median[1]) and (kept[1] >= 12).all()
    assert (kept[0] < 0).sum() >= (at_median[0] < 0).sum()


@pytest.mark.parametrize("mode", href.MODES)
@pytest.mark.parametrize("rho", [1.0, 2.0])
def test_prominent_peaks_of_the_uniform_cloud(uniform, rho, mode):
    peaks_at_three_thresholds(uniform, rho * E, random_values(uniform.m), mode)


@pytest.mark.parametrize("mode", href.MODES)
def test_prominent_peaks_on_levels_classes_and_nan(uniform, mode):
    rng = np.random.default_rng(13)
    value = ref.quantised(random_values(uniform.m), 8)
    value[rng.random(uniform.m) < 0.05] = np.nan
    cls = rng.integers(-1, 2, uniform.m) * 5
    peaks_at_three_thresholds(uniform, 2.0 ** 0.5 * E, value, mode, cls)


@pytest.mark.parametrize("mode", href.MODES)
def test_prominent_peaks_of_sparse_structures(sparse, mode):
    value = sparse.voxels[:, 2] + 0.05 * random_values(sparse.m, seed=3)
    peaks_at_three_thresholds(sparse, 2 * E, value, mode)


# ---- 4. prominent_segments ------------------------------------------------------------------------------------------------

def test_prominent_segments_on_the_scene(scene):
    cloud, e = scene.cloud, scene.edge
    assert len(cloud) == 3000
    r = 1.5 * e
    lat = nearest_reference.oracle.Lattice(cloud, e)
    unique, inverse, counts = np.unique(lat.coordinate_to_address(cloud), return_inverse=True, return_counts=True)
    assert len(unique) == scene.m
    top = np.full(scene.m, -np.inf)
    np.maximum.at(top, inverse, cloud[:, 2])
    other = np.cos(3.0 * cloud[:, 0]) + np.sin(2.0 * cloud[:, 1])
    other_top = np.full(scene.m, -np.inf)
    np.maximum.at(other_top, inverse, other)
    point_class = (np.arange(len(cloud)) % 11 == 0).astype(np.int64) - (np.arange(len(cloud)) % 97 == 0)
    voxel_class = np.full(scene.m, 1 << 40)
    np.minimum.at(voxel_class, inverse, point_class)
    runs = ((None, top, "highest", None, None, 1, 0.3), (None, top, "nearest", None, None, 12, 0.1),
            (other, other_top, "highest", point_class, voxel_class, 5, 0.05))
    for point_value, value, mode, pcls, vcls, min_points, tau in runs:
        want = ref.prominent_peaks_of_edges(scene.voxels, scene.edges(r), value, tau, mode, voxel_class=vcls,
                                            voxel_weight=counts, min_size=min_points)
        plain = href.hill_climb_of_edges(scene.voxels, scene.edges(r), value, mode, voxel_class=vcls,
                                         voxel_weight=counts, min_size=min_points)
        print("%s: %d segments of hill_climb's %d" % (mode, len(want[1]), len(plain[1])))
        assert 1 <= len(want[1]) <= len(plain[1])
        got = multiscale.prominent_segments(cloud, e, r, tau, point_value=point_value, link=mode, point_class=pcls,
                                            min_points=min_points)
        point_labels, sizes, peak_xyz, peak_value, prominence = got
        assert len(got) == 5 and all(isinstance(t, np.ndarray) for t in got)
        assert point_labels.dtype == np.int64 and point_labels.shape == (len(cloud),)
        assert np.array_equal(point_labels, want[0][inverse]) and np.array_equal(sizes, want[1])
        assert np.array_equal(peak_xyz, scene.voxels[want[2]]) and np.array_equal(peak_value, value[want[2]])
        assert prominence.dtype == np.float64 and np.array_equal(prominence, want[3])
        assert np.array_equal(np.bincount(point_labels[point_labels >= 0], minlength=len(sizes)), sizes)
        tensors = multiscale.prominent_segments(
            torch.from_numpy(cloud).cuda(), e, r, tau, link=mode, min_points=min_points,
            point_value=None if point_value is None else torch.from_numpy(point_value),
            point_class=None if pcls is None else torch.from_numpy(pcls).cuda())
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors)
        assert same_bits([t.cpu().numpy() for t in tensors], got)


def test_torch_stays_torch(uniform):
    index = multiscale.NeighborIndex(torch.from_numpy(uniform.cloud).cuda(), E, method="index")
    labels = scattered_labels(uniform.m)
    value = random_values(uniform.m).astype(np.float32)
    cls = np.random.default_rng(12).integers(-1, 2, uniform.m)
    want = ref.adjacency_of_edges(labels, uniform.edges(2 * E), value.astype(np.float64), cls)
    got = index.adjacency(2 * E, torch.from_numpy(labels.astype(np.int32)).cuda(), torch.from_numpy(value).cuda(),
                          torch.from_numpy(cls))
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got)
    assert [t.dtype for t in got] == [torch.int64, torch.int64, torch.float64]
    assert all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(got, want))
    # numpy arguments to a torch handle, no classes: torch out all the same
    got = index.adjacency(2 * E, labels)
    want_plain = ref.adjacency_of_edges(labels, uniform.edges(2 * E))
    assert got[2] is None and all(t.is_cuda and np.array_equal(t.cpu().numpy(), w) for t, w in zip(got[:2], want_plain))
    peaks = index.prominent_peaks(2 * E, torch.from_numpy(value).cuda(), 0.2, voxel_class=cls)
    want = ref.prominent_peaks_of_edges(uniform.voxels, uniform.edges(2 * E), value.astype(np.float64), 0.2,
                                        voxel_class=cls)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in peaks)
    assert all(np.array_equal(t.cpu().numpy(), w) for t, w in zip(peaks, want))


# ---- 5. argument errors -----------------------------------------------------------------------------------------------------

def test_argument_errors(uniform):
    index, m = uniform.index, uniform.m
    labels, value = np.zeros(m, dtype=np.int64), np.zeros(m)
    searching = multiscale.NeighborIndex(uniform.cloud, E, method="search")
    with pytest.raises(ValueError, match="index form"):
        searching.adjacency(E, labels)
    with pytest.raises(ValueError, match="index form"):
        searching.prominent_peaks(E, value, 1.0)
    for bad in (-1.0, float("nan"), 1e6):
        with pytest.raises(ValueError):
            index.adjacency(bad, labels)
        with pytest.raises(ValueError):
            index.prominent_peaks(bad, value, 1.0)
    for bad in (np.zeros(m), labels[:-1], np.zeros((m, 1), dtype=np.int64), torch.zeros(m)):
        with pytest.raises(ValueError):
            index.adjacency(E, bad)
    for bad in (value[:-1], np.zeros((m, 1)), labels):
        with pytest.raises(ValueError):
            index.adjacency(E, labels, voxel_value=bad)
        with pytest.raises(ValueError):
            index.prominent_peaks(E, bad, 1.0)
    for bad in (labels[:-1], np.zeros(m)):
        with pytest.raises(ValueError):
            index.adjacency(E, labels, voxel_class=bad)
    # a label that does not fit the key
    for where in (0, m // 2, m - 1):
        big = labels.copy()
        big[where] = 1 << 31
        with pytest.raises(ValueError, match="2\\^31"):
            index.adjacency(E, big)
    big = np.arange(m) + (1 << 40)
    with pytest.raises(ValueError, match="2\\^31"):
        index.adjacency(E, big, value)
    for bad in (-1.0, -1e-300, float("nan"), -INF, None, "high"):
        with pytest.raises(ValueError, match="min_prominence"):
            index.prominent_peaks(E, value, bad)
        with pytest.raises(ValueError, match="min_prominence"):
            multiscale.prominent_segments(uniform.cloud, E, E, bad)
    with pytest.raises(ValueError, match="link must be"):
        index.prominent_peaks(E, value, 1.0, link="up")
    for bad in (1.5, None, True):
        with pytest.raises(ValueError):
            index.prominent_peaks(E, value, 1.0, min_size=bad)
    with pytest.raises(ValueError):
        multiscale.prominent_segments(uniform.cloud, E, -1.0, 1.0)
    with pytest.raises(ValueError):
        multiscale.prominent_segments(uniform.cloud, E, E, 1.0, min_points=2.5)
    with pytest.raises(ValueError):
        multiscale.prominent_segments(uniform.cloud, E, E, 1.0, point_value=np.zeros(len(uniform.cloud) - 1))
    index._rt.check_async(wait=True)
    # the handle is as usable as before
    uniform.check(E, scattered_labels(m), value)
