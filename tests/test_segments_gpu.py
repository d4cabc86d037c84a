"""
GPU tests of multiscale.segment_table / cluster_features / NeighborIndex.component_table (nm_segments.hip) against the
numpy reference of tests/segments_reference.py, which test_segments_cpu.py pins on segments computed by hand.

the bounds are derived, not measured (segments_reference.tolerances): with u = 2^-53, r the segment's rows and D its
box diagonal - n and the box array_equal; covariance 8 (r + 4) u D^2; centroid 4 (r + 4) u D + 2 u max|p|; eigenvalues
3 tol_cov + 1e-13 trace; vectors sin(angle) <= 2 tol_eig / gap, checked only where the reference's gap is at least
0.05 lambda_1 - which is asserted, not skipped.  every comparison prints its worst figure before it asserts.
"""


import numpy as np
import pytest
import torch

import components_reference
import segments_reference as ref
from nimrud_amd import _ffi
from nimrud_amd import device as _device
from nimrud_amd.minimal import multiscale

pytestmark = pytest.mark.gpu

K = _ffi.NM_SEGMENT_CHUNK
OFFSET = np.array([4.0e5, 5.1e6, 300.0])              # the shift of golden/g3_offset
LENGTHS = [0, 1, 2, 3, K - 1, K, K + 1, 2 * K + 1, 64 * K + 3]


def check_table(got, points, labels, weights=None, vectors=(), what="", repeated=False):
    """hold every row of `got` to the reference within the derived bounds; `vectors`: per segment the names
    ("normal", "axis") to check, or one tuple for all segments.  repeated: `got` was computed from the cloud with
    every row repeated weight times - the r of its bounds is that number of rows"""
    points = np.asarray(points)[:, :3]
    want = ref.segment_table(points, labels, weights, n_segments=len(got))
    assert got.shape == want.shape and got.dtype == np.float64
    worst = np.zeros(4)
    for s in range(len(want)):
        mine = labels == s
        if weights is not None:
            mine = mine & (np.asarray(weights) > 0)
        rows = int(mine.sum())
        g, w = got[s], want[s]
        if repeated:
            rows = int(w[0])
        assert g[0] == w[0] and np.array_equal(g[4:10], w[4:10]), (what, s, g[:10], w[:10])
        if rows == 0:
            assert not g.any(), (what, s)
            continue
        tol_cov, tol_centroid, tol_eig = ref.tolerances(w, rows, np.abs(points[mine]).max())
        err = [np.abs(g[10:16] - w[10:16]).max(), np.abs(g[1:4] - w[1:4]).max(), np.abs(g[16:19] - w[16:19]).max()]
        for k, tol in enumerate((tol_cov, tol_centroid, tol_eig)):
            worst[k] = max(worst[k], err[k] / tol if tol > 0 else (0.0 if err[k] == 0 else np.inf))
        assert err[0] <= tol_cov, (what, s, "covariance", err[0], tol_cov)
        assert err[1] <= tol_centroid, (what, s, "centroid", err[1], tol_centroid)
        assert err[2] <= tol_eig, (what, s, "eigenvalues", err[2], tol_eig)
        assert np.all(np.diff(g[16:19]) <= 0), (what, s, "eigenvalues descend")
        names = vectors[s] if (len(vectors) and isinstance(vectors[0], tuple)) else vectors
        for name in names:
            which, at = (2, slice(19, 22)) if name == "normal" else (0, slice(22, 25))
            gap = ref.gap_of(w, which)
            assert gap >= 0.05 * w[16], (what, s, name, "the shape does not separate this eigenvalue", w[16:19])
            sine = ref.sin_angle(g[at], w[at])
            worst[3] = max(worst[3], sine / (2.0 * tol_eig / gap))
            assert abs(np.linalg.norm(g[at]) - 1.0) <= 1e-14, (what, s, name)
            assert sine <= 2.0 * tol_eig / gap, (what, s, name, sine, 2.0 * tol_eig / gap)
            assert np.dot(g[at], w[at]) > 0, (what, s, name, "sign rule", g[at], w[at])
    print("%s: worst error / bound: covariance %.3g, centroid %.3g, eigenvalues %.3g, vectors %.3g"
          % (what, worst[0], worst[1], worst[2], worst[3]))
    return want


class Case1(object):
    """segments of LENGTHS rows of random points in a unit box: contiguous, and interleaved by a seeded permutation
    that keeps every segment's ascending row order (made once, never changed)"""

    def __init__(self):
        rng = np.random.default_rng(11)
        self.labels = np.repeat(np.arange(len(LENGTHS)), LENGTHS)
        self.points = rng.random((len(self.labels), 3))
        # interleaved: draw the label sequence at random, hand each segment its rows in their old order
        self.mixed_labels = rng.permutation(self.labels)
        source = np.empty(len(self.labels), dtype=np.int64)
        for s in range(len(LENGTHS)):
            source[self.mixed_labels == s] = np.nonzero(self.labels == s)[0]
        self.mixed_points = self.points[source]
        for a in (self.labels, self.points, self.mixed_labels, self.mixed_points):
            a.setflags(write=False)
        self.table = multiscale.segment_table(self.points, self.labels, n_segments=len(LENGTHS))
        self.table.setflags(write=False)


@pytest.fixture(scope="module")
def case1():
    return Case1()


# ---- 1. every path length in one call -----------------------------------------------------------------------------------

def test_lengths_contiguous_and_interleaved(case1):
    assert isinstance(case1.table, np.ndarray) and case1.table.shape == (len(LENGTHS), 25)
    check_table(case1.table, case1.points, case1.labels, what="contiguous")
    assert np.array_equal(case1.table[:, 0], LENGTHS)
    mixed = multiscale.segment_table(case1.mixed_points, case1.mixed_labels, n_segments=len(LENGTHS))
    assert np.array_equal(mixed.view(np.uint64), case1.table.view(np.uint64))


# ---- 2. a segment is a function of its own rows -----------------------------------------------------------------------------

def test_a_segment_is_a_function_of_its_own_rows(case1):
    rng = np.random.default_rng(12)
    n, extra, shift = len(case1.labels), 5000, 40
    at = np.sort(rng.choice(n + extra, size=extra, replace=False))          # where the new rows go
    old = np.setdiff1d(np.arange(n + extra), at)
    points = np.empty((n + extra, 3))
    labels = np.empty(n + extra, dtype=np.int64)
    points[old], labels[old] = case1.mixed_points, case1.mixed_labels + shift
    points[at] = rng.random((extra, 3)) * 3.0
    labels[at] = rng.integers(0, shift, extra)
    c = shift + len(LENGTHS)
    table = multiscale.segment_table(points, labels, n_segments=c)
    assert np.array_equal(table[shift:].view(np.uint64), case1.table.view(np.uint64))
    again = multiscale.segment_table(points, labels, n_segments=c)
    assert np.array_equal(again.view(np.uint64), table.view(np.uint64))
    check_table(table[:shift], points, labels, what="the rows in between")


# ---- 3. rows of no segment, empty calls, strides ----------------------------------------------------------------------------

def test_rows_of_no_segment_and_empty_calls(case1):
    rng = np.random.default_rng(13)
    c = len(LENGTHS)
    points = np.vstack([case1.points, rng.random((300, 3)) * 9.0])
    labels = np.concatenate([case1.labels, np.where(rng.random(300) < 0.5, -1, c + rng.integers(0, 5, 300))])
    table = multiscale.segment_table(points, labels, n_segments=c)
    assert np.array_equal(table.view(np.uint64), case1.table.view(np.uint64))
    assert multiscale.segment_table(points, labels, n_segments=0).shape == (0, 25)
    assert multiscale.segment_table(points[:0], labels[:0]).shape == (0, 25)
    empty = multiscale.segment_table(points[:0], labels[:0], n_segments=3)
    assert empty.shape == (3, 25) and not empty.any()
    assert multiscale.segment_table(points, np.full(len(points), -1)).shape == (0, 25)


def test_table_stride_and_cloud_stride(case1):
    rt = _device.get_runtime()
    c, n = len(LENGTHS), len(case1.labels)
    wide = np.hstack([case1.points, np.random.default_rng(14).random((n, 2))])             # row stride 5
    assert np.array_equal(multiscale.segment_table(wide, case1.labels, n_segments=c).view(np.uint64),
                          case1.table.view(np.uint64))
    cloud = torch.from_numpy(wide).to(rt.device)
    labels = torch.from_numpy(case1.labels).to(rt.device)
    out = torch.full((c, 32), -7.0, dtype=torch.float64, device=rt.device)
    nbytes = rt.lib.nm_segment_table_workspace_bytes(n, c)
    tmp = torch.empty(nbytes, dtype=torch.uint8, device=rt.device)
    rc = rt.lib.nm_segment_table(rt.ctx, _device.ptr(cloud), n, 5, _device.ptr(labels), c, None, _device.ptr(out), 32,
                                 _device.ptr(tmp), nbytes, rt.stream())
    assert rc == _ffi.NM_OK
    out = out.cpu().numpy()
    assert np.array_equal(out[:, :25].view(np.uint64), case1.table.view(np.uint64))
    assert np.all(out[:, 25:] == -7.0)
    # the errors, before anything is queued
    spare = torch.zeros((c, 25), dtype=torch.float64, device=rt.device)
    args = (rt.ctx, _device.ptr(cloud), n, 5, _device.ptr(labels), c, None, _device.ptr(spare))
    assert rt.lib.nm_segment_table(*args, 24, _device.ptr(tmp), nbytes, rt.stream()) == _ffi.NM_ERR_INVALID
    assert rt.lib.nm_segment_table(*args, 25, _device.ptr(tmp), nbytes - 1, rt.stream()) == _ffi.NM_ERR_WORKSPACE
    assert rt.lib.nm_segment_table(*args, 25, _device.ptr(tmp), nbytes, rt.stream()) == _ffi.NM_OK
    assert np.array_equal(spare.cpu().numpy().view(np.uint64), case1.table.view(np.uint64))


# ---- 4. / 5. shapes, at the origin and at the offset -------------------------------------------------------------------------

def shapes(seed):
    """(points, labels, vectors): a tilted 3 cm x 2 cm plane patch of 1 000 points, a 2 m pole of 600 points with
    2 cm of jitter, a box of 2 000 points with extents 3 : 2 : 1"""
    rng = np.random.default_rng(seed)
    u, v = np.array([1.0, 0.2, 0.3]), np.array([-0.1, 1.0, 0.4])
    u /= np.linalg.norm(u)
    v -= v.dot(u) * u
    v /= np.linalg.norm(v)
    patch = np.outer(rng.random(1000) * 0.03, u) + np.outer(rng.random(1000) * 0.02, v)
    pole = np.column_stack([rng.normal(0, 0.02, 600), rng.normal(0, 0.02, 600), rng.random(600) * 2.0]) + [5.0, 3.0, 0]
    box = rng.random((2000, 3)) * [3.0, 2.0, 1.0] + [-8.0, 1.0, 2.0]
    points = np.vstack([patch, pole, box])
    labels = np.repeat([0, 1, 2], [1000, 600, 2000])
    order = rng.permutation(len(points))
    return points[order], labels[order], [("normal", "axis"), ("axis",), ("normal", "axis")]


def test_shapes_at_the_origin():
    points, labels, vectors = shapes(21)
    table = multiscale.segment_table(points, labels)
    want = check_table(table, points, labels, vectors=vectors, what="shapes at the origin")
    assert abs(want[1, 24]) > 0.999 and abs(table[1, 24]) > 0.999            # the pole stands


def test_shapes_at_the_offset():
    points, labels, vectors = shapes(22)
    points = points + OFFSET
    table = multiscale.segment_table(points, labels)
    check_table(table, points, labels, vectors=vectors, what="shapes at the offset")
    # the bound scales with the box, not with the coordinates: 8 * 1004 * u * (0.03^2 + 0.02^2) for the patch, where
    # raw second moments of y = 5.1e6 carry u * 1000 * 2.6e13 = 3e0
    assert ref.tolerances(ref.segment_row(points[labels == 0]), 1000, 5.1e6)[0] < 2e-15


# ---- 6. exact degenerates ---------------------------------------------------------------------------------------------------------

def test_exact_degenerates():
    line = np.arange(41)[:, None] * np.array([0.25, 0.5, 0.5]) + [1.0, 2.0, 3.0]
    same = np.tile([[0.1, 0.7, -0.3]], (50, 1))
    pair = np.array([[0.0, 1.0, 2.0], [0.5, 1.0, 4.0]])
    points = np.vstack([line, same, pair])
    labels = np.repeat([0, 1, 2], [41, 50, 2])
    table = multiscale.segment_table(points, labels)
    want = check_table(table, points, labels, vectors=[("axis",), (), ()], what="degenerates")
    tol_eig = ref.tolerances(want[0], 41, 30.0)[2]
    assert abs(table[0, 17]) <= tol_eig and abs(table[0, 18]) <= tol_eig
    assert table[1, 0] == 50 and np.array_equal(table[1, 1:4], same[0]) and not table[1, 10:].any()
    assert not table[2, 19:].any()
    trace = table[2, 10] + table[2, 13] + table[2, 15]
    tol_eig = ref.tolerances(want[2], 2, 4.0)[2]
    assert abs(table[2, 16] - trace) <= tol_eig and abs(table[2, 17]) <= tol_eig and abs(table[2, 18]) <= tol_eig


# ---- 7. weights ---------------------------------------------------------------------------------------------------------------------

def test_weights_are_frequencies():
    rng = np.random.default_rng(31)
    lengths = [3, 40, K + 5, 3 * K + 1, 7]
    labels = rng.permutation(np.repeat(np.arange(len(lengths)), lengths))
    points = rng.random((len(labels), 3)) * [4.0, 2.0, 1.0]
    weights = rng.integers(0, 6, len(labels))
    weights[labels == 4] = 0                                   # a segment with nothing in it
    assert (weights[labels != 4] == 0).any()
    table = multiscale.segment_table(points, labels, weights)
    check_table(table, points, labels, weights, what="weights")
    assert not table[4].any()
    assert np.array_equal(table[:, 0], np.bincount(labels, weights=weights, minlength=5))
    # the same cloud with its rows repeated, unweighted
    repeated = multiscale.segment_table(np.repeat(points, weights, axis=0), np.repeat(labels, weights), n_segments=5)
    check_table(repeated, points, labels, weights, what="rows repeated", repeated=True)
    assert np.array_equal(repeated[:, 0], table[:, 0]) and np.array_equal(repeated[:, 4:10], table[:, 4:10])
    big = multiscale.segment_table(points, labels, np.where(labels == 1, 2 ** 40, 0))
    assert big[1, 0] == float(2 ** 40 * 40) and not big[0].any()


# ---- 8. the interface ---------------------------------------------------------------------------------------------------------------

def test_interface(case1):
    rt = _device.get_runtime()
    c = len(LENGTHS)
    cloud = torch.from_numpy(case1.points).to(rt.device)
    labels = torch.from_numpy(case1.labels).to(rt.device)
    table = multiscale.segment_table(cloud, labels)
    assert isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.float64
    assert np.array_equal(table.cpu().numpy().view(np.uint64), case1.table.view(np.uint64))
    small = multiscale.segment_table(case1.points, case1.labels.astype(np.int32), n_segments=c)
    assert isinstance(small, np.ndarray) and np.array_equal(small.view(np.uint64), case1.table.view(np.uint64))
    assert np.array_equal(multiscale.segment_table(cloud, labels.to(torch.int32)).cpu().numpy(), case1.table)
    assert sorted(multiscale.SEGMENT_COLUMNS) == sorted(["n", "centroid", "min", "max", "covariance", "eigenvalues",
                                                         "normal", "axis"])
    covered = np.zeros(25, dtype=int)
    for piece in multiscale.SEGMENT_COLUMNS.values():
        covered[piece] += 1
    assert np.all(covered == 1)
    assert np.array_equal(case1.table[:, multiscale.SEGMENT_COLUMNS["n"]][:, 0], LENGTHS)
    with pytest.raises(ValueError):
        multiscale.segment_table(case1.points, case1.labels.astype(np.float64))
    with pytest.raises(ValueError):
        multiscale.segment_table(case1.points, case1.labels[:-1])
    with pytest.raises(ValueError):
        multiscale.segment_table(case1.points, case1.labels, weights=np.ones(len(case1.labels)))
    with pytest.raises(ValueError):
        multiscale.segment_table(case1.points[:, :2], case1.labels)


# ---- 9. cluster_features ----------------------------------------------------------------------------------------------------------

def test_cluster_features_on_the_random_lattice():
    e = components_reference.EDGE
    cloud = components_reference.cells_cloud(components_reference.random_lattice_cells(), seed=41)
    point_labels, sizes = multiscale.cluster_cloud(cloud, e, e, min_points=2)
    got = multiscale.cluster_features(cloud, e, e, min_points=2)
    assert all(isinstance(a, np.ndarray) for a in got) and got[2].shape == (len(sizes), 25)
    assert np.array_equal(got[0], point_labels) and np.array_equal(got[1], sizes)
    assert len(sizes) > 100 and (point_labels < 0).any()
    assert np.array_equal(got[2][:, 0], sizes)
    table = multiscale.segment_table(cloud, point_labels, n_segments=len(sizes))
    assert np.array_equal(got[2].view(np.uint64), table.view(np.uint64))
    check_table(table, cloud, point_labels, what="clusters")
    index = multiscale.NeighborIndex(cloud, e, method="index")
    labels, voxel_sizes = index.components(e, voxel_weight=index.point_counts(), min_size=2)
    assert np.array_equal(voxel_sizes, sizes)
    by_voxel = index.component_table(labels, index.point_counts())
    assert by_voxel.shape == (len(sizes), 25) and np.array_equal(by_voxel[:, 0], sizes)
    check_table(by_voxel, index.voxels(), labels, index.point_counts(), what="components over voxels")
    tensors = multiscale.cluster_features(torch.from_numpy(cloud).cuda(), e, e, min_points=2)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors)
    assert np.array_equal(tensors[2].cpu().numpy().view(np.uint64), table.view(np.uint64))
