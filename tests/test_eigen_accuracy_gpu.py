"""
every branch of the eigen-solver, on every path that consumes it, against exact arithmetic (run with `-m gpu`).

inputs are exact (tests/eigen_cases.py: lattice islands with dyadic coordinates), the reference is the exact
integer scatter matrix with eigenvalues from mpmath, and each neighborhood carries the label of the branch
the solver takes for it (triple / double / near-double / band above the switch / generic, top or bottom,
rank 1).  bound on both eigen columns: 1e-13 absolute, per class - what the project already asserts on one
uniform cloud (test_far_from_the_origin_...) and what the solver's comment claims for its closed form down
to the switch.  every test prints one line per (path, class): count and worst error; LAPACK's figures on the
same matrices are printed by tests/test_eigen_reference_cpu.py (all below 1e-15).
"""

from fractions import Fraction

import numpy as np
import pytest
import torch

import eigen_cases as ec
from nimrud_amd.minimal import classification, features, multiscale

pytestmark = pytest.mark.gpu

BOUND = 1e-13


def _gpu(points):
    return torch.from_numpy(np.array(points, dtype=np.float64, order="C")).cuda()


# ---- the fused LUT kernels and the generic kernel ----------------------------------------------------------------

@pytest.mark.parametrize("name,rho", ec.LEGS, ids=[leg[0] for leg in ec.LEGS])
def test_lattice_kernels_per_branch(name, rho):
    """one single-scale call per kernel leg (W = 3, 5, 7, 7 mirrored, 9, 11 and the generic kernel at W = 13)
    on that leg's island cloud: population exact, eigen columns within 1e-13 per class, structural values to
    1e-15, centroid column within a few ulp of the exact distance."""
    cloud, n, U, A, feats, cent, refs = ec.leg_reference(rho)
    dev = _gpu(cloud.points)
    got = multiscale.process_gpu(dev, dev, [ec.E], [rho * ec.E]).cpu().numpy()
    report = ec.merged({k: v[0] for k, v in ec.check_eigen_rows(name, got, n, feats, refs, BOUND).items()})
    for cls in ("triple", "double_top", "double_bottom", "generic_top", "rank1"):
        assert report.get(cls, 0) >= 3
    assert name in ec.NO_GENERIC_BOTTOM_LEGS or report.get("generic_bottom", 0) >= 3
    assert name in ec.NO_BAND_LEGS or report["band"] >= 3
    assert name in ec.NO_NEAR_LEGS or report["near"] >= 3
    ec.check_centroid_rows(name, got, cent, cloud.points)


def _ladder_cloud():
    """islands for the edges e, 2e, 4e side by side: coordinates in units of e, the islands of edge m*e on
    multiples of m, every sub-cloud's minimum on a multiple of 4 (so each is cell-centred on its own scale)"""
    parts, shift = [], 0
    for m in (1, 2, 4):
        pats = [p for p in ec.patterns_for_leg(3.0)
                if p[0].startswith(("ball3", "ball4.5", "disc3/", "line", "pair", "plane111", "blob1",
                                    "slab2.5/", "slab3/", "rod2.5/", "rod3/", "ball-1", "disc-2"))]
        sub = ec.IslandCloud(pats, gap_cells=9, origin=(0, 0, 0)).cells * m
        sub[:, 0] += shift
        shift = int(sub[:, 0].max()) // 4 * 4 + 64
        parts.append(sub)
    return np.concatenate(parts, axis=0)


def test_three_scale_ladder_of_the_mirrored_kernel():
    """edges e, 2e, 4e with r/e = 3 on every scale, three ways.  (a) ONE ladder call: below
    NM_SPLIT_SCALES_BELOW slots that is one launch of the <7,3> kernel with a workgroup per (scale, batch),
    LOOP = false.  (b) per_scale=True: one launch per scale.  (c) the SCALE LOOP, LOOP = true, where a wave
    walks the three scales and keeps its queries: at this size only a call with a forest attached takes it
    (launch_scale_kernel: the forest epilogue always rides the loop form), so a two-leaf forest on the first
    scale's l0 is attached through classification.classify_cloud; its labels are checked as well.  all three
    are bit-identical, and the loop form's output is the one held to 1e-13 per class on every scale.  queries
    of the other sub-clouds are off-centre at a scale, and the coarse cells of fine islands are neighborhoods
    too: the reference is the general one (eigen_cases.lattice_neighborhoods).

    last, over all three scales: exactly planar neighborhoods have l0 + l1 within 1e-15 of 1.  (with the closed
    form taken down to t = 1e-6 on both sides this failed: three rows of five cells, A = [[50,25,0],[25,14,0],
    [0,0,0]], spectrum (0.98134, 0.01866, 0), r > 0, t = 2.8e-4, came out at 1 + 1.55e-15, where
    numpy.linalg.eigvalsh gives 1 + 0; for r >= 0 the solver now deflates below t = 1e-2, measured 2.2e-16.)"""
    k = _ladder_cloud()
    assert len(k) <= 20000
    pts = k.astype(np.float64) * ec.E
    dev = _gpu(pts)
    edges = [ec.E, 2 * ec.E, 4 * ec.E]
    radii = [3 * e for e in edges]
    got = multiscale.process_gpu(dev, dev, edges, radii)
    per = multiscale.process_gpu(dev, dev, edges, radii, per_scale=True)
    assert torch.equal(got, per)
    # one tree: l0 of the first scale (feature 2) <= 0.5 -> class 0, else class 1
    forest = classification.ForestModel(left=[1, -1, -1], right=[2, -1, -1], feature=[2, 0, 0],
                                        threshold=[0.5, 0.0, 0.0], value=[[0.5, 0.5], [1.0, 0.0], [0.0, 1.0]],
                                        roots=[0], classes=[0, 1], n_features=12)
    label, loop = classification.classify_cloud(dev, edges, radii, forest)
    assert torch.equal(loop, got)
    got = loop.cpu().numpy()
    assert np.array_equal(label.cpu().numpy(), (got[:, 2].astype(np.float32) > np.float32(0.5)).astype(np.int32))
    assert 0 < int(label.sum()) < len(label)
    planar = []
    for s, m in enumerate((1, 2, 4)):
        n, U, A = ec.lattice_neighborhoods(k, m, 3.0)
        feats, cent, refs = ec.reference_rows(n, U, A)
        report = ec.check_eigen_rows("ladder scale %d" % s, got[:, 4 * s:4 * s + 4], n, feats, refs, BOUND,
                                     planar_sum=planar)
        counts = ec.merged({key: v[0] for key, v in report.items()})
        for cls in ("triple", "double_top", "double_bottom", "generic_top", "generic_bottom", "band", "near"):
            assert counts.get(cls, 0) >= 1, (s, cls)
        ec.check_centroid_rows("ladder scale %d" % s, got[:, 4 * s:4 * s + 4], cent, pts)
    print("%-28s %-15s n %5d  worst |l0 + l1 - 1| %.3g" % ("ladder", "planar", len(planar), max(planar)[0]))
    assert max(planar)[0] <= 1e-15, sorted(planar, reverse=True)[:4]


# ---- covariance output ----------------------------------------------------------------------------------------

def _blob_cloud(rho):
    pats = []
    for salt in (1, 2, 3):
        cells = ec.blob(min(rho + 1.0, 4.0), salt)
        for fx, fy, fz in ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, 1), (-1, 1, -1),
                           (1, -1, -1), (-1, -1, -1)):
            pats.append(("blob%d/%d%d%d" % (salt, fx, fy, fz), tuple((x * fx, y * fy, z * fz)
                                                                      for x, y, z in cells)))
    return ec.IslandCloud(pats, gap_cells=int(np.ceil(2 * rho)) + 3)


@pytest.mark.parametrize("name,rho", [("W7_mirrored", 3.0), ("W5", 2.0), ("W13_generic", 5.5)])
def test_covariance_output_is_exact_to_rounding(name, rho):
    """process_gpu_covariance on asymmetric blobs and their mirror images in every axis.  each of the six
    entries within 4 ulp of the exact Fraction e^2 A / (n (n-1)): the integer moments are exact below 2^53,
    e*e and n*(n-1) are exact, one division and two products round.  exact zeros come out as zeros; the signs
    of the off-diagonals follow from the bound, and all eight sign patterns occur."""
    cloud = _blob_cloud(rho)
    n, U, A = ec.island_neighborhoods(cloud, rho)
    dev = _gpu(cloud.points)
    feats, cov = multiscale.process_gpu_covariance(dev, dev, [ec.E], [rho * ec.E])
    cov = cov.cpu().numpy()
    assert np.array_equal(feats.cpu().numpy()[:, 0], n)
    worst, zeros, signs = 0.0, 0, set()
    for i in range(len(n)):
        if n[i] < 2:
            assert not cov[i].any()
            continue
        want = ec.exact_covariance(n[i], A[i])
        for c in range(6):
            if want[c] == 0:
                zeros += 1
                assert cov[i, c] == 0.0, (name, i, c, cov[i, c])
                continue
            ulp = Fraction(float(np.spacing(abs(float(want[c])))))
            off = abs(Fraction(float(cov[i, c])) - want[c]) / ulp
            worst = max(worst, float(off))
            assert off <= 4, (name, i, c, float(off))
        if all(want[c] != 0 for c in (1, 2, 4)):
            signs.add(tuple(want[c] > 0 for c in (1, 2, 4)))
    print("%-28s %-15s n %5d  worst %.3g ulp, %d exact zeros, %d off-diagonal sign patterns" % (
        "covariance " + name, "all", len(n), worst, zeros, len(signs)))
    assert len(signs) == 8


# ---- normal output ----------------------------------------------------------------------------------------

PLANE_NORMALS = ((0, 0, 1), (1, 1, 0), (1, 1, 1), (1, 2, 0))


@pytest.mark.parametrize("name,rho", [("W7_mirrored", 3.0), ("W7", 2.5)])
def test_normal_output_against_the_exact_eigenvector(name, rho):
    """process_gpu_normals on planar islands and blobs, rows with at least three cells and a relative gap
    (l1 - l2) / tr >= 0.05: within 1e-12 of the mpmath eigenvector, sign rule (last non-zero component
    positive) included - an eigenvector error of a few eps divided by the gap is below 1e-13.  on exactly
    planar neighborhoods of the plane islands the normal is the plane's rational one to 1e-14."""
    pats = [("plane%d%d%d" % nrm, ec.plane(nrm, 4.0)) for nrm in PLANE_NORMALS]
    pats += [("blob%d" % salt, ec.blob(4.0, salt)) for salt in (1, 2, 3)]
    cloud = ec.IslandCloud(pats, gap_cells=int(np.ceil(2 * rho)) + 3)
    n, U, A = ec.island_neighborhoods(cloud, rho)
    dev = _gpu(cloud.points)
    feats, normals = multiscale.process_gpu_normals(dev, dev, [ec.E], [rho * ec.E])
    normals = normals.cpu().numpy()
    assert np.array_equal(feats.cpu().numpy()[:, 0], n)
    worst = worst_plane = 0.0
    checked = planes = 0
    for i in range(len(n)):
        if n[i] < 3:
            assert not normals[i].any()
            continue
        key = tuple(int(v) for v in A[i])
        ref = ec.exact_eigen(key)
        if ref.gap < 0.05:
            continue
        want = np.array(ec.exact_normal(key))
        checked += 1
        worst = max(worst, np.abs(normals[i] - want).max())
        if ref.planar and cloud.island[i] < len(PLANE_NORMALS):
            nrm = np.array(PLANE_NORMALS[cloud.island[i]], dtype=np.float64)
            planes += 1
            worst_plane = max(worst_plane, np.abs(normals[i] - nrm / np.sqrt((nrm * nrm).sum())).max())
    print("%-28s %-15s n %5d  worst %.3g;  exact planes n %d worst %.3g" % (
        "normals " + name, "gap>=0.05", checked, worst, planes, worst_plane))
    assert checked >= 200 and planes >= 50
    assert worst <= 1e-12
    assert worst_plane <= 1e-14


# ---- k-nearest-voxel fallback -----------------------------------------------------------------------------

KNN_ISLANDS_8 = (
    ("line_x", tuple((t, 0, 0) for t in range(8))),
    ("line_diag", tuple((t, t, 0) for t in range(8))),
    ("line_space", tuple((t, -t, t) for t in range(-2, 6))),
    ("planar_grid", ((0, 0, 0), (3, 0, 0), (6, 0, 0), (0, 3, 0), (3, 3, 0), (6, 3, 0), (0, 6, 0), (3, 6, 0))),
    ("planar_tilted", ((0, 0, 0), (3, 0, 3), (6, 0, 6), (0, 3, 0), (3, 3, 3), (5, 3, 5), (0, 6, 0), (2, 6, 2))),
    ("planar_ring", ((3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0), (2, 2, 0), (-2, 2, 0), (2, -2, 0),
                     (-2, -2, 0))),
    ("blob_a", ((0, 0, 0), (3, 1, 0), (1, 3, 2), (-2, 2, 3), (-3, -1, 1), (0, -3, -2), (2, -2, 3), (1, 1, -3))),
    ("blob_b", ((0, 0, 0), (4, 0, 1), (0, 3, -1), (-3, 0, 2), (1, -3, 3), (3, 3, 3), (-2, -2, -2), (2, -1, -3))),
    ("blob_c", ((0, 0, 0), (0, 0, 3), (0, 3, 0), (3, 0, 0), (3, 3, 1), (1, 3, 3), (3, 1, 3), (5, 5, 5))),
)
KNN_ISLANDS_2 = (("pair_a", ((0, 0, 0), (3, 1, 0))), ("pair_b", ((0, 0, 0), (0, 0, 4))),
                 ("pair_c", ((0, 0, 0), (2, 2, 2))), ("pair_d", ((0, 0, 0), (-1, 4, 2))))


@pytest.mark.parametrize("k,islands", [(8, KNN_ISLANDS_8), (2, KNN_ISLANDS_2)], ids=["k8", "k2"])
def test_knn_fallback_per_branch(k, islands):
    """knn_min = k on islands of exactly k cells with r/e = 2 and radius factor 7: every cell of an island is
    within 14 cells of every other and fewer than k are within 2, so (oracle.one_scale_knn: the k nearest
    voxels within factor * r) the fallback's set is the whole island, whatever the ties - no pattern's set is
    ambiguous, none was dropped.  islands lie more than 2 * 7 * 2 + 2 cells apart.  column 0 keeps the radius
    population; the eigen columns meet 1e-13 against the island's exact spectrum."""
    rho, factor = 2.0, 7.0
    cloud = ec.IslandCloud(list(islands), gap_cells=int(2 * factor * rho) + 3)
    n_radius, _, _ = ec.island_neighborhoods(cloud, rho)
    whole = lambda c: np.ones((len(c), len(c)), dtype=bool)
    n, U, A = ec.island_neighborhoods(cloud, rho, rows_of=whole)
    for num in range(len(islands)):
        c = cloud.cells[cloud.island == num]
        assert len(c) == k and len(np.unique(c, axis=0)) == k
        d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(2)
        assert d2.max() <= (factor * rho) ** 2 and (n_radius[cloud.island == num] < k).all()
    feats, cent, refs = ec.reference_rows(n, U, A)
    dev = _gpu(cloud.points)
    got = multiscale.process_gpu(dev, dev, [ec.E], [rho * ec.E], knn_min=k,
                                 knn_radius_factor=factor).cpu().numpy()
    assert np.array_equal(got[:, 0], n_radius)
    got[:, 0] = n
    report = ec.check_eigen_rows("knn k=%d" % k, got, n, feats, refs, BOUND)
    # the classes the islands are there for: lines and pairs (double_top, rank 1), the symmetric ring
    # (double_bottom), the other planar sets (generic_bottom) and the blobs (generic_top)
    for cls in ("double_top", "rank1") + (("double_bottom", "generic_bottom", "generic_top") if k == 8 else ()):
        assert report.get(cls, (0, 0.0))[0] >= len(cloud.cells[cloud.island == 0]), cls
    ec.check_centroid_rows("knn k=%d" % k, got, cent, cloud.points)


# ---- explicit neighborhoods (nm_eig3 on floating-point moments) ---------------------------------------------------

def _perturbed_sets():
    """square-symmetric dyadic point sets with one point moved by 2^-k, k = 6 .. 20: the double pair of the
    symmetric set splits by about 2^-k / 10 of the trace.  flat ones (pair on top of a small third
    eigenvalue: r < 0) and tall ones (pair below a large one: r > 0)."""
    sets = []
    for height in (0.5, 4.0):
        base = [(1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0),
                (0, 0, height), (0, 0, -height)]
        for k in range(6, 21):
            pts = np.array(base, dtype=np.float64)
            pts[4, 0] += 2.0 ** -k
            sets.append(pts + np.array([3.0, -2.0, 1.0]))
    return sets


def test_explicit_neighborhoods_per_branch():
    """features.neighborhood_features (k_neighborhood_features: mean, deviations and moments in fp64, then
    nm_eig3) on the catalogue's cell sets as point lists (coordinates up to 16 in magnitude) and on
    non-lattice dyadic sets with near-double spectra.  reference: exact from the Fractions of the inputs.
    bound 1e-13: with max|x|^2 / variance of order 1 and n <= 600 the moment matrix carries a relative error
    of a few n*eps = 1e-13 at the very worst, typically 1e-15.  features.pca, the scalar form, on a few."""
    sets = [np.asarray(cells, dtype=np.float64) * ec.E + np.array([11.0, -9.5, 4.25])
            for _, cells in ec.patterns_for_leg(5.0) if len(cells) <= 600]
    sets += _perturbed_sets()
    assert max(len(s) for s in sets) <= 600 and max(np.abs(s).max() for s in sets) <= 16.0
    offsets = np.concatenate(([0], np.cumsum([len(s) for s in sets])))
    points = np.concatenate(sets, axis=0)
    query = np.array([s[0] for s in sets])
    got = features.neighborhood_features(points, offsets, query)
    n = np.array([len(s) for s in sets], dtype=np.int64)
    refs = [ec.exact_eigen(ec.scatter_of_points(s)[1]) for s in sets]
    feats = np.array([r.f[:2] for r in refs])
    report = ec.check_eigen_rows("explicit neighborhoods", got, n, feats, refs, BOUND)
    for cls in ("triple", "double_top", "double_bottom", "near_top", "near_bottom", "band_top", "band_bottom",
                "generic_top", "generic_bottom", "rank1"):
        assert cls in report, cls
    for i in (0, len(sets) // 2, len(sets) - 1):
        assert np.abs(features.pca(sets[i]) - feats[i]).max() <= BOUND
