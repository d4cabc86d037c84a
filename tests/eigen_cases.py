"""
case catalogue and exact reference for the 3x3 eigen-solver (nm_eig3_fast / nm_eig3 in nm_features.hip).

plain helper module: no GPU code, no test.  tests/test_eigen_reference_cpu.py pins it against the oracle and
checks what it covers, tests/test_eigen_accuracy_gpu.py holds the kernels to it.

the inputs are exact.  a pattern is a set of integer cells; one search point sits at the centre of each cell
of a lattice with edge E = 0.25, so every coordinate is k*E, a dyadic number, and because the lattice's
minimum corner is lo - E/2 (oracle.Lattice) every point IS its cell's centre.  squared distances between
centres are integers times E*E: the radius test has no rounding either.  patterns are tiled as islands, far
enough apart that no neighborhood spans two of them; every point is a query, so an island yields one
neighborhood per cell (the island cut by a ball around that cell).

the reference is exact too: n, S1, S2 of the integer cells as Python ints, A = n*S2 - S1*S1^T (n*(n-1)/E^2
times the ddof=1 covariance), its eigenvalues in mpmath at 80 digits (closed form of the cubic; the
discriminant is tested for zero in integers first), normalised by the exact trace.

the branch classifier works on the same integers.  with M = 3A - tr(A)*I, P2 = sum of M's squared entries
and D = det M, the solver's r satisfies r^2 = 54 D^2 / P2^3 (a rational) and sign r = sign D; its separated
root is x = 2 cos(acos|r| / 3) and its switch variable t = (2-x)(2+x)/4 = sin^2(acos|r| / 3).
"""

import functools
import itertools
from fractions import Fraction

import mpmath
import numpy as np

E = 0.25
MP_DIGITS = 80

# the kernel legs: name, r/e.  W = 2*floor(r/e + 1/2) + 1 candidates per axis
LEGS = (("W3", 1.0), ("W5", 2.0), ("W7", 2.5), ("W7_mirrored", 3.0), ("W9", 4.0), ("W11", 5.0),
        ("W13_generic", 5.5))
BALL_RADII = (1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0)

NEAR_T = 5e-7              # 0 < t < NEAR_T: deflation branch, safely below the kernel's switch at 1e-6
BAND_LO, BAND_HI = 1e-6, 1e-4     # closed form just above the switch


# ---- pattern builders -------------------------------------------------------------------------------------

def _cube(m):
    rng = range(-m, m + 1)
    return itertools.product(rng, rng, rng)


def ball(rho):
    """cells within rho of the origin (inclusive, tested in integers: 4 d^2 <= (2 rho)^2)"""
    lim = int(round(4 * rho * rho))
    m = int(rho)
    return tuple(c for c in _cube(m) if 4 * (c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) <= lim)


def slab(rho, half, axis=2):
    """the ball's cells with |c[axis]| <= half: half = 0 is a disc"""
    return tuple(c for c in ball(rho) if abs(c[axis]) <= half)


def rod(rho, width, axis=0):
    """the ball's cells within `width` of the axis: a prolate set whose two small eigenvalues coincide"""
    lim = int(round(4 * width * width))
    return tuple(c for c in ball(rho) if 4 * sum(c[a] * c[a] for a in range(3) if a != axis) <= lim)


def plane(normal, rho):
    """the ball's cells on the plane through the origin with that integer normal"""
    return tuple(c for c in ball(rho) if c[0] * normal[0] + c[1] * normal[1] + c[2] * normal[2] == 0)


def line(direction, half):
    return tuple((t * direction[0], t * direction[1], t * direction[2]) for t in range(-half, half + 1))


def minus(cells, removed):
    gone = set(removed)
    assert gone <= set(cells)
    return tuple(c for c in cells if c not in gone)


def blob(rho, salt):
    """an asymmetric subset of the ball: each octant keeps its cells at a density of its own (3 to 10 in
    11), chosen by a fixed integer hash - no two octants alike, all three off-diagonal moments non-zero"""
    keep = []
    for (x, y, z) in ball(rho):
        octant = (x > 0) + 2 * (y > 0) + 4 * (z > 0)
        h = (x * 73 + y * 179 + z * 283 + x * y * 31 + y * z * 17 + x * z * 7 + salt * 101) % 11
        if (x, y, z) == (0, 0, 0) or h < 3 + octant:
            keep.append((x, y, z))
    return tuple(keep)


# the near-double (0 < t < 5e-7) and band (1e-6 <= t < 1e-4) patterns: found by search_near_double() below
# and frozen here as (base, rho, half-height or width, removed cells, t, side); every entry was confirmed in
# exact arithmetic, and the CPU test recomputes t and the side.  the search does not run at test time.
# bases: discs and slabs |z| <= 1 of the balls (oblate: the pair is the two large eigenvalues, r < 0,
# "bottom") and rods of width 1 and 1.5 around the x axis (prolate: the pair is the two small ones, r > 0,
# "top"), with up to three cells other than the centre removed.  the whole pattern is one neighborhood for
# the query at its centre cell on every leg with r/e >= rho.
# what the search did NOT find: nothing with 0 < t < 1e-4 inside rho <= 1.5 (slabs and rods of the balls 1
# and 1.5, up to three cells removed), and nothing with 0 < t < 1e-6 inside rho = 2 (28 + 12 + 20 band
# patterns there, no near one).  so leg W3 has neither class and leg W5 no near_*: the coverage condition
# exempts them by name (NO_BAND_LEGS, NO_NEAR_LEGS).
FROZEN = (
    ("slab", 2.5, 1, ((-1, -1, -1), (-1, 1, -1), (0, 0, 1)), 2.39e-10, "bottom"),
    ("slab", 2.5, 1, ((-2, 0, 1), (0, 0, -1), (0, 2, 1)), 9.8e-09, "bottom"),
    ("slab", 2.5, 1, ((-2, 1, 1), (-1, -2, 1), (0, 0, 1)), 1.15e-07, "bottom"),
    ("slab", 2.5, 1, ((-1, 0, 0), (0, 0, 1), (0, 1, 1)), 2.7e-07, "bottom"),
    ("slab", 3.0, 1, ((-1, 0, -1), (0, -1, -1)), 3.64e-09, "bottom"),
    ("slab", 3.0, 1, ((-1, -2, -1), (2, -1, -1)), 8.32e-08, "bottom"),
    ("slab", 4.0, 0, ((-1, 0, 0), (0, -1, 0)), 3.72e-08, "bottom"),
    ("slab", 4.0, 0, ((-1, -1, 0), (-1, 1, 0)), 1.51e-07, "bottom"),
    ("slab", 4.0, 1, ((-1, 0, -1), (0, -1, -1)), 3.97e-10, "bottom"),
    ("slab", 5.0, 0, ((-1, 0, 0), (0, -1, 0)), 1.74e-09, "bottom"),
    ("slab", 5.0, 0, ((-2, -1, 0), (-1, 2, 0)), 4.43e-08, "bottom"),
    ("slab", 5.0, 0, ((-3, 0, 0), (0, -3, 0)), 1.46e-07, "bottom"),
    ("slab", 5.0, 0, ((-3, -2, 0), (-2, 3, 0)), 3.09e-07, "bottom"),
    ("rod", 2.5, 1.5, ((-1, -1, 0), (1, 0, -1)), 3.43e-08, "top"),
    ("rod", 2.5, 1.5, ((-1, 1, 0), (1, 0, 1), (2, 0, 0)), 3.47e-08, "top"),
    ("rod", 2.5, 1.5, ((-1, 1, 1), (1, -1, 1)), 1.45e-07, "top"),
    ("rod", 2.5, 1.5, ((-1, -1, 1), (-1, 0, 0), (1, 1, 1)), 1.65e-07, "top"),
    ("rod", 3.0, 1.5, ((-1, -1, 0), (1, 0, -1)), 4.31e-08, "top"),
    ("rod", 3.0, 1.5, ((-1, 1, -1), (1, 1, 1)), 1.74e-07, "top"),
    ("rod", 3.0, 1, ((-1, -1, 0), (1, 0, -1)), 4.65e-07, "top"),
    ("rod", 4.0, 1, ((-2, -1, 0), (2, 0, -1)), 5.74e-10, "top"),
    ("rod", 4.0, 1, ((-2, 1, 0), (0, 0, -1), (2, 0, 0)), 1.37e-07, "top"),
    ("rod", 4.0, 1.5, ((-3, 0, 1), (1, -1, 0)), 1.79e-08, "top"),
    ("rod", 5.0, 1, ((-3, -1, 0), (-1, 0, 0), (3, 0, -1)), 1.08e-09, "top"),
    ("rod", 5.0, 1, ((-4, 0, -1), (3, 1, 0)), 1.32e-08, "top"),
    ("rod", 5.0, 1, ((-3, 0, 1), (-2, 1, 0)), 5.57e-08, "top"),
    ("rod", 5.0, 1.5, ((-2, -1, 0), (2, 0, -1)), 2.45e-10, "top"),
    ("slab", 2.0, 1, ((-1, -1, -1), (-1, 1, -1), (1, 0, 1)), 1.5e-06, "bottom"),
    ("slab", 2.0, 1, ((-1, 0, 0), (0, 0, -1), (0, 1, 0)), 5.92e-05, "bottom"),
    ("slab", 2.5, 0, ((-1, 0, 0), (0, -1, 0)), 7.66e-06, "bottom"),
    ("slab", 2.5, 0, ((-1, -1, 0), (-1, 1, 0)), 3.27e-05, "bottom"),
    ("slab", 2.5, 1, ((-1, -1, -1), (-1, 1, 0), (0, 0, -1)), 1.12e-06, "bottom"),
    ("slab", 2.5, 1, ((-2, 0, -1), (0, 0, -1), (0, 2, 0)), 4.87e-06, "bottom"),
    ("slab", 3.0, 0, ((-2, -2, 0), (-1, 2, 0), (2, -1, 0)), 1.28e-06, "bottom"),
    ("slab", 3.0, 0, ((0, 2, 0), (2, 0, 0)), 1.61e-05, "bottom"),
    ("slab", 3.0, 1, ((-2, -1, -1), (-1, 2, 0)), 1.07e-06, "bottom"),
    ("slab", 4.0, 0, ((-2, -2, 0), (-2, 2, 0)), 2.57e-06, "bottom"),
    ("slab", 4.0, 0, ((-3, -1, 0), (1, -3, 0)), 4.11e-06, "bottom"),
    ("slab", 5.0, 0, ((-5, 0, 0), (0, -5, 0)), 1.2e-06, "bottom"),
    ("slab", 5.0, 0, ((-1, -1, 0), (2, -1, 0)), 3.57e-05, "bottom"),
    ("rod", 2.0, 1, ((-1, -1, 0), (1, 0, -1)), 1.21e-05, "top"),
    ("rod", 2.0, 1, ((-1, 0, -1), (1, -1, 0), (1, 0, 0)), 2.59e-05, "top"),
    ("rod", 2.0, 1.5, ((0, -1, 0), (0, 0, -1)), 5.04e-05, "top"),
    ("rod", 2.5, 1, ((0, -1, 0), (0, 0, -1)), 3.37e-06, "top"),
    ("rod", 2.5, 1.5, ((-2, -1, 0), (-1, 0, 0), (1, 0, -1)), 1.02e-06, "top"),
    ("rod", 2.5, 1.5, ((-1, 1, -1), (0, 1, 1), (1, 0, 0)), 2.11e-06, "top"),
    ("rod", 3.0, 1, ((-3, 0, 0), (-1, -1, 0), (2, 0, -1)), 1.17e-06, "top"),
    ("rod", 3.0, 1, ((0, -1, 0), (1, 0, 0), (1, 0, 1)), 1.83e-06, "top"),
    ("rod", 4.0, 1, ((-3, -1, 0), (-2, 0, -1), (-2, 0, 0)), 1.02e-06, "top"),
    ("rod", 4.0, 1.5, ((0, -1, 0),), 1.32e-05, "top"),
    ("rod", 5.0, 1, ((-4, -1, 0), (0, 0, -1), (0, 0, 1)), 6.37e-06, "top"),
    ("rod", 5.0, 1.5, ((0, -1, 0),), 2.67e-06, "top"),
)
NO_BAND_LEGS = ("W3",)
NO_NEAR_LEGS = ("W3", "W5")
# r/e = 1 sees the query's cell and up to six face neighbors.  of the 63 non-empty neighbor sets none is
# generic with r < 0: the spectra are, up to symmetry, (1,0,0), (8,3,0), (3,1,0), (10,5,3) - all r > 0 - and
# the double or triple roots (tests/test_eigen_reference_cpu.py enumerates them)
NO_GENERIC_BOTTOM_LEGS = ("W3",)


BASES = {"slab": slab, "rod": rod}


def frozen_cells(entry):
    kind, rho, half, removed = entry[:4]
    return minus(BASES[kind](rho, half), removed)


def patterns_for_leg(rho):
    """[(name, cells)] of the islands of the leg with r/e = rho.  balls one size up give interior queries
    whose neighborhood is the whole ball of the leg (triple roots), discs and planes the planar double roots,
    lines the collinear ones; their rims give the generic neighborhoods."""
    out = []
    big = min(rho + 1.5, 6.5)
    for b in BALL_RADII:
        if b <= big:
            out.append(("ball%g" % b, ball(b)))
    out.append(("ball%g" % big, ball(big)))
    for b in BALL_RADII:
        if b <= rho + 1.0:
            for axis in (0, 1, 2):
                out.append(("disc%g/%d" % (b, axis), slab(b, 0, axis)))
            out.append(("slab%g" % b, slab(b, 1)))
    for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, -1), (1, 1, 1), (1, -1, 1), (2, 1, 0)):
        out.append(("line%d%d%d" % d, line(d, 3)))
    out.append(("pair", ((0, 0, 0), (1, 0, 0))))
    out.append(("pair_diag", ((0, 0, 0), (1, 1, 0))))
    for nrm in ((0, 0, 1), (1, 1, 0), (1, 1, 1), (1, 2, 0)):
        out.append(("plane%d%d%d" % nrm, plane(nrm, min(rho + 1.0, 4.0))))
    base = ball(min(rho, 3.0))
    rim = [c for c in base if c[0] > 0 and c[1] >= 0][:3]
    for k in (1, 2, 3):
        out.append(("ball-%d" % k, minus(base, rim[:k])))
        d = slab(min(rho, 3.0), 0)
        out.append(("disc-%d" % k, minus(d, [c for c in d if c[0] > 0 and c[1] >= 0][:k])))
    for salt in (1, 2, 3):
        out.append(("blob%d" % salt, blob(min(rho + 1.0, 4.0), salt)))
    for entry in FROZEN:
        if entry[1] <= rho:
            out.append(("%s%g/%g-%d" % (entry[0], entry[1], entry[2], len(entry[3])), frozen_cells(entry)))
    return out


# ---- island clouds ----------------------------------------------------------------------------------------

class IslandCloud(object):
    """islands tiled in a 3-D grid.  .cells (N,3) int64 global cell coordinates, .points = cells * edge
    (exact), .island (N,) island number, .names.  gap_cells: free cells between the bounding boxes of two
    islands; it must exceed 2*factor*rho + 2."""

    def __init__(self, patterns, gap_cells, edge=E, origin=(-37, 5, 11)):
        ext = 1 + max(max(max(c[a] for c in cells) - min(c[a] for c in cells) for a in range(3))
                      for _, cells in patterns)
        pitch = ext + int(gap_cells)
        side = int(np.ceil(len(patterns) ** (1.0 / 3.0)))
        cells, island = [], []
        for num, (_, pat) in enumerate(patterns):
            arr = np.asarray(pat, dtype=np.int64).reshape(-1, 3)
            slot = np.array([num % side, (num // side) % side, num // (side * side)], dtype=np.int64)
            cells.append(arr - arr.min(0) + slot * pitch + np.asarray(origin, dtype=np.int64))
            island.append(np.full(len(arr), num, dtype=np.int64))
        self.names = [name for name, _ in patterns]
        self.cells = np.concatenate(cells, axis=0)
        self.island = np.concatenate(island)
        self.edge = edge
        self.points = self.cells.astype(np.float64) * edge
        assert np.array_equal(self.points / edge, self.cells)


def leg_cloud(rho):
    return IslandCloud(patterns_for_leg(rho), gap_cells=int(np.ceil(2 * rho)) + 3)


def island_neighborhoods(cloud, rho, rows_of=None):
    """exact integer sums of every query's neighborhood (the island's cells within rho cells of the query):
    n (N,), U = n*c - S1 (N,3) (n/e times the vector from the centroid to the query), A (N,6) = upper
    triangle of n*S2 - S1*S1^T.  all int64, taken in island-local coordinates (A and U do not depend on the
    origin); rows_of = a function island cells -> neighborhood mask overrides the ball."""
    lim = int(round(4 * rho * rho))
    total = len(cloud.cells)
    n = np.zeros(total, dtype=np.int64)
    U = np.zeros((total, 3), dtype=np.int64)
    A = np.zeros((total, 6), dtype=np.int64)
    iu = np.triu_indices(3)
    for num in range(len(cloud.names)):
        rows = np.flatnonzero(cloud.island == num)
        c = cloud.cells[rows] - cloud.cells[rows].min(0)
        d = c[:, None, :] - c[None, :, :]
        mask = (4 * (d * d).sum(2) <= lim) if rows_of is None else rows_of(c)
        mask = mask.astype(np.int64)
        cnt = mask.sum(1)
        s1 = mask @ c
        s2 = mask @ (c[:, :, None] * c[:, None, :])[:, iu[0], iu[1]]
        assert (cnt * np.abs(s2).max(1)).max() < 2 ** 52
        n[rows] = cnt
        U[rows] = cnt[:, None] * c - s1
        A[rows] = cnt[:, None] * s2 - (s1[:, :, None] * s1[:, None, :])[:, iu[0], iu[1]]
    return n, U, A


def lattice_neighborhoods(k, m, rho):
    """the general form, for clouds whose neighborhoods are not confined to islands (the ladder test): k (N,3)
    int64 = point coordinates in units of the finest edge with min 0 on every axis, m = this scale's edge
    in those units (1, 2, 4), rho = r/e of the scale.  the scale's cells are j = floor(k/m + 1/2) (the
    lattice's minimum corner is half a cell below the cloud's minimum), its voxel centres j*m; a voxel is in
    a query's neighborhood when |k - j*m|^2 <= (rho*m)^2, all integers.  returns n, U = n*k - S1(j*m), A of
    the cells j, like island_neighborhoods."""
    from scipy.spatial import cKDTree
    k = np.asarray(k, dtype=np.int64)
    assert (k.min(0) == 0).all()
    j = np.unique((2 * k + m) // (2 * m), axis=0)
    lists = cKDTree(j.astype(np.float64) * m).query_ball_point(k.astype(np.float64), rho * m + 0.25)
    lim = int(round(4 * rho * rho * m * m))
    iu = np.triu_indices(3)
    n = np.zeros(len(k), dtype=np.int64)
    U = np.zeros((len(k), 3), dtype=np.int64)
    A = np.zeros((len(k), 6), dtype=np.int64)
    for i, idx in enumerate(lists):
        c = j[np.asarray(idx, dtype=np.int64)].reshape(-1, 3)
        c = c[4 * ((c * m - k[i]) ** 2).sum(1) <= lim]
        n[i] = len(c)
        if not len(c):
            continue
        ref = c[0].copy()
        d = c - ref
        s1 = d.sum(0)
        s2 = (d[:, :, None] * d[:, None, :])[:, iu[0], iu[1]].sum(0)
        U[i] = n[i] * (k[i] - ref * m) - s1 * m
        A[i] = n[i] * s2 - (s1[:, None] * s1[None, :])[iu]
    return n, U, A


# ---- exact reference --------------------------------------------------------------------------------------

def scatter_of_points(points):
    """(n, A) for an explicit point list whose coordinates are dyadic: scaled to integers (a power of two
    that makes every coordinate whole), then n*S2 - S1*S1^T in Python ints.  normalised eigenvalues do not
    depend on the scale."""
    fr = [[Fraction(float(v)) for v in p] for p in np.asarray(points, dtype=np.float64)[:, :3]]
    scale = max(v.denominator for p in fr for v in p)
    pts = [[int(v * scale) for v in p] for p in fr]
    n = len(pts)
    s1 = [sum(p[a] for p in pts) for a in range(3)]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    return n, tuple(n * sum(p[a] * p[b] for p in pts) - s1[a] * s1[b] for a, b in pairs)


class EigenRef(object):
    """exact spectrum of one scatter matrix.  .f = the three eigenvalues over the trace, descending, as
    correctly rounded floats (.f_mp: mpmath); .classes = set of branch labels, .label = the primary one;
    .t = the solver's switch variable (float; 0.0 exactly for double roots, None for triple);
    .collinear / .planar: rank <= 1 / rank 2 in exact arithmetic; .gap = (l1 - l2) / trace."""
    __slots__ = ("f", "f_mp", "classes", "label", "t", "top", "collinear", "planar", "gap", "A")


def _det3(a00, a01, a02, a11, a12, a22):
    return a00 * (a11 * a22 - a12 * a12) - a01 * (a01 * a22 - a12 * a02) + a02 * (a01 * a12 - a11 * a02)


@functools.lru_cache(maxsize=None)
def exact_eigen(A):
    """A = (a00, a01, a02, a11, a12, a22), Python ints, positive trace."""
    a00, a01, a02, a11, a12, a22 = (int(v) for v in A)
    tr = a00 + a11 + a22
    assert tr > 0
    m00, m11, m22, m01, m02, m12 = 3 * a00 - tr, 3 * a11 - tr, 3 * a22 - tr, 3 * a01, 3 * a02, 3 * a12
    P2 = m00 * m00 + m11 * m11 + m22 * m22 + 2 * (m01 * m01 + m02 * m02 + m12 * m12)
    D = _det3(m00, m01, m02, m11, m12, m22)
    ref = EigenRef()
    ref.A = (a00, a01, a02, a11, a12, a22)
    minors = (a00 * a11 - a01 * a01, a00 * a22 - a02 * a02, a11 * a22 - a12 * a12,
              a00 * a12 - a01 * a02, a01 * a12 - a02 * a11, a01 * a22 - a02 * a12)
    ref.collinear = all(v == 0 for v in minors)
    ref.planar = (not ref.collinear) and _det3(a00, a01, a02, a11, a12, a22) == 0
    ref.top = D >= 0
    side = "top" if ref.top else "bottom"
    with mpmath.workdps(MP_DIGITS):
        third = mpmath.mpf(1) / 3
        if P2 == 0:
            ref.t = None
            ref.label = "triple"
            xs = (mpmath.mpf(0),) * 3
            scale = mpmath.mpf(0)
        else:
            r2 = Fraction(54 * D * D, P2 ** 3)
            assert r2 <= 1
            if r2 == 1:
                ref.t = 0.0
                ref.label = "double_" + side
                x, s3 = mpmath.mpf(2), mpmath.mpf(0)
            else:
                theta = mpmath.acos(mpmath.sqrt(mpmath.mpf(r2.numerator) / r2.denominator)) / 3
                x = 2 * mpmath.cos(theta)
                t = mpmath.sin(theta) ** 2
                s3 = mpmath.sqrt(3 * t)
                ref.t = float(t)
                if ref.t < NEAR_T:
                    ref.label = "near_" + side
                elif ref.t < BAND_LO:
                    ref.label = "switch_" + side        # either branch may take it; not a required class
                elif ref.t < BAND_HI:
                    ref.label = "band_" + side
                else:
                    ref.label = "generic_" + side
            xs = (x, s3 - x / 2, -x / 2 - s3) if ref.top else (x / 2 + s3, x / 2 - s3, -x)
            # lambda/tr = 1/3 + (p/tr) x with p = sqrt(p2/6), p2 = P2/9
            scale = mpmath.sqrt(mpmath.mpf(P2) / 54) / tr
        ref.f_mp = tuple(third + scale * v for v in xs)
        ref.f = tuple(float(v) for v in ref.f_mp)
        ref.gap = float(ref.f_mp[1] - ref.f_mp[2])
    ref.classes = {ref.label}
    if ref.collinear:
        ref.classes.add("rank1")
    return ref


@functools.lru_cache(maxsize=None)
def exact_normal(A):
    """unit eigenvector of the smallest eigenvalue (which must be simple), last non-zero component positive:
    the largest cross product of two rows of A - lambda*I, in mpmath.  returns three floats."""
    ref = exact_eigen(A)
    a00, a01, a02, a11, a12, a22 = ref.A
    with mpmath.workdps(MP_DIGITS):
        lam = ref.f_mp[2] * (a00 + a11 + a22)
        rows = ((a00 - lam, mpmath.mpf(a01), mpmath.mpf(a02)), (mpmath.mpf(a01), a11 - lam, mpmath.mpf(a12)),
                (mpmath.mpf(a02), mpmath.mpf(a12), a22 - lam))
        best, best_n = None, -1
        for i, j in ((0, 1), (0, 2), (1, 2)):
            u, w = rows[i], rows[j]
            v = (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])
            nn = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
            if nn > best_n:
                best, best_n = v, nn
        norm = mpmath.sqrt(best_n)
        v = [c / norm for c in best]
        v = [c if abs(c) > mpmath.mpf(10) ** (-MP_DIGITS // 2) else mpmath.mpf(0) for c in v]
        last = [c for c in v if c != 0][-1]
        if last < 0:
            v = [-c for c in v]
        return tuple(float(c) for c in v)


def exact_covariance(n, A, edge=E):
    """upper triangle of the ddof=1 covariance, edge^2 * A / (n (n-1)), as Fractions"""
    f = Fraction(edge) ** 2 / (int(n) * (int(n) - 1))
    return tuple(f * int(v) for v in A)


def exact_centroid_distance(n, U, edge=E):
    """|query - centroid| = edge * |n*c - S1| / n, correctly rounded"""
    with mpmath.workdps(MP_DIGITS):
        return float(mpmath.sqrt(sum(int(v) ** 2 for v in U)) * mpmath.mpf(edge) / int(n))


def reference_rows(n, U, A):
    """per row of island_neighborhoods' output: (f0, f1) floats (zeros below two cells), centroid distance,
    the EigenRef (None below two cells)"""
    feats = np.zeros((len(n), 2))
    cent = np.zeros(len(n))
    refs = [None] * len(n)
    for i in range(len(n)):
        cent[i] = exact_centroid_distance(n[i], U[i])
        if n[i] >= 2:
            refs[i] = exact_eigen(tuple(int(v) for v in A[i]))
            feats[i] = refs[i].f[:2]
    return feats, cent, refs


@functools.lru_cache(maxsize=None)
def leg_reference(rho):
    """(cloud, n, U, A, feats (N,2), centroid (N,), refs) of a leg's island cloud: computed once per process,
    shared by the tests, never modified"""
    cloud = leg_cloud(rho)
    n, U, A = island_neighborhoods(cloud, rho)
    feats, cent, refs = reference_rows(n, U, A)
    for arr in (cloud.points, cloud.cells, n, U, A, feats, cent):
        arr.setflags(write=False)
    return cloud, n, U, A, feats, cent, refs


def count_classes(refs):
    counts = {}
    for r in refs:
        if r is not None:
            for c in r.classes:
                counts[c] = counts.get(c, 0) + 1
    return counts


def merged(counts):
    """near_* and band_* either side, as the coverage condition counts them"""
    out = dict(counts)
    for fam in ("near", "band"):
        out[fam] = counts.get(fam + "_top", 0) + counts.get(fam + "_bottom", 0)
    return out


# ---- the search that produced FROZEN (kept for the record; never called by a test) ---------------------------

def search_near_double(rho, half, max_removed, t_lo=0.0, t_hi=BAND_HI, limit=200000, kind="slab"):
    """base = slab(rho, half) or rod(rho, half); every way of removing up to max_removed cells other than the centre (the first
    `limit` combinations per count).  filters in extended precision on 1 - r^2 ~ 9t, confirms in exact
    arithmetic.  returns [(t, top, removed cells)] with t_lo < t < t_hi."""
    base = list(BASES[kind](rho, half))
    arr = np.asarray(base, dtype=np.int64)
    iu = np.triu_indices(3)
    full_n = len(arr)
    full_s1 = arr.sum(0)
    full_s2 = (arr[:, :, None] * arr[:, None, :])[:, iu[0], iu[1]].sum(0)
    movable = [i for i, c in enumerate(base) if c != (0, 0, 0)]
    hits = []
    for k in range(0, max_removed + 1):
        combos = np.asarray(list(itertools.islice(itertools.combinations(movable, k), limit)),
                            dtype=np.int64).reshape(-1, k) if k else np.zeros((1, 0), dtype=np.int64)
        gone = arr[combos]                                                   # (C, k, 3)
        n = full_n - k
        s1 = full_s1[None, :] - gone.sum(1)
        s2 = full_s2[None, :] - (gone[:, :, :, None] * gone[:, :, None, :])[:, :, iu[0], iu[1]].sum(1)
        A = n * s2 - (s1[:, :, None] * s1[:, None, :])[:, iu[0], iu[1]]
        tr = A[:, 0] + A[:, 3] + A[:, 5]
        M = (3 * A).astype(np.longdouble)
        for col in (0, 3, 5):
            M[:, col] -= tr
        P2 = M[:, 0] ** 2 + M[:, 3] ** 2 + M[:, 5] ** 2 + 2 * (M[:, 1] ** 2 + M[:, 2] ** 2 + M[:, 4] ** 2)
        D = _det3(M[:, 0], M[:, 1], M[:, 2], M[:, 3], M[:, 4], M[:, 5])
        with np.errstate(divide="ignore", invalid="ignore"):
            u = 1 - 54 * D * D / P2 ** 3
        for i in np.flatnonzero((u > 9 * t_lo * 0.5 - 1e-15) & (u < 9 * t_hi * 2)):
            ref = exact_eigen(tuple(int(v) for v in A[i]))
            if ref.t is not None and t_lo < ref.t < t_hi:
                hits.append((ref.t, ref.top, tuple(base[j] for j in combos[i])))
    return hits


# ---- the checks (shared by every path of tests/test_eigen_accuracy_gpu.py) ------------------------------------

def check_eigen_rows(path, got, n, feats, refs, bound=1e-13, planar_sum=None):
    """got (N,4) feature rows of one scale against the exact reference: population exact, both eigen columns
    within `bound` absolute, asserted and printed per class; the structural facts exactly where the exact
    answer is structural.  returns {class: (count, worst)}.  planar_sum: a list that receives the deviations
    |l0 + l1 - 1| of the exactly planar rows INSTEAD of their assertion here - for a caller that asserts the
    same 1e-15 itself after its other checks."""
    got = np.asarray(got)
    assert got.shape == (len(n), 4)
    assert np.array_equal(got[:, 0], n), "%s: population differs" % path
    assert not got[n < 2, 2:].any(), "%s: eigen-features of a neighborhood below two cells are not zero" % path
    err = np.abs(got[:, 2:] - feats).max(1)
    assert (got[:, 3] <= got[:, 2]).all(), "%s: l1 > l0" % path
    by_class = {}
    for i, ref in enumerate(refs):
        if ref is None:
            continue
        for cls in ref.classes:
            by_class.setdefault(cls, []).append(i)
    report = {}
    for cls in sorted(by_class):
        rows = np.asarray(by_class[cls])
        worst = float(err[rows].max())
        report[cls] = (len(rows), worst)
        print("%-28s %-15s n %5d  worst %.3g" % (path, cls, len(rows), worst))
    for cls, (count, worst) in sorted(report.items()):
        assert worst <= bound, "%s: class %s off by %.3g (row %d)" % (
            path, cls, worst, by_class[cls][int(np.argmax(err[np.asarray(by_class[cls])]))])
    for i, ref in enumerate(refs):
        if ref is None:
            continue
        l0, l1 = got[i, 2], got[i, 3]
        if ref.label == "triple":
            assert abs(l0 - 1.0 / 3.0) <= 1e-15 and abs(l1 - 1.0 / 3.0) <= 1e-15, (path, "triple", i, l0, l1)
        if ref.collinear:
            assert abs(l0 - 1.0) <= 1e-15 and abs(l1) <= 1e-15, (path, "collinear", i, l0, l1)
        if ref.planar and planar_sum is not None:
            planar_sum.append((abs(l0 + l1 - 1.0), path, i, ref.label, ref.t))
        elif ref.planar:
            assert abs(l0 + l1 - 1.0) <= 1e-15, (path, "planar", i, l0 + l1 - 1.0)
    return report


def check_centroid_rows(path, got, cent, points):
    """centroid column against the exact distance.  bound: 8 ulp of the largest coordinate (one subtraction
    at coordinate magnitude) plus 8 ulp of the value (an fma chain and a refined rsqrt at value magnitude)."""
    err = np.abs(np.asarray(got)[:, 1] - cent)
    tol = 8 * np.spacing(np.abs(points).max()) + 8 * np.spacing(cent)
    print("%-28s %-15s n %5d  worst %.3g (worst allowed/err ratio %.3g)" % (
        path, "centroid", len(cent), err.max(), (err / tol).max()))
    assert (err <= tol).all(), "%s: centroid off by %.3g, %.3g allowed" % (
        path, err.max(), tol[int(np.argmax(err / tol))])
