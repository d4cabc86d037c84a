"""
the exact reference and the case catalogue of tests/eigen_cases.py, checked without a GPU: the reference
computes what the oracle computes, the catalogue reaches every branch of the eigen-solver on every kernel leg,
and LAPACK on the same exact matrices shows what fp64 can deliver (the yardstick printed next to the kernels'
figures in tests/test_eigen_accuracy_gpu.py and DESIGN.md).
"""

import itertools

import mpmath
import numpy as np

import eigen_cases as ec
from oracle import nimrud_oracle as oracle

REQUIRED = ("triple", "double_top", "double_bottom", "generic_top", "generic_bottom")


def test_reference_agrees_with_the_oracle():
    """same quantity: population exactly, centroid distance and both eigen-features within the oracle's own
    fp64 noise (1e-9; the coordinates are small) on every neighborhood of the W7 leg's cloud (> 2000)."""
    rho = 2.5
    cloud, n, U, A, feats, cent, refs = ec.leg_reference(rho)
    want = oracle.one_scale(cloud.points, cloud.points, ec.E, rho * ec.E)
    assert len(want) >= 200
    assert np.array_equal(want[:, 0], n)
    assert np.abs(want[:, 1] - cent).max() <= 1e-9
    assert np.abs(want[:, 2:] - feats).max() <= 1e-9
    rows = np.flatnonzero(n >= 2)[::7]
    for i in rows:
        cov = np.array([float(v) for v in ec.exact_covariance(n[i], A[i])])
        nb = cloud.points[(cloud.island == cloud.island[i]) &
                          (((cloud.cells - cloud.cells[i]) ** 2).sum(1) * 4 <= round(4 * rho * rho))]
        assert len(nb) == n[i]
        assert np.abs(np.cov(nb, rowvar=False)[np.triu_indices(3)] - cov).max() <= 1e-9


def test_closed_form_agrees_with_mpmath_eigsy_and_the_frozen_patterns_are_what_they_say():
    """the reference's closed form of the cubic against mpmath's own symmetric eigen-solver at 80 digits, on
    every class; and each frozen pattern, recomputed exactly, has the t and the side recorded beside it."""
    seen = {}
    for _, rho in ec.LEGS[1:4]:
        for ref in ec.leg_reference(rho)[6]:
            if ref is not None and seen.get(ref.label, 0) < 12:
                seen[ref.label] = seen.get(ref.label, 0) + 1
                a00, a01, a02, a11, a12, a22 = ref.A
                with mpmath.workdps(ec.MP_DIGITS):
                    w = mpmath.eigsy(mpmath.matrix([[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]),
                                     eigvals_only=True)
                    w = sorted((v / (a00 + a11 + a22) for v in w), reverse=True)
                    assert max(abs(a - b) for a, b in zip(w, ref.f_mp)) < mpmath.mpf(10) ** -60
    assert len(seen) >= 9
    for entry in ec.FROZEN:
        n, A = ec.scatter_of_points(np.asarray(ec.frozen_cells(entry), dtype=np.float64))
        ref = ec.exact_eigen(A)
        assert abs(ref.t - entry[4]) <= 0.01 * entry[4], entry
        assert ref.top == (entry[5] == "top"), entry
        assert ref.label.split("_")[0] in ("near", "band"), entry


def test_unit_radius_has_no_generic_neighborhood_with_negative_r():
    """the exemption NO_GENERIC_BOTTOM_LEGS = (W3,) is a fact: all 63 neighborhoods of r/e = 1 enumerated"""
    faces = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
    labels = set()
    for k in range(1, 7):
        for sub in itertools.combinations(faces, k):
            n, A = ec.scatter_of_points(np.asarray(((0, 0, 0),) + sub, dtype=np.float64))
            labels.add(ec.exact_eigen(A).label)
    assert labels == {"triple", "double_top", "double_bottom", "generic_top"}


def test_catalogue_covers_every_branch_on_every_leg():
    """a condition, not a measurement.  exemptions are by leg name and stated in eigen_cases.py."""
    for name, rho in ec.LEGS:
        cloud, n, U, A, feats, cent, refs = ec.leg_reference(rho)
        assert len(cloud.points) <= 20000
        counts = ec.merged(ec.count_classes(refs))
        print("%-12s %5d points  %s" % (name, len(cloud.points),
                                        "  ".join("%s %d" % kv for kv in sorted(counts.items()))))
        for cls in REQUIRED:
            if cls == "generic_bottom" and name in ec.NO_GENERIC_BOTTOM_LEGS:
                assert counts.get(cls, 0) == 0
                continue
            assert counts.get(cls, 0) >= 3, (name, cls)
        assert counts.get("rank1", 0) >= 3, name
        if name not in ec.NO_BAND_LEGS:
            assert counts["band"] >= 3, name
        if name not in ec.NO_NEAR_LEGS:
            assert counts["near"] >= 3, name
            assert counts.get("near_top", 0) >= 1 and counts.get("near_bottom", 0) >= 1, name
    assert set(ec.NO_BAND_LEGS) <= {"W3"} and set(ec.NO_NEAR_LEGS) <= {"W3", "W5"}


def test_calibration_numpy_eigvalsh_on_the_exact_matrices():
    """what fp64 delivers: LAPACK (numpy.linalg.eigvalsh) on A as float64 (exact: the entries are integers
    below 2^53) against the exact reference, worst normalised-eigenvalue error per class."""
    worst = {}
    for name, rho in ec.LEGS:
        refs = [r for r in ec.leg_reference(rho)[6] if r is not None]
        mats = np.zeros((len(refs), 3, 3))
        for i, r in enumerate(refs):
            a00, a01, a02, a11, a12, a22 = r.A
            mats[i] = [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]
        w = np.linalg.eigvalsh(mats)
        w = w / np.trace(mats, axis1=1, axis2=2)[:, None]
        want = np.array([r.f for r in refs])
        err = np.abs(w[:, ::-1] - want)[:, :2].max(1)
        for r, e in zip(refs, err):
            worst[r.label] = max(worst.get(r.label, 0.0), float(e))
    for label in sorted(worst):
        print("calibration numpy.linalg.eigvalsh  %-15s worst %.3g" % (label, worst[label]))
    assert max(worst.values()) < 1e-13
