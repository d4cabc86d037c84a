"""
numpy reference of the segment table (nm_segment_table / multiscale.segment_table), one segment at a time, and the
error bounds the GPU tests hold the kernel to.  this is also "the only route before the kernel": download, group,
reduce on the CPU (tools/segments_timing.py times it).

per segment: n, min and max exact; the centroid from math.fsum per axis over the weighted rows and one division;
the covariance np.cov(p - p.min(0), rowvar=False, fweights=w, ddof=1); eigenpairs from np.linalg.eigh.
rows of weight 0 count for nothing (frequency weights: they are not there).
"""

import math

import numpy as np

COLUMNS = 25
U = 2.0 ** -53


def orient(v):
    """the table's sign rule: last non-zero of (x, y, z) positive; below 1e-12 a component counts as zero"""
    v = np.asarray(v, dtype=np.float64)
    for a in (2, 1, 0):
        if abs(v[a]) > 1e-12:
            return v if v[a] > 0 else -v
    return v


def segment_row(points, weights=None):
    """the 25 columns of one segment from its rows (r, 3) and integer weights (r,) or None"""
    row = np.zeros(COLUMNS)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    w = np.ones(len(p), dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    keep = w > 0
    p, w = p[keep], w[keep]
    n = int(w.sum())
    if n == 0:
        return row
    row[0] = n
    for a in range(3):
        row[1 + a] = math.fsum(float(x) * int(k) for x, k in zip(p[:, a], w)) / n
    row[4:7] = p.min(0)
    row[7:10] = p.max(0)
    if n < 2:
        return row
    cov = np.atleast_2d(np.cov(p - p.min(0), rowvar=False, fweights=w, ddof=1))
    row[10:16] = [cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2]]
    if not np.trace(cov) > 0.0:
        return row
    lam, vec = np.linalg.eigh(cov)          # ascending
    row[16:19] = lam[::-1]
    if len(p) >= 3:
        row[19:22] = orient(vec[:, 0])
        row[22:25] = orient(vec[:, 2])
    return row


def segment_table(points, labels, weights=None, n_segments=None):
    """(C, 25): group the rows by label (a stable sort, so every segment's rows ascend) and reduce each segment"""
    points = np.asarray(points, dtype=np.float64)[:, :3]
    labels = np.asarray(labels, dtype=np.int64)
    if n_segments is None:
        n_segments = int(labels.max()) + 1 if len(labels) else 0
    c = max(int(n_segments), 0)
    table = np.zeros((c, COLUMNS))
    valid = (labels >= 0) & (labels < c)
    rows = np.nonzero(valid)[0]
    rows = rows[np.argsort(labels[rows], kind="stable")]
    start = np.searchsorted(labels[rows], np.arange(c + 1))
    for s in range(c):
        mine = rows[start[s]:start[s + 1]]
        if len(mine):
            table[s] = segment_row(points[mine], None if weights is None else np.asarray(weights)[mine])
    return table


# ---- the bounds (derived, not measured): u = 2^-53, r rows, D the box diagonal --------------------------------------

def tolerances(ref_row, rows, max_abs):
    """(tol_cov, tol_centroid, tol_eig) of a segment of `rows` rows whose reference row is ref_row.
    covariance: 8 (r + 4) u D^2 - r-term sums of products <= D^2 plus the S1 S1^T / n term.
    centroid: 4 (r + 4) u D + 2 u max|p|.  eigenvalues: 3 tol_cov (Weyl) + 1e-13 trace (the solver's own bar)."""
    d2 = float(((ref_row[7:10] - ref_row[4:7]) ** 2).sum())
    tol_cov = 8.0 * (rows + 4) * U * d2
    tol_centroid = 4.0 * (rows + 4) * U * math.sqrt(d2) + 2.0 * U * max_abs
    trace = float(ref_row[10] + ref_row[13] + ref_row[15])
    tol_eig = 3.0 * tol_cov + 1e-13 * trace
    return tol_cov, tol_centroid, tol_eig


def gap_of(ref_row, which):
    """distance from reference eigenvalue `which` (0 largest, 2 smallest) to the nearest other one"""
    lam = ref_row[16:19]
    return float(min(abs(lam[which] - lam[k]) for k in range(3) if k != which))


def sin_angle(a, b):
    """sine of the angle between two unit vectors, whatever their signs"""
    return float(np.linalg.norm(np.cross(a, b)))
