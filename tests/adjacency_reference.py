"""
numpy reference for NeighborIndex.adjacency and NeighborIndex.prominent_peaks (no GPU), on the pairs of
components_reference.edges and the segments of hill_climb_reference.hill_climb_of_edges.

adjacency: the graph is that of components() - u ~ v when (dx*dx + dy*dy) + dz*dz <= r*r on their centres and both
carry the same class >= 0 - less the voxels whose value is NaN.  an edge {u, v} crosses when label[u] and label[v] are
both >= 0 and differ.  one row per unordered pair of labels a < b that a crossing edge joins: links = the number of
such edges, saddle = the largest min(value[u], value[v]) over them; rows ascend by (a, b).

prominent_peaks: hill_climb's segments 0..S-1 with peak values p; a is HIGHER than b when p[a] > p[b] or (p[a] == p[b]
and a < b).  the adjacency's rows by descending saddle, equal saddles by ascending (a, b), go through a union-find:
ra = find(a), rb = find(b), nothing where they are equal; lo the lower root, hi the higher; p[lo] - s < min_prominence
(strict) merges lo under hi, hi stays the root; otherwise lo's prominence, if none is recorded yet, is p[lo] - s.  a
root that never loses keeps +inf.  the surviving roots are the segments: sizes are sums of weights, segments below
min_size are dropped, the others numbered by ascending peak position.
plain loops: slow and obviously right.
"""

import numpy as np

import components_reference as cref
import hill_climb_reference as href

EDGE = cref.EDGE


def adjacency_of_edges(labels, edges, value=None, cls=None):
    """(pair int64 (E, 2), links int64 (E,), saddle fp64 (E,) or None): `edges` are components_reference.edges"""
    labels = np.asarray(labels, dtype=np.int64)
    i, j = edges
    ok = (labels[i] >= 0) & (labels[j] >= 0) & (labels[i] != labels[j])
    if cls is not None:
        cls = np.asarray(cls, dtype=np.int64)
        ok &= (cls[i] >= 0) & (cls[i] == cls[j])
    if value is not None:
        value = np.asarray(value, dtype=np.float64)
        ok &= (value[i] == value[i]) & (value[j] == value[j])
    i, j = i[ok], j[ok]
    rows = {}
    for u, v in zip(i.tolist(), j.tolist()):
        a, b = int(labels[u]), int(labels[v])
        key = (min(a, b), max(a, b))
        links, saddle = rows.get(key, (0, None))
        if value is not None:
            low = min(float(value[u]), float(value[v]))
            saddle = low if saddle is None else max(saddle, low)
        rows[key] = (links + 1, saddle)
    keys = sorted(rows)
    pair = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
    links = np.asarray([rows[k][0] for k in keys], dtype=np.int64)
    saddle = None if value is None else np.asarray([rows[k][1] for k in keys], dtype=np.float64)
    return pair, links, saddle


def adjacency(voxels, radius, labels, value=None, cls=None):
    return adjacency_of_edges(labels, cref.edges(voxels, radius), value, cls)


def merge_by_prominence(p, pair, saddle, min_prominence):
    """(root int64 (S,), prom fp64 (S,)): the union-find of the contract.  prom of a root: what was recorded, +inf if
    it never lost; of a merged segment: the p[lo] - s it was merged at"""
    p = np.asarray(p, dtype=np.float64)
    pair = np.asarray(pair, dtype=np.int64).reshape(-1, 2)
    saddle = np.asarray(saddle, dtype=np.float64)
    n_seg = len(p)
    parent = list(range(n_seg))
    prom = np.full(n_seg, np.inf)
    recorded = [False] * n_seg

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    def higher(a, b):
        return p[a] > p[b] or (p[a] == p[b] and a < b)

    order = sorted(range(len(pair)), key=lambda e: (-saddle[e], pair[e, 0], pair[e, 1]))
    for e in order:
        a, b, s = int(pair[e, 0]), int(pair[e, 1]), saddle[e]
        ra, rb = find(a), find(b)
        if ra == rb:
            continue
        lo, hi = (rb, ra) if higher(ra, rb) else (ra, rb)
        rise = p[lo] - s
        if rise < min_prominence:
            parent[lo] = hi
            prom[lo] = rise
        elif not recorded[lo]:
            recorded[lo] = True
            prom[lo] = rise
    root = np.asarray([find(c) for c in range(n_seg)], dtype=np.int64)
    return root, prom


def segments_of_roots(labels0, peaks0, root, prom, voxel_weight=None, min_size=1):
    """step 4: (labels, sizes, peaks, prominence) of the surviving roots"""
    labels0 = np.asarray(labels0, dtype=np.int64)
    m = len(labels0)
    weight = np.ones(m, dtype=np.int64) if voxel_weight is None else np.asarray(voxel_weight, dtype=np.int64)
    labels = np.full(m, -1, dtype=np.int64)
    sizes, peaks, prominence = [], [], []
    for c in range(len(root)):                   # ascending segment = ascending peak position
        if root[c] != c:
            continue
        members = (labels0 >= 0) & (root[np.maximum(labels0, 0)] == c)
        size = int(weight[members].sum())
        if size >= min_size:
            labels[members] = len(sizes)
            sizes.append(size)
            peaks.append(int(peaks0[c]))
            prominence.append(prom[c])
    return (labels, np.asarray(sizes, dtype=np.int64), np.asarray(peaks, dtype=np.int64),
            np.asarray(prominence, dtype=np.float64))


def prominent_peaks_of_edges(voxels, edges, value, min_prominence, mode="highest", voxel_class=None,
                             voxel_weight=None, min_size=1):
    """(labels int64 (m,), sizes int64 (C,), peaks int64 (C,), prominence fp64 (C,))"""
    value = np.asarray(value, dtype=np.float64)
    labels0, _, peaks0, _, _ = href.hill_climb_of_edges(voxels, edges, value, mode, voxel_class=voxel_class)
    pair, _, saddle = adjacency_of_edges(labels0, edges, value, voxel_class)
    root, prom = merge_by_prominence(value[peaks0], pair, saddle, min_prominence)
    return segments_of_roots(labels0, peaks0, root, prom, voxel_weight, min_size)


def prominent_peaks(voxels, radius, value, min_prominence, mode="highest", **kwargs):
    return prominent_peaks_of_edges(voxels, cref.edges(voxels, radius), value, min_prominence, mode, **kwargs)


def same_partition(a, b):
    """do two labellings (-1: in none) cut the voxels into the same sets, whatever the numbering?"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    inside = a >= 0
    both = np.unique(np.stack((a[inside], b[inside]), axis=1), axis=0)
    return len(both) == len(np.unique(a[inside])) == len(np.unique(b[inside]))


# ---- inputs --------------------------------------------------------------------------------------------------------
centres = href.centres
row_cells = href.row_cells

# a line of five voxels at a radius of one edge: segments {0, 1} (peak 3 at position 1) and {2, 3, 4} (peak 5 at
# position 3); the one crossing edge is {1, 2}: saddle min(3, 2) = 2, the lower peak's prominence 3 - 2 = 1 exactly
LINE_VALUES = [1.0, 3.0, 2.0, 5.0, 4.0]
LINE_LABELS = [0, 0, 1, 1, 1]
LINE_PEAKS = [1, 3]

# three peaks in a chain along a row of seven: positions 1, 3, 5 carry the peaks, 2 and 4 the passes.  segments are
# numbered by peak position, so A = segment 0 (position 1), B = 1, C = 2 - with A > B > C in value
CHAIN_PEAKS = [1, 3, 5]


def chain_values(a, b, c, s_ab, s_bc):
    """a row of seven: slopes, peak A, pass, peak B, pass, peak C, slope.  a pass voxel climbs to the higher of its
    two neighbors, so it belongs to A (or B), and the saddle of the pair is the pass voxel's own value"""
    return [a - 10.0, a, s_ab, b, s_bc, c, c - 10.0]


def quantised(values, levels):
    """values on `levels` equally spaced levels of their range: plateaus and equal saddles"""
    values = np.asarray(values, dtype=np.float64)
    lo, hi = np.nanmin(values), np.nanmax(values)
    return np.floor(levels * (values - lo) / ((hi - lo) * (1.0 + 1e-9)))


def random_segment_graph(rng, n_seg, levels=5):
    """a small random segment graph for the host merge: (p (S,), pair (E, 2) ascending, saddle (E,)), values on a
    handful of levels so that ties are common, every saddle <= both peaks"""
    p = rng.integers(0, levels, n_seg).astype(np.float64)
    rows = [(a, b) for a in range(n_seg) for b in range(a + 1, n_seg) if rng.random() < 0.4]
    pair = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    top = np.minimum(p[pair[:, 0]], p[pair[:, 1]])
    saddle = top - rng.integers(0, levels, len(pair)).astype(np.float64)
    return p, pair, saddle
