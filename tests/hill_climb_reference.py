"""
numpy reference for NeighborIndex.hill_climb (no GPU), on the pairs of components_reference.edges.

the contract: the graph is that of components() - u ~ v when (dx*dx + dy*dy) + dz*dz <= r*r on their centres and both
carry the same class.  a voxel is in the graph when its class is >= 0 and its value is no NaN.  u is HIGHER than v when
value[u] > value[v] or (value[u] == value[v] and u < v); a neighbor u of v is a candidate when it has v's class, a
value that is no NaN and is higher than v.  link[v] is, among the candidates,
    "highest": the largest value, among equal values the smaller d2, among equal d2 the smaller position
    "nearest": the smallest d2, among equal d2 the larger value, then the smaller position
with d2 = (dx*dx + dy*dy) + dz*dz on centre(v) - centre(u); v itself where there is none (a peak); -1 outside the
graph.  a segment is what the links lead to one peak; segments are numbered by ascending peak position, a segment's
size is the sum of its members' weights, segments below min_size are dropped and the others keep their order.
a plain loop over the voxels: slow and obviously right.
"""

import numpy as np

import components_reference as cref

MODES = ("highest", "nearest")


def higher(value, u, v):
    """the strict total order of the contract (False for NaN)"""
    return bool(value[u] > value[v] or (value[u] == value[v] and u < v))


def neighbor_lists(m, pairs):
    """per voxel the ascending positions of its neighbors (the voxel itself is left out: it is never higher than
    itself)"""
    i, j = pairs
    src, dst = np.concatenate((i, j)), np.concatenate((j, i))
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    start = np.searchsorted(src, np.arange(m + 1))
    return [dst[start[v]:start[v + 1]] for v in range(m)]


def links_of_edges(voxels, pairs, value, mode, voxel_class=None):
    """link int64 (m,): the uphill neighbor of every voxel, itself at a peak, -1 outside the graph"""
    assert mode in MODES
    voxels = np.asarray(voxels, dtype=np.float64)
    m = len(voxels)
    value = np.asarray(value, dtype=np.float64)
    cls = np.zeros(m, dtype=np.int64) if voxel_class is None else np.asarray(voxel_class, dtype=np.int64)
    assert value.shape == cls.shape == (m,)
    near = neighbor_lists(m, pairs)
    link = np.full(m, -1, dtype=np.int64)
    for v in range(m):
        if cls[v] < 0 or value[v] != value[v]:
            continue
        best, best_value, best_d2 = v, 0.0, 0.0
        for u in near[v]:                        # ascending position: "strictly better replaces"
            u = int(u)
            if cls[u] != cls[v] or value[u] != value[u] or not higher(value, u, v):
                continue
            dx, dy, dz = voxels[v] - voxels[u]
            d2 = (dx * dx + dy * dy) + dz * dz
            x = value[u]
            if best == v:
                better = True
            elif mode == "highest":
                better = x > best_value or (x == best_value and d2 < best_d2)
            else:
                better = d2 < best_d2 or (d2 == best_d2 and x > best_value)
            if better:
                best, best_value, best_d2 = u, x, d2
        link[v] = best
    return link


def roots_of_links(link):
    """root int64 (m,): the peak every voxel's chain of links ends in, -1 outside the graph"""
    m = len(link)
    root = np.full(m, -1, dtype=np.int64)
    for v in range(m):
        if link[v] < 0:
            continue
        x, steps = v, 0
        while link[x] != x:
            x = int(link[x])
            steps += 1
            assert steps <= m, "a cycle in the links"
        root[v] = x
    return root


def hill_climb_of_edges(voxels, pairs, value, mode="highest", voxel_class=None, voxel_weight=None, min_size=1):
    """(labels int64 (m,), sizes int64 (C,), peaks int64 (C,), link int64 (m,), total): `pairs` are
    components_reference.edges(voxels, radius); `total` counts the peaks before min_size"""
    m = len(voxels)
    weight = np.ones(m, dtype=np.int64) if voxel_weight is None else np.asarray(voxel_weight, dtype=np.int64)
    assert weight.shape == (m,)
    link = links_of_edges(voxels, pairs, value, mode, voxel_class)
    root = roots_of_links(link)
    labels = np.full(m, -1, dtype=np.int64)
    sizes, peaks = [], []
    total = 0
    for v in range(m):                           # ascending position: the peaks in their order (as components_of_edges)
        if link[v] != v:
            continue
        total += 1
        members = root == v
        size = int(weight[members].sum())
        if size >= min_size:
            labels[members] = len(sizes)
            sizes.append(size)
            peaks.append(v)
    return labels, np.asarray(sizes, dtype=np.int64), np.asarray(peaks, dtype=np.int64), link, total


def hill_climb(voxels, radius, value, mode="highest", **kwargs):
    """(labels, sizes, peaks, link) of the voxel graph at `radius`"""
    return hill_climb_of_edges(voxels, cref.edges(voxels, radius), value, mode, **kwargs)[:4]


# ---- inputs --------------------------------------------------------------------------------------------------------
EDGE = cref.EDGE


def centres(cells, edge=EDGE):
    """the voxel centres of integer cells listed in position order (z, then y, then x ascending)"""
    return (np.asarray(cells, dtype=np.float64) + 0.5) * edge


# the hand graphs: (cells in position order, values) and what is expected of them at a radius of one edge unless said
# otherwise.  all of them are rows along x at y = z = 0, so position = x
RAMP_VALUES = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]

# two bumps and a saddle: peaks at 1 (value 5) and 5 (value 7), the saddle 3 (value 1) between slopes 2 and 4 of EQUAL
# value 3.  at one edge the saddle's candidates are 2 and 4: equal value, equal d2 - both modes take the smaller
# position, 2, and the saddle goes LEFT.  at two edges its candidates are 1, 2, 4, 5: "highest" takes 5 (value 7), the
# saddle goes RIGHT; "nearest" still takes 2
BUMPS_VALUES = [2.0, 5.0, 3.0, 1.0, 3.0, 7.0, 4.0]
BUMPS_LINK_1 = [1, 1, 1, 2, 5, 5, 5]
BUMPS_LABELS_1 = [0, 0, 0, 0, 1, 1, 1]
BUMPS_LINK_2 = {"highest": [1, 1, 1, 5, 5, 5, 5], "nearest": [1, 1, 1, 2, 5, 5, 5]}
BUMPS_LABELS_2 = {"highest": [0, 0, 0, 1, 1, 1, 1], "nearest": [0, 0, 0, 0, 1, 1, 1]}

# "highest" and "nearest" differ: voxel 0 (value 0) at two edges sees 1 (value 1, d2 = e^2) and 2 (value 2, 4 e^2)
DIFFER_VALUES = [0.0, 1.0, 2.0]
DIFFER_LINK = {"highest": [2, 2, 2], "nearest": [1, 2, 2]}


def row_cells(n):
    return [(x, 0, 0) for x in range(n)]


def plateau_cells():
    """an L of equal values in the layer z = 0: the row y = 0, x = 0..4 and the column x = 4, y = 1..4.  positions run
    y, then x: 0..4 the row, 5..8 the column.  at one edge every voxel steps to its neighbor of the smaller position
    and all reach 0; at 2 edges all still do (among equal values the smaller d2: still one cell at a time).  a U - the
    L and a second row y = 4 - is not convex: the far row's smallest position is a peak of its own (u_cells)"""
    return [(x, 0, 0) for x in range(5)] + [(4, y, 0) for y in range(1, 5)]


def u_cells():
    """plateau_cells() with the row y = 4, x = 0..3 in front of its last voxel: positions 0..4 the near row, 5..7 the
    column's middle, 8..11 the far row, 12 the corner (4, 4).  at one edge the far row climbs to position 8 = (0, 4),
    which has no neighbor of a smaller position: a second peak on one plateau.  the corner 12 has (4, 3) = 7 and
    (3, 4) = 11 at equal distance and takes the smaller position, 7: it goes with the near row"""
    return [(x, 0, 0) for x in range(5)] + [(4, y, 0) for y in range(1, 4)] + [(x, 4, 0) for x in range(5)]


U_LABELS = [0] * 8 + [1] * 4 + [0]
U_PEAKS = [0, 8]


def smooth_values(voxels):
    """a sum of four Gaussians of the voxel centres (box-relative): a few peaks per lattice, hardly any exact tie"""
    voxels = np.asarray(voxels, dtype=np.float64)
    lo, hi = voxels.min(axis=0), voxels.max(axis=0)
    t = (voxels - lo) / (hi - lo)
    out = np.zeros(len(voxels))
    for cx, cy, cz, s, a in ((0.2, 0.3, 0.5, 0.15, 1.0), (0.7, 0.6, 0.4, 0.2, 0.8), (0.5, 0.2, 0.8, 0.1, 0.6),
                             (0.9, 0.9, 0.1, 0.12, 0.9)):
        d = (t[:, 0] - cx) ** 2 + (t[:, 1] - cy) ** 2 + (t[:, 2] - cz) ** 2
        out += a * np.exp(-d / (2.0 * s * s))
    return out


def quantised_values(voxels):
    """smooth_values on four levels (0, 1, 2, 3): equal-value ties everywhere, plateaus of every shape"""
    x = smooth_values(voxels)
    return np.floor(4.0 * x / (x.max() * (1.0 + 1e-9))).astype(np.float64)


def case_classes(m, seed=3):
    """three classes and about a quarter of the voxels out of the graph"""
    return np.random.default_rng(seed).integers(-1, 3, m)
