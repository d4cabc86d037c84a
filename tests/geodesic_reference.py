"""
numpy reference for NeighborIndex.geodesic (no GPU), on the pairs of components_reference.edges, and the cases the CPU
and GPU tests share.

the contract: the graph is that of components() - u ~ v when (dx*dx + dy*dy) + dz*dz <= r*r on their centres and both
carry the same class >= 0.  an edge weighs w = np.sqrt of that same d2 (IEEE: correctly rounded).  a voxel of the graph
with a non-zero seed entry is at distance 0; dist is the least fixpoint of dist[v] = min over neighbors u of
fl(dist[u] + w(u, v)), everything else starting at +inf, a candidate above max_distance not taken.  the reference
relaxes ALL edges at once from the values of the sweep before (Jacobi) until nothing changes: the kernel relaxes in
place, in whatever order its lanes run - the fixpoint is the same, which the GPU tests show.
u is LOWER than v when dist[u] < dist[v] or (dist[u] == dist[v] and u < v).  for a reached voxel v that is no seed the
candidates are the neighbors u with fl(dist[u] + w) == dist[v] that are lower than v; link[v] is the one of the smallest
dist[u], then of the smallest position; v itself at a seed; -1 where v is unreached, out of the graph, or has no
candidate (an ORPHAN: only a dist short of the fixpoint has one).  a segment is what the links lead to one seed;
whatever leads to an orphan is in none.  segments are numbered by ascending seed position, a segment's size is the sum
of its members' weights, segments below min_size are dropped and the others keep their order.
"""

import numpy as np

import components_reference as cref

EDGE = cref.EDGE
INF = float("inf")


def directed_edges(voxels, pairs, voxel_class=None):
    """(src, dst, w): both directions of every pair whose ends share a class >= 0, ordered by (dst, src), and
    their lengths"""
    voxels = np.asarray(voxels, dtype=np.float64)
    m = len(voxels)
    i, j = pairs
    cls = np.zeros(m, dtype=np.int64) if voxel_class is None else np.asarray(voxel_class, dtype=np.int64)
    assert cls.shape == (m,)
    ok = (cls[i] >= 0) & (cls[i] == cls[j])
    i, j = i[ok], j[ok]
    src, dst = np.concatenate((i, j)), np.concatenate((j, i))
    order = np.lexsort((src, dst))
    src, dst = src[order], dst[order]
    dx = voxels[dst, 0] - voxels[src, 0]
    dy = voxels[dst, 1] - voxels[src, 1]
    dz = voxels[dst, 2] - voxels[src, 2]
    return src, dst, np.sqrt((dx * dx + dy * dy) + dz * dz)


def start(m, voxel_seed, voxel_class=None):
    """dist before the first sweep: 0 at the seeds of the graph, +inf elsewhere"""
    seed = np.asarray(voxel_seed) != 0
    assert seed.shape == (m,)
    if voxel_class is not None:
        seed = seed & (np.asarray(voxel_class) >= 0)
    return np.where(seed, 0.0, INF)


def sweep(dist, edges, max_distance=INF):
    """one Jacobi sweep: (the new dist, how many voxels it lowered)"""
    src, dst, w = edges
    new = dist.copy()
    if len(src):
        through = dist[src] + w
        through[~(through <= max_distance)] = INF
        heads = np.nonzero(np.diff(dst, prepend=-1))[0]          # (dst is sorted)
        at = dst[heads]
        new[at] = np.minimum(new[at], np.minimum.reduceat(through, heads))
    return new, int((new < dist).sum())


def distances(m, edges, voxel_seed, voxel_class=None, max_distance=INF):
    """(dist fp64 (m,), sweeps): relaxation to the fixpoint; `sweeps` counts the sweeps that lowered something"""
    dist = start(m, voxel_seed, voxel_class)
    sweeps = 0
    while True:
        dist, lowered = sweep(dist, edges, max_distance)
        if not lowered:
            return dist, sweeps
        sweeps += 1
        assert sweeps <= m, "no fixpoint after M sweeps"


def links(dist, edges, voxel_class=None):
    """(link int64 (m,), orphans): the rule of the contract on ANY dist (at the fixpoint there is no orphan)"""
    m = len(dist)
    src, dst, w = edges
    cls = np.zeros(m, dtype=np.int64) if voxel_class is None else np.asarray(voxel_class, dtype=np.int64)
    inside = (cls >= 0) & (dist < INF)
    link = np.full(m, -1, dtype=np.int64)
    is_seed = inside & (dist == 0.0)
    link[is_seed] = np.nonzero(is_seed)[0]
    du, dv = dist[src], dist[dst]
    lower = (du < dv) | ((du == dv) & (src < dst))
    ok = inside[dst] & ~is_seed[dst] & lower & (du + w == dv)
    s, d, du = src[ok], dst[ok], du[ok]
    order = np.lexsort((s, du, d))                               # per voxel: smallest dist[u], then smallest u
    s, d = s[order], d[order]
    heads = np.nonzero(np.diff(d, prepend=-1))[0]
    link[d[heads]] = s[heads]
    orphans = int((inside & (link < 0)).sum())
    return link, orphans


def roots_of_links(link):
    """root int64 (m,): the voxel every chain of links ends in - a seed, or the last voxel before a link of -1 (an
    orphan); -1 where the voxel itself has no link"""
    m = len(link)
    at = np.where(link >= 0, link, np.arange(m))
    steps = 0
    while True:
        nxt = np.where(link[at] >= 0, link[at], at)
        if np.array_equal(nxt, at):
            break
        at = nxt
        steps += 1
        assert steps <= m, "a cycle in the links"
    return np.where(link >= 0, at, -1)


def segments(dist, link, voxel_weight=None, min_size=1):
    """(labels int64 (m,), sizes int64 (C,), sources int64 (C,), total): `total` counts the seeds in the graph"""
    m = len(link)
    weight = np.ones(m, dtype=np.int64) if voxel_weight is None else np.asarray(voxel_weight, dtype=np.int64)
    assert weight.shape == (m,)
    root = roots_of_links(link)
    labels = np.full(m, -1, dtype=np.int64)
    sizes, sources = [], []
    seeds = np.nonzero(link == np.arange(m))[0]
    for v in seeds:                              # ascending position
        members = root == v
        size = int(weight[members].sum())
        if size >= min_size:
            labels[members] = len(sizes)
            sizes.append(size)
            sources.append(v)
    return labels, np.asarray(sizes, dtype=np.int64), np.asarray(sources, dtype=np.int64), len(seeds)


def geodesic_of_edges(voxels, pairs, voxel_seed, max_distance=None, voxel_class=None, voxel_weight=None, min_size=1):
    """(dist, labels, sizes, sources, link, total, sweeps): `pairs` are components_reference.edges(voxels, radius)"""
    m = len(voxels)
    edges = directed_edges(voxels, pairs, voxel_class)
    limit = INF if max_distance is None else float(max_distance)
    dist, sweeps = distances(m, edges, voxel_seed, voxel_class, limit)
    link, orphans = links(dist, edges, voxel_class)
    assert orphans == 0
    labels, sizes, sources, total = segments(dist, link, voxel_weight, min_size)
    return dist, labels, sizes, sources, link, total, sweeps


def geodesic(voxels, radius, voxel_seed, **kwargs):
    """(dist, labels, sizes, sources, link) of the voxel graph at `radius`"""
    return geodesic_of_edges(voxels, cref.edges(voxels, radius), voxel_seed, **kwargs)[:5]


def bits(x):
    """fp64 as its int64 bit pattern: +inf, -0 and every last bit count in a comparison"""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# ---- inputs --------------------------------------------------------------------------------------------------------

def centres(cells, edge=EDGE):
    """the voxel centres of integer cells listed in position order (z, then y, then x ascending)"""
    return (np.asarray(cells, dtype=np.float64) + 0.5) * edge


def in_position_order(cells):
    return sorted(cells, key=lambda c: (c[2], c[1], c[0]))


def row_cells(n):
    return [(x, 0, 0) for x in range(n)]


def horseshoe_cells():
    """a U in the layer z = 0 whose tips (0, 0) and (2, 0) are two cells apart.  positions: 0, 1 the tips, 2, 3 the
    arms' middles (0, 1) and (2, 1), 4, 5, 6 the bend (0, 2), (1, 2), (2, 2).  at one edge the way from tip to tip is
    the six steps round the bend; at two edges the gap is one step"""
    return in_position_order([(0, 0, 0), (0, 1, 0), (0, 2, 0), (1, 2, 0), (2, 2, 0), (2, 1, 0), (2, 0, 0)])


HORSESHOE_LINK_1 = [0, 3, 0, 6, 2, 4, 5]
# at two edges, in edges: the tip (2, 0), (0, 1) and (0, 2) straight from the seed at 2, 1 and 2; (1, 2) over (0, 1) at
# 1 + sqrt(2); (2, 1) at 3 over the tip (2 + 1) or over (0, 1) (1 + 2) - the candidate of the smaller distance, (0, 1);
# (2, 2) over (1, 2) at 2 + sqrt(2), which beats the three ways of length 4
HORSESHOE_LINK_2 = [0, 0, 0, 2, 0, 2, 5]


def staircase_cells():
    """steps in the layer z = 0: (0, 0), (1, 0), (1, 1), (2, 1), (2, 2) are positions 0..4.  at 1.5 edges the diagonal
    (0, 0) - (1, 1) of sqrt(2) edges beats the two straight steps through (1, 0).  (2, 1) is 1 + sqrt(2) over (1, 0)
    and sqrt(2) + 1 over (1, 1): the same number bit for bit (addition commutes), so the candidate of the smaller
    distance, (1, 0), is its link.  (2, 2) is two diagonals from the seed"""
    return [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0), (2, 2, 0)]


STAIRCASE_LINK = [0, 0, 0, 1, 2]


def serpentine_cells(nx=40, ny=99):
    """cref.snake_cells in one layer: rows of nx cells at y = 0, 2, 4, ... joined at alternating ends, in PATH order.
    40 x 99: 2049 cells; at one edge the graph is the path"""
    return cref.snake_cells(nx, ny, 1)


def case_seeds(m, count, seed=29):
    """`count` seed voxels drawn without replacement, as a bool array"""
    out = np.zeros(m, dtype=bool)
    out[np.random.default_rng(seed + count).choice(m, size=count, replace=False)] = True
    return out


def median_distance(dist):
    """the upper median of the finite distances: a distance some voxel HAS, so a limit there is met exactly"""
    finite = np.sort(dist[dist < INF])
    return float(finite[len(finite) // 2])


def case_classes(m, seed=13):
    """two classes and about a fifth of the voxels out of the graph"""
    return np.random.default_rng(seed).choice(np.array([-1, 0, 0, 1, 1]), size=m)


# the lattice cases of the CPU and GPU tests: (radius in edges, seeds, two classes, max_distance at the median of the
# finite distances of the same case without a limit)
LATTICE_CASES = [(rho, seeds, False, False) for rho in (1.0, 2.0, 3.0) for seeds in (1, 7, 200)] + \
                [(rho, 7, True, False) for rho in (1.0, 2.0, 3.0)] + \
                [(1.0, 200, False, True), (2.0, 7, False, True), (3.0, 1, False, True), (2.0, 200, True, True)]
