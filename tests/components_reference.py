"""
numpy + scipy reference for NeighborIndex.components and the inputs of its tests (no GPU).

the contract: vertices are the voxels of nearest_reference.voxels_of(cloud, e) by position; u and v are joined when
(dx*dx + dy*dy) + dz*dz <= r*r on their centres, elementwise in fp64 (numpy does not fuse; the limit is inclusive)
and both carry the same class >= 0; scipy.sparse.csgraph.connected_components labels that graph; components are
renumbered by their smallest member, a component's size is the sum of its voxels' weights, components below min_size
are dropped and the others keep their order.  brute force over all pairs, in chunks of rows.
"""

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from nearest_reference import voxels_of  # noqa: F401  (the centres every test starts from)

CHUNK = 256


def edges(voxels, radius):
    """(i, j) int64 arrays, i < j: every pair of voxels within `radius` - the kernel's expression order"""
    voxels = np.asarray(voxels, dtype=np.float64)
    m = len(voxels)
    r2 = float(radius) * float(radius)
    out_i, out_j = [], []
    for lo in range(0, m, CHUNK):
        rows = voxels[lo:lo + CHUNK]
        cols = voxels[lo:]                       # j >= the chunk's first row; j > i is taken below
        dx = rows[:, None, 0] - cols[None, :, 0]
        dy = rows[:, None, 1] - cols[None, :, 1]
        dz = rows[:, None, 2] - cols[None, :, 2]
        i, j = np.nonzero((dx * dx + dy * dy) + dz * dz <= r2)
        upper = j > i
        out_i.append(i[upper] + lo)
        out_j.append(j[upper] + lo)
    if not out_i:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(out_i).astype(np.int64), np.concatenate(out_j).astype(np.int64)


def components_of_edges(m, pairs, voxel_class=None, voxel_weight=None, min_size=1):
    """(labels int64 (m,), sizes int64 (C,), total): `total` counts the components before min_size"""
    i, j = pairs
    cls = np.zeros(m, dtype=np.int64) if voxel_class is None else np.asarray(voxel_class, dtype=np.int64)
    weight = np.ones(m, dtype=np.int64) if voxel_weight is None else np.asarray(voxel_weight, dtype=np.int64)
    assert cls.shape == weight.shape == (m,)
    alive = cls >= 0
    ok = alive[i] & alive[j] & (cls[i] == cls[j])
    graph = coo_matrix((np.ones(int(ok.sum()), dtype=np.int8), (i[ok], j[ok])), shape=(m, m))
    _, raw = connected_components(graph, directed=False)
    labels = np.full(m, -1, dtype=np.int64)
    sizes = []
    total = 0
    seen = {}
    for v in range(m):                           # ascending position: a component is met at its smallest member
        if not alive[v]:
            continue
        c = int(raw[v])
        if c not in seen:
            total += 1
            members = raw == c                   # (removed voxels are alone in theirs: never reached here)
            size = int(weight[members].sum())
            if size >= min_size:
                seen[c] = len(sizes)
                sizes.append(size)
            else:
                seen[c] = -1
        labels[v] = seen[c]
    return labels, np.asarray(sizes, dtype=np.int64), total


def components(voxels, radius, voxel_class=None, voxel_weight=None, min_size=1):
    """(labels, sizes) of the voxel graph at `radius`"""
    return components_of_edges(len(voxels), edges(voxels, radius), voxel_class, voxel_weight, min_size)[:2]


# ---- inputs --------------------------------------------------------------------------------------------------------
EDGE = 0.25


def cells_cloud(cells, edge=EDGE, seed=None):
    """one point inside each integer cell (i, j, k): at its centre, or with a seed somewhere in its middle half"""
    cells = np.asarray(cells, dtype=np.float64)
    at = 0.5 if seed is None else 0.25 + 0.5 * np.random.default_rng(seed).random(cells.shape)
    return np.ascontiguousarray((cells + at) * edge)


def random_lattice_cells():
    """20 000 integer cells drawn uniformly in 96 x 40 x 24: 17 991 distinct ones"""
    return np.random.default_rng(7).integers(0, [96, 40, 24], size=(20000, 3))


def checkerboard_cells(nx=12, ny=10, nz=9):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    return g[(g.sum(axis=1) % 2) == 0]


def block_cells(nx=12, ny=10, nz=9):
    return np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)


def snake_cells(nx=40, ny=40, nz=11):
    """a one-voxel-thick serpentine through an nx x ny x nz box, in PATH order: along x in the rows y = 0, 2, 4, ...
    of the layers z = 0, 2, 4, ..., one cell in the odd row between two rows at alternating ends, one cell in the odd
    layer between two layers, and back.  consecutive cells are face neighbors, all other pairs are at least sqrt(2)
    cells apart: at a radius of one edge the graph IS the path.  40 x 40 x 11: 4919 cells (a path cannot fill a box
    it must not touch itself in: three layers hold 1639), across the superblock borders x = 32, y = 8.., z = 8"""
    path = []
    for z in range(0, nz, 2):
        rows = list(range(0, ny, 2))
        if (z // 2) % 2:
            rows.reverse()
        for n, y in enumerate(rows):
            forward = (len(path) == 0) or path[-1][0] == 0
            xs = range(nx) if forward else range(nx - 1, -1, -1)
            path.extend((x, y, z) for x in xs)
            if n + 1 < len(rows):
                path.append((path[-1][0], (y + rows[n + 1]) // 2, z))
        if z + 2 < nz:
            path.append((path[-1][0], path[-1][1], z + 1))
    return np.asarray(path, dtype=np.int64)


def thin_cells():
    """a long thin lattice, 700 x 6 x 5 cells: runs along x broken by gaps, so that components end and begin inside
    and across the 32-cell superblocks and the 512-cell pieces of a row"""
    rng = np.random.default_rng(23)
    g = block_cells(700, 6, 5)
    return g[rng.random(len(g)) < 0.45]
