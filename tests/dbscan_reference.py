"""
numpy reference for NeighborIndex.dbscan (no GPU), on top of components_reference.edges / components_of_edges.

the contract: the graph is that of components() - u ~ v when (dx*dx + dy*dy) + dz*dz <= r*r on their centres and both
carry the same class >= 0.  density[v] = weight[v] + the weights of v's neighbors (int64; 0 outside the graph);
core[v] = density[v] >= min_weight; the clusters are the connected components of the graph restricted to core voxels,
numbered by their smallest core member; a voxel of the graph that is not core takes the cluster of its nearest core
neighbor, by (d2, position) - border - or -1 when it has none - noise; a cluster's size is the sum of the weights of
its members, core and border; clusters below min_size are dropped and the others keep their order.
test_dbscan_cpu.py pins this to sklearn.cluster.DBSCAN with sample_weight.
"""

import numpy as np

import components_reference as cref


def class_edges(m, pairs, voxel_class):
    """(cls, alive, i, j): the pairs whose two ends carry the same class >= 0"""
    i, j = pairs
    cls = np.zeros(m, dtype=np.int64) if voxel_class is None else np.asarray(voxel_class, dtype=np.int64)
    assert cls.shape == (m,)
    alive = cls >= 0
    ok = alive[i] & alive[j] & (cls[i] == cls[j])
    return cls, alive, i[ok], j[ok]


def dbscan_of_edges(voxels, pairs, min_weight, voxel_weight=None, voxel_class=None, min_size=1):
    """(labels int64 (m,), sizes int64 (C,), core bool (m,), density int64 (m,), total): `pairs` are
    components_reference.edges(voxels, radius); `total` counts the clusters before min_size"""
    voxels = np.asarray(voxels, dtype=np.float64)
    m = len(voxels)
    weight = np.ones(m, dtype=np.int64) if voxel_weight is None else np.asarray(voxel_weight, dtype=np.int64)
    assert weight.shape == (m,) and (weight >= 0).all()
    cls, alive, i, j = class_edges(m, pairs, voxel_class)
    density = np.where(alive, weight, 0)
    np.add.at(density, i, weight[j])
    np.add.at(density, j, weight[i])
    core = alive & (density >= min_weight)
    # the core clusters, every one of them, numbered by smallest (core) member
    raw, _, total = cref.components_of_edges(m, (i, j), np.where(core, cls, -1), None, 1)
    # border: every (voxel that is not core, core neighbor) pair, the best per voxel by (d2, position)
    src, dst = np.concatenate((i, j)), np.concatenate((j, i))
    take = alive[src] & ~core[src] & core[dst]
    src, dst = src[take], dst[take]
    d = voxels[src] - voxels[dst]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    order = np.lexsort((dst, d2, src))
    src, dst = src[order], dst[order]
    first = np.ones(len(src), dtype=bool)
    first[1:] = src[1:] != src[:-1]
    raw = raw.copy()
    raw[src[first]] = raw[dst[first]]
    # sizes, then min_size
    member = raw >= 0
    all_sizes = np.zeros(total, dtype=np.int64)
    np.add.at(all_sizes, raw[member], weight[member])
    keep = all_sizes >= min_size
    renumber = np.full(total + 1, -1, dtype=np.int64)            # (the last entry serves the label -1)
    renumber[:total][keep] = np.arange(int(keep.sum()))
    return renumber[raw], all_sizes[keep], core, density, total


def dbscan(voxels, radius, min_weight, voxel_weight=None, voxel_class=None, min_size=1):
    """(labels, sizes, core, density) of the voxel graph at `radius`"""
    return dbscan_of_edges(voxels, cref.edges(voxels, radius), min_weight, voxel_weight, voxel_class, min_size)[:4]


# ---- inputs --------------------------------------------------------------------------------------------------------
EDGE = cref.EDGE

# (lattice, radius in edges, min_weight) of the sklearn comparison and of the GPU tests; weights: case_weights(M).
# 1.5 and 2.2 lie between the square roots of two integers, so no pair of cell centres sits at the limit; at 1.0 face
# neighbors do, and the dyadic centres of the CPU test (E = 1/4) reach it exactly in every arithmetic
CASES = (("random", 1.0, 4), ("random", 1.5, 12), ("random", 2.2, 40), ("random", 2.2, 60), ("thin", 2.2, 40))


def lattice_cells(name):
    return {"random": cref.random_lattice_cells, "thin": cref.thin_cells}[name]()


def case_weights(m):
    return np.random.default_rng(3).integers(1, 6, m)


def bridge_cells():
    """two filled 6 x 6 x 6 blocks, 10 cells apart along x, joined by a one-voxel-thick bridge of 10 cells"""
    a = cref.block_cells(6, 6, 6)
    b = a + np.array([16, 0, 0])
    bridge = np.array([(x, 2, 2) for x in range(6, 16)])
    return np.concatenate((a, bridge, b))


# a voxel (2, 1) that is not core between two clusters, one cell from a core voxel of each: (2, 0), the smaller
# position, belongs to the cluster with the LARGER number (the other cluster starts at (0, 0)).  the last voxel, three
# layers up and out of everybody's reach, gives the cloud an extent along z; it is noise
TIE_CELLS = np.array([(0, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (0, 1, 0), (2, 1, 0), (0, 2, 0), (1, 2, 0), (2, 2, 0),
                      (0, 0, 3)])
TIE_WEIGHTS = np.array([5, 3, 5, 5, 5, 0, 5, 5, 3, 1])
TIE_MIN_WEIGHT = 7
TIE_LABELS = [0, 1, 1, 1, 0, 1, 0, 0, 0, -1]
TIE_SIZES = [23, 13]
TIE_DENSITY = [10, 8, 13, 10, 15, 6, 15, 13, 8, 1]
