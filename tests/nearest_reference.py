"""
brute-force numpy reference for NeighborIndex.nearest and the inputs of its tests (no GPU, no scipy).

the contract: candidates are the voxels of oracle.Lattice(cloud, e).unique_voxels(cloud); a voxel's squared distance
is (dx*dx + dy*dy) + dz*dz, elementwise in fp64 (numpy does not fuse); rows are ordered by (d2, voxel index) with
np.lexsort; a voxel qualifies when d2 <= lim*lim; unused slots hold inf / -1.
"""

import numpy as np

from oracle import nimrud_oracle as oracle


def voxels_of(cloud, edge):
    return oracle.Lattice(cloud, edge).unique_voxels(cloud)


def all_d2(voxels, query):
    """(Nq, M) squared distances, the kernel's operation order"""
    dx = query[:, None, 0] - voxels[None, :, 0]
    dy = query[:, None, 1] - voxels[None, :, 1]
    dz = query[:, None, 2] - voxels[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest(voxels, query, k, max_distance=None, d2=None):
    """(d2 fp64 (Nq, k), index int64 (Nq, k), found int64 (Nq,)).  d2: all_d2(voxels, query) when the caller has it"""
    query = np.asarray(query, dtype=np.float64)
    nq, m = len(query), len(voxels)
    out_d = np.full((nq, k), np.inf)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    found = np.zeros(nq, dtype=np.int64)
    if nq == 0:
        return out_d, out_i, found
    if d2 is None:
        d2 = all_d2(voxels, query)
    index = np.arange(m)
    for q in range(nq):
        row = d2[q]
        order = np.lexsort((index, row))
        if max_distance is not None:
            order = order[row[order] <= max_distance * max_distance]
        order = order[:k]
        found[q] = len(order)
        out_d[q, :len(order)] = row[order]
        out_i[q, :len(order)] = order
    return out_d, out_i, found


# ---- inputs --------------------------------------------------------------------------------------------------------
SCENE_EDGE = 0.25
ISLAND_EDGE = 0.25
ISLAND_SEED = 11


def scene_cloud():
    """a plane, a pole and a blob: 3000 points, 884 voxels at e = 0.25; queries = every third point plus 300 uniform
    points of a box that reaches beyond the lattice"""
    rs = np.random.RandomState(5)
    plane = np.column_stack((rs.rand(1800, 2) * 6.0, rs.normal(0.0, 0.01, 1800)))
    pole = np.column_stack((3.0 + rs.normal(0.0, 0.01, (400, 2)), rs.rand(400) * 4.0))
    blob = rs.normal((1.5, 4.5, 2.0), 0.4, (800, 3))
    cloud = np.ascontiguousarray(np.vstack((plane, pole, blob)))
    box = rs.rand(300, 3) * np.array([8.0, 8.0, 6.0]) - 1.0
    query = np.ascontiguousarray(np.vstack((cloud[::3], box)))
    return cloud, query


def island_cloud():
    """sites of the 6^3 grid times 0.25, each kept with probability 0.6: at e = 0.25 every point is a cell centre
    and every squared distance is exact, so rows are full of exact ties"""
    rs = np.random.RandomState(ISLAND_SEED)
    g = np.arange(6, dtype=np.float64) * 0.25
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(sites[rs.rand(len(sites)) < 0.6])


def far_cloud():
    """two clusters 25 apart at e = 0.1 (a lattice of 256 cells a side): their points, 64 points between them and
    four well outside the lattice as queries"""
    rs = np.random.RandomState(17)
    a = rs.rand(50, 3) * 0.5
    b = rs.rand(50, 3) * 0.5 + 25.0
    cloud = np.ascontiguousarray(np.vstack((a, b)))
    t = (np.arange(64) + 0.5) / 64.0
    between = t[:, None] * np.array([25.5, 25.5, 25.5]) + rs.normal(0.0, 0.05, (64, 3))
    outside = np.array([[-30.0, 12.0, 40.0], [60.0, 60.0, 60.0], [12.0, -45.0, 3.0], [26.0, 24.0, -33.0]])
    query = np.ascontiguousarray(np.vstack((cloud, between, outside)))
    return cloud, query


def sparse_box():
    """400 points in [0, 20]^3 at e = 0.25 and 2000 queries of the same box: k-th neighbors from under one cell to
    tens of cells away"""
    rs = np.random.RandomState(29)
    return rs.rand(400, 3) * 20.0, rs.rand(2000, 3) * 20.0
