"""
numpy reference for NeighborIndex.regions (no GPU), on top of components_reference.edges / components_of_edges and the
border rule of dbscan_reference.

the contract: the graph is that of components() - u ~ v when (dx*dx + dy*dy) + dz*dz <= r*r on their centres and both
carry the same class >= 0.  a voxel of the graph is a seed where voxel_seed says so (None: everywhere).  a graph edge
between two seeds links them when
    normals given:  fabs((nu.x*nv.x + nu.y*nv.y) + nu.z*nv.z) >= min_cos      (elementwise numpy: unfused, this order)
    values given:   fabs(value_u[c] - value_v[c]) <= max_step[c] for every c  (inclusive)
both hold; a comparison with NaN is false.  the regions are the connected components of the seeds under the linked
edges, numbered by their smallest seed; a voxel of the graph that is no seed takes the region of its nearest seed
neighbor, by (d2, position), whatever the two tests say - or -1 when it has none; a region's size is the sum of the
weights of its members; regions below min_size are dropped and the others keep their order.
"""

import math

import numpy as np

import components_reference as cref
import dbscan_reference as dref


def min_cos_of(max_angle):
    """what NeighborIndex.regions makes of max_angle: its cosine, and 0 from a right angle on - the float pi/2 lies
    below the real one and its cosine, 6e-17, would cut normals that are perpendicular exactly"""
    return math.cos(max_angle) if max_angle < math.pi / 2 else 0.0


def seed_edges(m, pairs, voxel_normal=None, min_cos=None, voxel_value=None, max_step=None, voxel_seed=None,
               voxel_class=None):
    """(cls, alive, seed, (i, j) of every class edge, (si, sj) of the seed-seed edges among them, normal_ok, value_ok):
    the two tests on every seed-seed edge, each all True where its table is not given"""
    cls, alive, i, j = dref.class_edges(m, pairs, voxel_class)
    seed = alive.copy() if voxel_seed is None else alive & (np.asarray(voxel_seed).reshape(m) != 0)
    both = seed[i] & seed[j]
    si, sj = i[both], j[both]
    normal_ok = np.ones(len(si), dtype=bool)
    value_ok = np.ones(len(si), dtype=bool)
    with np.errstate(invalid="ignore"):
        if voxel_normal is not None:
            n = np.asarray(voxel_normal, dtype=np.float64)
            assert n.shape == (m, 3)
            nu, nv = n[si], n[sj]
            normal_ok = np.abs((nu[:, 0] * nv[:, 0] + nu[:, 1] * nv[:, 1]) + nu[:, 2] * nv[:, 2]) >= min_cos
        if voxel_value is not None:
            x = np.asarray(voxel_value, dtype=np.float64).reshape(m, -1)
            step = np.broadcast_to(np.asarray(max_step, dtype=np.float64), (x.shape[1],))
            value_ok = (np.abs(x[si] - x[sj]) <= step[None, :]).all(axis=1)
    return cls, alive, seed, (i, j), (si, sj), normal_ok, value_ok


def regions_of_edges(voxels, pairs, voxel_normal=None, min_cos=None, voxel_value=None, max_step=None, voxel_seed=None,
                     voxel_class=None, voxel_weight=None, min_size=1):
    """(labels int64 (m,), sizes int64 (C,), seed bool (m,), total): `pairs` are components_reference.edges(voxels,
    radius); `total` counts the regions before min_size"""
    voxels = np.asarray(voxels, dtype=np.float64)
    m = len(voxels)
    weight = np.ones(m, dtype=np.int64) if voxel_weight is None else np.asarray(voxel_weight, dtype=np.int64)
    assert weight.shape == (m,)
    cls, alive, seed, (i, j), (si, sj), normal_ok, value_ok = seed_edges(
        m, pairs, voxel_normal, min_cos, voxel_value, max_step, voxel_seed, voxel_class)
    link = normal_ok & value_ok
    # the regions of the seeds, every one of them, numbered by smallest (seed) member
    raw, _, total = cref.components_of_edges(m, (si[link], sj[link]), np.where(seed, cls, -1), None, 1)
    # border (as dbscan_reference, the seeds in the place of the core voxels): every (voxel that is no seed, seed
    # neighbor) pair over ALL the class edges, the best per voxel by (d2, position)
    src, dst = np.concatenate((i, j)), np.concatenate((j, i))
    take = alive[src] & ~seed[src] & seed[dst]
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
    return renumber[raw], all_sizes[keep], seed, total


def regions(voxels, radius, **kwargs):
    """(labels, sizes, seed) of the voxel graph at `radius`"""
    return regions_of_edges(voxels, cref.edges(voxels, radius), **kwargs)[:3]


# ---- inputs --------------------------------------------------------------------------------------------------------
EDGE = cref.EDGE

# the roof: a 6 x 4 horizontal plane (z = 3, x = 0..3) and a 6 x 4 wall below its edge (x = 3, z = 0..3) that share the
# ridge row (3, y, 3).  normals (0, 0, 1) on the plane and (1, 0, 0) on the wall; the six ridge voxels are no seeds (and
# carry no normal).  at 1.5 edges a plane seed (2, y, 3) and a wall seed (3, y, 2) are neighbors (sqrt 2), so only the
# normals keep the two faces apart.  positions run z, y, x: the wall's rows z = 0, 1, 2 come first (18 voxels), then
# the layer z = 3 with, per y, three plane seeds and the ridge voxel.  a ridge voxel is one edge from the plane seed
# (2, y, 3) and from the wall seed (3, y, 2): a tie, which goes to the smaller position - the wall's (z = 2).  the
# wall holds the smallest seed (position 0), so it is region 0
ROOF_RADIUS_IN_EDGES = 1.5


def roof_cells(valley=False):
    """the roof; with `valley` the wall stands ON the edge (z = 3..6) and the tie goes to the plane's seed instead"""
    plane = [(x, y, 3) for y in range(6) for x in range(4)]
    wall = [(3, y, z) for z in (range(4, 7) if valley else range(0, 3)) for y in range(6)]
    cells = np.asarray(plane + wall, dtype=np.int64)
    return cells[np.lexsort((cells[:, 0], cells[:, 1], cells[:, 2]))]


def roof_inputs(cells):
    """(normals (m, 3), seed (m,)) of roof_cells() in position order"""
    on_plane = cells[:, 2] == 3
    ridge = on_plane & (cells[:, 0] == 3)
    normal = np.where(on_plane[:, None], (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    normal[ridge] = 0.0
    return normal, ~ridge


ROOF_LABELS = [0] * 18 + [1, 1, 1, 0] * 6               # max_angle 0.5: the ridge goes to the wall
ROOF_SIZES = [24, 18]
VALLEY_LABELS = [0, 0, 0, 0] * 6 + [1] * 18             # the plane comes first and takes the ridge
VALLEY_SIZES = [24, 18]

# the lattices of the GPU tests and their random inputs: per-voxel tables that depend on the voxel's centre alone
def lattice_cloud(name):
    """the cloud the GPU tests build their handle from: one point somewhere in the middle of every cell"""
    cells, seed = {"random": (cref.random_lattice_cells, 41), "thin": (cref.thin_cells, 5)}[name]
    return cref.cells_cloud(cells(), seed=seed)


MAX_ANGLE = 0.35
MAX_STEP = (0.3, 0.25, 0.5, 0.4)
DIRECTIONS = np.array([(0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.6, 0.0, 0.8)])


def case_inputs(voxels, seed=19):
    """(normals (m, 3), values (m, 4), voxel_seed bool (m,), voxel_class (m,)): normals drawn from four directions, one
    per block of 8 x 8 x 8 cells, plus jitter, unit length, 5 % set to zero; four value columns, ramps along the axes
    plus noise; about 70 % seeds; three classes, one per slab of 32 cells along x, and 8 % of the voxels out of the
    graph"""
    voxels = np.asarray(voxels, dtype=np.float64)
    m = len(voxels)
    rng = np.random.default_rng(seed)
    block = np.floor(voxels / (8.0 * EDGE)).astype(np.int64)
    normal = DIRECTIONS[(block[:, 0] + 2 * block[:, 1] + 3 * block[:, 2]) % 4] + rng.normal(0.0, 0.1, (m, 3))
    normal /= np.sqrt((normal * normal).sum(axis=1))[:, None]
    normal[rng.random(m) < 0.05] = 0.0
    value = np.column_stack((voxels[:, 0], voxels[:, 1], voxels[:, 2], voxels.sum(axis=1))) * 0.5
    value = value + rng.normal(0.0, 0.12, (m, 4))
    voxel_seed = rng.random(m) < 0.7
    voxel_class = np.where(rng.random(m) < 0.08, -1, (block[:, 0] // 4) % 3)
    return np.ascontiguousarray(normal), np.ascontiguousarray(value), voxel_seed, voxel_class


# (normal, value columns) per mode: every instance of the link kernel - <NORMAL, DIMS> with DIMS 0..4 - but <false, 0>,
# which the identities reach
MODES = {"normal": (True, 0), "value1": (False, 1), "value2": (False, 2), "value3": (False, 3), "value4": (False, 4),
         "both1": (True, 1), "both2": (True, 2), "both3": (True, 3), "both4": (True, 4)}


def mode_arguments(mode, normal, value):
    """the keyword arguments of regions_of_edges for a mode (min_cos form)"""
    with_normal, dims = MODES[mode]
    out = {}
    if with_normal:
        out.update(voxel_normal=normal, min_cos=min_cos_of(MAX_ANGLE))
    if dims:
        out.update(voxel_value=value[:, :dims], max_step=np.asarray(MAX_STEP[:dims]))
    return out
