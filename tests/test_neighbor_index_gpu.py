"""
GPU tests of the neighbor index (nm_neighbors.hip, multiscale.NeighborIndex): lists read off the dense occupancy
index and its rank table must equal, element for element, the reference's captured lists, the oracle's, and the
address search they replace.  every comparison is np.array_equal: there is no tolerance in this feature.
"""

import ctypes

import numpy as np
import pytest
import torch

from nimrud_amd import _ffi
from nimrud_amd import device as _device
from nimrud_amd.minimal import multiscale
from nimrud_amd.utils import geometry
from oracle import nimrud_oracle as oracle

pytestmark = pytest.mark.gpu

PIPELINE_FIXTURES = ["g1_uniform.npz", "g2_scene.npz", "g3_offset.npz", "g4_lattice.npz"]
SCAN_TILE = 4096          # entries of the rank scan one block takes per round (NBR_SCAN_TILE, nm_neighbors.hip)
SCAN_MAX_BLOCKS = 2048    # its largest grid (NBR_SCAN_MAX_BLOCKS): more tiles than that and a block loops
CHUNK_LOG2 = 4            # leaves of a lattice row one wave walks (NBR_CHUNK_LOG2)


def superblock_bits(widths):
    return [max(int(widths[0]) - 5, 0), max(int(widths[1]) - 3, 0), max(int(widths[2]) - 3, 0)]


def scan_entries(widths):
    """entries of the rank table's scan for a lattice: 64 rows per (sbz, sby) strip and piece of 16 leaves"""
    bx, by, bz = superblock_bits(widths)
    return 64 << (bz + by + max(bx - CHUNK_LOG2, 0))


def uniform_box(n, extent, seed, origin=(0.0, 0.0, 0.0)):
    rs = np.random.RandomState(seed)
    return rs.rand(n, 3) * np.asarray(extent, dtype=np.float64) + np.asarray(origin, dtype=np.float64)


def unique_addresses(pts, edge):
    return np.unique(oracle.Lattice(pts, edge).coordinate_to_address(pts))


class CIndex(object):
    """the four C entry points on a hand-made lattice"""

    def __init__(self, search, lat):
        self.rt = _device.get_runtime()
        rt = self.rt
        self.lat = lat
        self.search = torch.from_numpy(np.ascontiguousarray(search, dtype=np.float64)).to(rt.device)
        ns = self.search.shape[0]
        nbytes = rt.lib.nm_neighbor_index_workspace_bytes(ns, ctypes.byref(lat))
        assert nbytes > 0
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=rt.device)
        count = torch.full((2,), -1, dtype=torch.int64, device=rt.device)
        rt.check(rt.lib.nm_neighbor_index_build(rt.ctx, _device.ptr(self.search), ns, 3, ctypes.byref(lat),
                                                _device.ptr(count), _device.ptr(self.work), nbytes, rt.stream()))
        self.m, self.outside = (int(v) for v in count.cpu())
        self.ns = ns

    def addresses(self):
        rt = self.rt
        out = torch.full((max(self.ns, 1),), -1, dtype=torch.int64, device=rt.device)
        rt.check(rt.lib.nm_neighbor_index_addresses(rt.ctx, ctypes.byref(self.lat), _device.ptr(self.work),
                                                    self.work.numel(), _device.ptr(out), rt.stream()))
        out = out.cpu().numpy()
        assert np.all(out[self.m:] == -1)           # nothing behind the M-th entry is touched
        return out[:self.m]

    def lists(self, query, radius):
        rt = self.rt
        q = torch.from_numpy(np.ascontiguousarray(query, dtype=np.float64).reshape(-1, 3)).to(rt.device)
        nq = q.shape[0]
        counts = torch.zeros(max(nq, 1), dtype=torch.int32, device=rt.device)
        args = (rt.ctx, _device.ptr(q) if nq else ctypes.c_void_p(0), nq, 3, ctypes.byref(self.lat), float(radius),
                _device.ptr(self.work), self.work.numel())
        rt.check(rt.lib.nm_neighbor_index_lists(*args, _device.ptr(counts), None, None, rt.stream()))
        offsets = np.concatenate(([0], np.cumsum(counts.cpu().numpy()[:nq].astype(np.int64))))
        index = torch.full((max(int(offsets[-1]), 1),), -1, dtype=torch.int64, device=rt.device)
        d_offsets = torch.from_numpy(offsets).to(rt.device)
        rt.check(rt.lib.nm_neighbor_index_lists(*args, None, _device.ptr(d_offsets), _device.ptr(index),
                                                rt.stream()))
        return offsets, index.cpu().numpy()[:int(offsets[-1])]


def brute_lists(query, lat, cells, radius):
    """the predicate spelled out, on the centres of `cells` (sorted by address) of a hand-made lattice"""
    mc = np.array(list(lat.min_corner))
    centres = cells * lat.edge + mc + lat.edge * 0.5
    return oracle.neighbors_to_csr(oracle.ball_neighbors_bruteforce(np.asarray(query).reshape(-1, 3), centres, radius))


# ---- goldens captured from the reference ------------------------------------------------------------------

@pytest.mark.parametrize("name", PIPELINE_FIXTURES)
def test_golden_lists_and_addresses_from_the_index(golden, name):
    g = golden(name)
    pts = g["points"]
    for s, (e, r) in enumerate(zip(g["edges"], g["radii"])):
        want_off, want_idx = g["s%d_nbr_offsets" % s], g["s%d_nbr_index" % s]
        n = len(want_off) - 1
        ix = multiscale.NeighborIndex(pts, e)
        assert ix.method == "index"
        off, idx = ix.lists(pts[:n], r)
        assert np.array_equal(off, want_off)
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(ix.addresses(), g["s%d_addresses" % s])
        assert ix.n_voxels == len(g["s%d_addresses" % s])
        assert np.array_equal(ix.voxels(), oracle.Lattice(pts, e).unique_voxels(pts))


# ---- leaf order, word order and address order all differ ---------------------------------------------------

@pytest.fixture(scope="module")
def permuted():
    """20 000 points, e = 1, in a 100 x 40 x 20 box: 128 x 64 x 32 cells, 4 x 8 x 4 superblocks, three widths"""
    pts = uniform_box(20000, (100.0, 40.0, 20.0), seed=11)
    ix = multiscale.NeighborIndex(pts, 1.0)
    return pts, ix


def test_permuted_order_addresses(permuted):
    pts, ix = permuted
    widths = [int(w) for w in ix.filter.widths]
    bx, by, bz = superblock_bits(widths)
    assert bx >= 1 and by >= 1 and bz >= 1 and len(set(widths)) == 3
    assert ix.method == "index"
    want = unique_addresses(pts, 1.0)
    assert ix.n_voxels == len(want)
    assert np.array_equal(ix.addresses(), want)
    assert np.array_equal(ix.voxels(), oracle.Lattice(pts, 1.0).unique_voxels(pts))


@pytest.mark.parametrize("ratio", [1.0, 2.0, 3.0, 4.0, 5.0, 0.75])       # W = 3, 5, 7, 9, 11 and a generic ratio
def test_permuted_order_lists(permuted, ratio):
    pts, ix = permuted
    query = pts[:4000]
    off, idx = ix.lists(query, ratio)
    want_off, want_idx = oracle.neighbor_lists_c(query, pts, 1.0, ratio)
    assert np.array_equal(off, want_off)
    assert np.array_equal(idx, want_idx)


# ---- the device-wide scan: several blocks, rows cut in pieces, blocks that loop -------------------------------

def test_scan_across_blocks_and_row_pieces():
    """3 x 10^5 points on 1024 x 64 x 128 cells: rows of 32 leaves are cut in two pieces and the scan has
    16 384 entries - four blocks - with M far beyond what one of them covers"""
    pts = uniform_box(300000, (1000.0, 60.0, 120.0), seed=12)
    ix = multiscale.NeighborIndex(pts, 1.0)
    widths = [int(w) for w in ix.filter.widths]
    assert widths == [10, 6, 7] and ix.method == "index"
    assert scan_entries(widths) >= 4 * SCAN_TILE
    want = unique_addresses(pts, 1.0)
    assert ix.n_voxels == len(want) > 4 * SCAN_TILE
    assert np.array_equal(ix.addresses(), want)
    query = pts[:3000]
    off, idx = ix.lists(query, 2.0)
    want_off, want_idx = oracle.neighbor_lists_c(query, pts, 1.0, 2.0)
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)


def test_scan_blocks_that_loop_on_a_lattice_one_leaf_wide():
    """32 x 4096 x 4096 cells: no superblock bits in x, 2^18 superblocks, 2^24 scan entries - more tiles than the
    scan has blocks, so every block takes two"""
    pts = uniform_box(6000, (30.0, 4000.0, 4000.0), seed=13)
    pts[:3000, 1:] = pts[:3000, 1:] % 40.0             # a dense corner: real neighborhoods
    ix = multiscale.NeighborIndex(pts, 1.0)
    widths = [int(w) for w in ix.filter.widths]
    assert widths == [5, 12, 12] and ix.method == "index"
    assert scan_entries(widths) == 2 * SCAN_MAX_BLOCKS * SCAN_TILE
    assert np.array_equal(ix.addresses(), unique_addresses(pts, 1.0))
    off, idx = ix.lists(pts[:4000], 2.0)
    want_off, want_idx = oracle.neighbor_lists_c(pts[:4000], pts, 1.0, 2.0)
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)
    assert idx.shape[0] > 6000


def test_long_thin_lattice_inside_the_range():
    """2^20 x 8 x 8 cells: one (sbz, sby) strip of 2^15 leaves, cut into 2^11 pieces"""
    pts = uniform_box(5000, (1.0e6, 6.0, 6.0), seed=14)
    pts[:2500, 0] = pts[:2500, 0] % 300.0              # a dense end, so that the lists are not all singletons
    ix = multiscale.NeighborIndex(pts, 1.0)
    widths = [int(w) for w in ix.filter.widths]
    assert widths == [20, 3, 3] and ix.method == "index"
    assert np.array_equal(ix.addresses(), unique_addresses(pts, 1.0))
    off, idx = ix.lists(pts, 3.0)
    want_off, want_idx = oracle.neighbor_lists_c(pts, pts, 1.0, 3.0)
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)
    assert idx.shape[0] > 3 * len(pts)


# ---- small and edge lattices ---------------------------------------------------------------------------------

def test_lattice_narrower_than_one_leaf():
    pts = uniform_box(300, (10.0, 5.0, 5.0), seed=15)
    ix = multiscale.NeighborIndex(pts, 1.0)
    widths = [int(w) for w in ix.filter.widths]
    assert widths[0] < 5 and superblock_bits(widths) == [0, 0, 0] and ix.method == "index"
    assert np.array_equal(ix.addresses(), unique_addresses(pts, 1.0))
    for r in (1.0, 2.5):
        off, idx = ix.lists(pts, r)
        want_off, want_idx = oracle.neighbor_lists_c(pts, pts, 1.0, r)
        assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)


def test_one_search_point_and_no_query_points():
    lat = geometry.make_nm_lattice([0.0, 0.0, 0.0], 1.0, [6, 4, 4])
    cell = np.array([[37, 9, 14]])
    ci = CIndex(cell + 0.25, lat)
    assert (ci.m, ci.outside) == (1, 0)
    assert np.array_equal(ci.addresses(), [37 + (9 << 6) + (14 << 10)])
    query = cell + 0.5 + np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 0.1, 0.0], [-40.0, 0.0, 0.0]])
    off, idx = ci.lists(query, 2.0)
    assert np.array_equal(off, [0, 1, 2, 2, 2]) and np.array_equal(idx, [0, 0])
    # no query points: NM_OK, nothing written
    off, idx = ci.lists(np.zeros((0, 3)), 2.0)
    assert np.array_equal(off, [0]) and idx.shape[0] == 0
    # no search points: NM_OK, M = 0, empty lists
    empty = CIndex(np.zeros((0, 3)), lat)
    assert (empty.m, empty.outside) == (0, 0)
    off, idx = empty.lists(query, 2.0)
    assert np.array_equal(off, [0, 0, 0, 0, 0]) and idx.shape[0] == 0
    # and through the handle
    pts = uniform_box(500, (20.0, 20.0, 20.0), seed=16)
    off, idx = multiscale.NeighborIndex(pts, 1.0).lists(np.zeros((0, 3)), 2.0)
    assert off.dtype == np.int64 and np.array_equal(off, [0]) and idx.shape == (0,)


def test_query_cloud_partly_outside_on_every_side_and_leading_rows():
    pts = uniform_box(8000, (40.0, 30.0, 20.0), seed=17)
    ix = multiscale.NeighborIndex(pts, 1.0)
    voxels = oracle.Lattice(pts, 1.0).unique_voxels(pts)
    # clamped home cells and clipped windows: a query cloud that overhangs the search lattice by 4 edges all round
    query = uniform_box(3000, (48.0, 38.0, 28.0), seed=18, origin=(-4.0, -4.0, -4.0))
    lo, hi = pts.min(0), pts.max(0)
    for a in range(3):
        assert (query[:, a] < lo[a] - 1.0).any() and (query[:, a] > hi[a] + 1.0).any()
    query = np.vstack((query, [[-1e6, 15.0, 10.0], [1e150, 15.0, 10.0], [20.0, -1e12, 1e12]]))
    off, idx = ix.lists(query, 3.0)
    want_off, want_idx = oracle.neighbors_to_csr(oracle.ball_neighbors_kdtree(query, voxels, 3.0))
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)
    # the leading rows of the search cloud, as a view of the tensor the index was built from
    dev = torch.from_numpy(pts).cuda()
    ixd = multiscale.NeighborIndex(dev, 1.0)
    off, idx = ixd.lists(dev[:1500], 2.0)
    assert isinstance(off, torch.Tensor) and isinstance(ixd.addresses(), torch.Tensor)
    want_off, want_idx = oracle.neighbor_lists_c(pts[:1500], pts, 1.0, 2.0)
    assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(idx.cpu().numpy(), want_idx)


def test_inclusive_boundary_on_a_lattice_aligned_cloud():
    """points at half-integers, e = 1, r = 3: voxel centres ARE the points, candidates sit at exactly r"""
    rs = np.random.RandomState(19)
    cells = np.unique(rs.randint(0, [40, 20, 12], size=(4000, 3)), axis=0)
    pts = cells + 0.5
    ix = multiscale.NeighborIndex(pts, 1.0)
    off, idx = ix.lists(pts, 3.0)
    want_off, want_idx = oracle.neighbor_lists_c(pts, pts, 1.0, 3.0)
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)
    # some neighbor is at distance exactly 3 along an axis, and it is in
    vox = ix.voxels()
    d2 = ((vox[idx] - np.repeat(pts, np.diff(off), axis=0)) ** 2).sum(1)
    assert d2.max() == 9.0


# ---- one build, many queries -----------------------------------------------------------------------------------

def test_one_build_three_radii_and_a_second_query_cloud():
    from nimrud_amd import synth
    pts, _ = synth.scene_cloud(20000, extent=8.0, n_poles=5, n_spheres=2, seed=71)
    e = 0.1
    ix = multiscale.NeighborIndex(pts, e)
    assert ix.method == "index"
    other = uniform_box(2000, (8.0, 8.0, 1.0), seed=20)
    for query, r in ((pts[:3000], 0.1), (pts[:3000], 0.2), (pts[:3000], 0.3), (other, 0.2)):
        off, idx = ix.lists(query, r)
        want_off, want_idx = multiscale.neighbor_lists(query, pts, e, r, method="search")
        assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)
        off, idx = multiscale.neighbor_lists(query, pts, e, r)            # "auto": the same, from a fresh build
        assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)


# ---- outside the range -------------------------------------------------------------------------------------------

def test_fallback_past_2_21_superblocks():
    pts = uniform_box(4000, (4000.0, 40.0, 40.0), seed=21)
    pts[:2000] = pts[:2000] % 0.4                       # a dense corner: real neighborhoods
    e, r = 0.01, 0.03
    ix = multiscale.NeighborIndex(pts, e)
    assert sum(superblock_bits(ix.filter.widths)) > 21
    assert ix.method == "search"
    off, idx = ix.lists(pts, r)
    want_off, want_idx = oracle.neighbor_lists_c(pts, pts, e, r)
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)
    assert idx.shape[0] > len(pts)
    assert np.array_equal(ix.addresses(), unique_addresses(pts, e)) and ix.n_voxels == len(ix.addresses())
    off, idx = multiscale.neighbor_lists(pts[:500], pts, e, r)
    assert np.array_equal(off, want_off[:501]) and np.array_equal(idx, want_idx[:want_off[500]])
    with pytest.raises(ValueError):
        multiscale.NeighborIndex(pts, e, method="index")
    with pytest.raises(ValueError):
        multiscale.neighbor_lists(pts, pts, e, r, method="index")
    # the C entry points say NM_ERR_LATTICE, with a message, before they touch anything
    rt = _device.get_runtime()
    lat = ix.filter.nm_lattice
    assert rt.lib.nm_neighbor_index_workspace_bytes(len(pts), ctypes.byref(lat)) == 0
    buf = torch.zeros(1024, dtype=torch.uint8, device=rt.device)
    dev = torch.from_numpy(pts).to(rt.device)
    rc = rt.lib.nm_neighbor_index_build(rt.ctx, _device.ptr(dev), len(pts), 3, ctypes.byref(lat), _device.ptr(buf),
                                        _device.ptr(buf), buf.numel(), rt.stream())
    assert rc == _ffi.NM_ERR_LATTICE and b"superblocks" in rt.lib.nm_last_error(rt.ctx)
    rc = rt.lib.nm_neighbor_index_lists(rt.ctx, _device.ptr(dev), len(pts), 3, ctypes.byref(lat), r, _device.ptr(buf),
                                        buf.numel(), _device.ptr(buf), None, None, rt.stream())
    assert rc == _ffi.NM_ERR_LATTICE
    rc = rt.lib.nm_neighbor_index_addresses(rt.ctx, ctypes.byref(lat), _device.ptr(buf), buf.numel(),
                                            _device.ptr(buf), rt.stream())
    assert rc == _ffi.NM_ERR_LATTICE
    # an in-range lattice with too small a workspace, and a ratio candidate_width rejects
    small = geometry.make_nm_lattice([0.0, 0.0, 0.0], 1.0, [6, 4, 4])
    rc = rt.lib.nm_neighbor_index_build(rt.ctx, _device.ptr(dev), len(pts), 3, ctypes.byref(small), _device.ptr(buf),
                                        _device.ptr(buf), buf.numel(), rt.stream())
    assert rc == _ffi.NM_ERR_WORKSPACE
    ci = CIndex(pts[:10], small)
    rc = rt.lib.nm_neighbor_index_lists(rt.ctx, _device.ptr(dev), 10, 3, ctypes.byref(small), 5000.0,
                                        _device.ptr(ci.work), ci.work.numel(), _device.ptr(buf), None, None,
                                        rt.stream())
    assert rc == _ffi.NM_ERR_RADIUS


# ---- search points outside the lattice -----------------------------------------------------------------------------

def test_out_of_bounds_search_points_are_counted_not_indexed():
    lat = geometry.make_nm_lattice([0.0, 0.0, 0.0], 1.0, [6, 4, 4])            # 64 x 16 x 16 cells
    pts = uniform_box(6000, (76.0, 22.0, 22.0), seed=22, origin=(-6.0, -3.0, -3.0))
    cells = np.floor(pts).astype(np.int64)
    inside = np.all((cells >= 0) & (cells < [64, 16, 16]), axis=1)
    assert 1000 < inside.sum() < 5000
    ci = CIndex(pts, lat)
    want = np.unique(cells[inside, 0] + (cells[inside, 1] << 6) + (cells[inside, 2] << 10))
    assert ci.outside == int((~inside).sum())
    assert ci.m == len(want)
    assert np.array_equal(ci.addresses(), want)
    want_cells = np.stack((want & 63, (want >> 6) & 15, want >> 10), axis=1)
    query = pts[:400]                                                          # inside and outside ones alike
    off, idx = ci.lists(query, 2.0)
    want_off, want_idx = brute_lists(query, lat, want_cells, 2.0)
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)
