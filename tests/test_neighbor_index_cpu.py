"""
CPU tests (no GPU) of the neighbor index's C ABI: the four nm_neighbor_index_* symbols are bound, the ABI
version moved with them, and the workspace query - a host function - knows the path's range.
"""

import ctypes

from nimrud_amd import _ffi
from nimrud_amd.utils import geometry

SYMBOLS = ("nm_neighbor_index_workspace_bytes", "nm_neighbor_index_build", "nm_neighbor_index_addresses",
           "nm_neighbor_index_lists")


def test_the_four_symbols_are_bound():
    lib = _ffi.load()
    for name in SYMBOLS:
        assert name in _ffi.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == _ffi.SIGNATURES[name][1] and fn.restype == _ffi.SIGNATURES[name][0]


def test_abi_version_is_7_on_both_sides():
    assert _ffi.ABI_VERSION == 7
    assert _ffi.load().nm_abi_version() == 7


def test_workspace_bytes_is_a_host_function_that_knows_the_range():
    lib = _ffi.load()
    nbytes = lib.nm_neighbor_index_workspace_bytes
    lat = geometry.make_nm_lattice([0.0, 0.0, 0.0], 0.1, [10, 10, 6])      # 2^(5+7+3) superblocks
    sizes = [nbytes(n, ctypes.byref(lat)) for n in (0, 1, 1000, 100000, 10000000)]
    assert sizes[0] > 0
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))                   # non-decreasing in n_search
    # leaves and ranks: a 256-byte leaf and as many rank words per superblock, at the least
    assert sizes[2] >= 2 * (1 << 15) * 256
    # narrower than one leaf on every axis: one superblock
    tiny = geometry.make_nm_lattice([0.0, 0.0, 0.0], 1.0, [4, 2, 2])
    assert 0 < nbytes(10, ctypes.byref(tiny)) < 1 << 16
    # the limit is 2^21 superblocks: (5+9) + (3+6) + (3+6) address bits are in, one more bit is out
    edge_case = geometry.make_nm_lattice([0.0, 0.0, 0.0], 0.1, [14, 9, 9])
    assert nbytes(1000, ctypes.byref(edge_case)) >= 2 * (1 << 21) * 256
    for widths in ([15, 9, 9], [14, 10, 9], [14, 9, 10], [27, 3, 3]):       # 2^22 superblocks
        beyond = geometry.make_nm_lattice([0.0, 0.0, 0.0], 0.1, widths)
        assert nbytes(1000, ctypes.byref(beyond)) == 0
    # and nothing for a lattice that is none, or a negative count
    bad = geometry.make_nm_lattice([0.0, 0.0, 0.0], 0.1, [10, 10, 6])
    bad.shifts[0] = 3
    assert nbytes(1000, ctypes.byref(bad)) == 0
    assert nbytes(-1, ctypes.byref(lat)) == 0
