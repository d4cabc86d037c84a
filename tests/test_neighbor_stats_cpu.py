"""
CPU tests (no GPU) of the attribute entry points of the neighbor index: the five new symbols are exported and
bound, they came without an ABI bump, and the grouping's scratch size - a host function - grows with the cloud.
"""

import os

from nimrud_amd import _ffi

SYMBOLS = ("nm_neighbor_index_voxel_of", "nm_neighbor_index_group_workspace_bytes", "nm_neighbor_index_group",
           "nm_neighbor_index_voxel_reduce", "nm_neighbor_index_stats")


def test_the_new_symbols_are_exported_and_bound():
    lib = _ffi.load()
    for name in SYMBOLS:
        assert name in _ffi.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == _ffi.SIGNATURES[name][1] and fn.restype == _ffi.SIGNATURES[name][0]


def test_the_header_declares_them_as_additive_within_abi_7():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nimrud_hip.h")
    with open(header) as f:
        text = f.read()
    for name in SYMBOLS:
        assert name + "(" in text
    assert "additive within ABI 7" in text
    assert _ffi.ABI_VERSION == 7
    assert _ffi.load().nm_abi_version() == 7
    assert _ffi.NM_REDUCE == {"mean": 0, "sum": 1, "min": 2, "max": 3} and _ffi.NM_STATS_MAX_DIMS == 16


def test_group_workspace_bytes_is_positive_and_non_decreasing():
    nbytes = _ffi.load().nm_neighbor_index_group_workspace_bytes
    sizes = [nbytes(n) for n in (1, 63, 64, 65, 4096, 4097, 2 ** 20, 2 ** 20 + 1)]
    assert all(s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    # a cursor word per voxel at the least, and there can be as many voxels as points
    assert sizes[-2] >= 4 * 2 ** 20 and sizes[-1] > sizes[-2]
    assert nbytes(0) > 0
    # outside the range: a negative count, or more rows than the int32 row numbers of the ordering hold
    assert nbytes(-1) == 0 and nbytes(2 ** 31) == 0
