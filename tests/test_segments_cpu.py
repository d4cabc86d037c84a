"""
CPU tests for the segment table: they pin the yardstick the GPU tests (test_segments_gpu.py) are measured against -
the numpy reference of tests/segments_reference.py on segments small enough to compute by hand - and check that the
library declares, binds and exports the new symbols under ABI 7, and that the workspace query is a host function.
"""

import os
import re

import numpy as np

import segments_reference as ref
from nimrud_amd import _ffi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nimrud_hip.h")
SYMBOLS = ("nm_segment_table", "nm_segment_table_workspace_bytes")


def test_unit_square_at_z_7():
    row = ref.segment_row([(0, 0, 7), (1, 0, 7), (0, 1, 7), (1, 1, 7)])
    assert row[0] == 4
    assert np.array_equal(row[1:4], [0.5, 0.5, 7.0])
    assert np.array_equal(row[4:7], [0, 0, 7]) and np.array_equal(row[7:10], [1, 1, 7])
    assert np.allclose(row[10:16], [1 / 3, 0, 0, 1 / 3, 0, 0], rtol=0, atol=1e-15)
    assert np.allclose(row[16:19], [1 / 3, 1 / 3, 0], rtol=0, atol=1e-15)
    assert np.allclose(row[19:22], [0, 0, 1], rtol=0, atol=1e-15)


def test_five_points_on_a_line():
    t = np.array([0.0, 1.0, 2.0, 3.5, 7.0])
    row = ref.segment_row(t[:, None] * np.array([1.0, 2.0, 2.0]))
    lam = np.var(t, ddof=1) * 9.0                         # |(1, 2, 2)|^2 = 9
    assert np.allclose(row[16:19], [lam, 0, 0], rtol=1e-14, atol=1e-14 * lam)
    assert np.allclose(row[22:25], [1 / 3, 2 / 3, 2 / 3], rtol=0, atol=1e-14)
    assert np.allclose(row[1:4], t.mean() * np.array([1.0, 2.0, 2.0]), rtol=1e-15)


def test_one_point_and_two_points():
    row = ref.segment_row([(3.0, -2.0, 5.0)])
    assert row[0] == 1 and np.array_equal(row[1:4], [3, -2, 5])
    assert np.array_equal(row[4:7], [3, -2, 5]) and np.array_equal(row[7:10], [3, -2, 5])
    assert not row[10:].any()
    row = ref.segment_row([(0.0, 0.0, 0.0), (2.0, 0.0, 0.0)])
    assert row[0] == 2 and np.array_equal(row[1:4], [1, 0, 0])
    assert np.array_equal(row[10:16], [2, 0, 0, 0, 0, 0])             # ((-1)^2 + 1^2) / (2 - 1)
    assert np.allclose(row[16:19], [2, 0, 0], rtol=0, atol=1e-15)
    assert not row[19:].any()                                         # fewer than 3 rows: no vectors
    assert not ref.segment_row(np.zeros((0, 3))).any()


def test_weights_are_frequencies():
    p = np.array([(0.0, 0.0, 0.0), (4.0, 2.0, 1.0)])
    weighted = ref.segment_row(p, [3, 1])
    repeated = ref.segment_row(p[[0, 0, 0, 1]])
    assert weighted[0] == 4 and np.array_equal(weighted[:10], repeated[:10])
    assert np.allclose(weighted[10:19], repeated[10:19], rtol=1e-15, atol=1e-15)
    assert np.array_equal(weighted[1:4], [1.0, 0.5, 0.25])
    # a row of weight 0 is not there: not in the box either
    assert np.array_equal(ref.segment_row(np.vstack([p, [(9.0, 9.0, 9.0)]]), [3, 1, 0]), weighted)
    assert not ref.segment_row(p, [0, 0]).any()


def test_table_groups_rows_by_label():
    p = np.arange(18, dtype=np.float64).reshape(6, 3) ** 1.5
    labels = np.array([1, -1, 0, 1, 5, 1])
    table = ref.segment_table(p, labels, n_segments=3)
    assert table.shape == (3, 25)
    assert np.array_equal(table[1], ref.segment_row(p[[0, 3, 5]]))
    assert np.array_equal(table[0], ref.segment_row(p[[2]]))
    assert not table[2].any()
    assert ref.segment_table(p, labels).shape == (6, 25)
    assert ref.segment_table(p[:0], labels[:0]).shape == (0, 25)


def test_ffi_declares_both_symbols():
    lib = _ffi.load()
    header = open(HEADER).read()
    for name in SYMBOLS:
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, header)
    assert len(_ffi.SIGNATURES["nm_segment_table"][1]) == 12
    assert lib.nm_abi_version() == 7 == _ffi.ABI_VERSION


def test_workspace_query_is_a_monotone_host_function():
    nbytes = _ffi.load().nm_segment_table_workspace_bytes
    sizes = [0, 1, 2, 3, 8, 9, 255, 256, 257, 1000, 4095, 4096, 4097, 65536, 100000, 262143, 262144, 262145, 10 ** 6,
             1750000, 10 ** 7, 2 ** 31 - 1]
    table = [[nbytes(n, c) for c in sizes] for n in sizes]
    assert all(v > 0 for line in table for v in line)
    for i in range(len(sizes)):
        for j in range(1, len(sizes)):
            assert table[i][j] >= table[i][j - 1], (sizes[i], sizes[j])
            assert table[j][i] >= table[j - 1][i], (sizes[j], sizes[i])
    for bad in (-1, 2 ** 31, 2 ** 40):
        assert nbytes(bad, 5) == 0 and nbytes(5, bad) == 0


def test_chunk_and_columns_agree_with_the_header():
    header = open(HEADER).read()
    chunk = int(re.search(r"#define NM_SEGMENT_CHUNK\s+(\d+)", header).group(1))
    columns = int(re.search(r"#define NM_SEGMENT_COLUMNS\s+(\d+)", header).group(1))
    assert chunk == _ffi.NM_SEGMENT_CHUNK and chunk > 0 and chunk & (chunk - 1) == 0
    assert columns == _ffi.NM_SEGMENT_COLUMNS == ref.COLUMNS == 25
