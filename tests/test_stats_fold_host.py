"""The statistics fold (gr_stats_fold.hpp) compiled for the host with g++ (tests/host_harness_stats_fold.cpp): the column sums of
an S x 9 block of 64-bit partial sums added into nine counters, against numpy; rows left at zero, row counts that are no multiple
of the unrolled four, counters that already hold an earlier launch's sums, wrapping sums, and the block left zero."""
import ctypes as C

import numpy as np
import pytest

import hostbuild


@pytest.fixture(scope="module")
def lib():
    L = hostbuild.load("host_harness_stats_fold.cpp")
    L.hsf_column_sum.restype = C.c_ulonglong
    L.hsf_column_sum.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.hsf_fold.restype = None
    L.hsf_fold.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.hsf_row_of.restype = C.c_uint
    L.hsf_row_of.argtypes = [C.c_uint]
    return L


def _fold(lib, part, counters, cols):
    rows, stride = part.shape
    lib.hsf_fold(part.ctypes.data, rows, stride, cols, counters.ctypes.data)


def test_layout(lib):
    S, stride, cols = lib.hsf_rows(), lib.hsf_stride(), lib.hsf_cols()
    assert cols == 9 and stride >= cols
    assert S >= 1 and S & (S - 1) == 0                       # a power of two: the row is the workgroup index masked
    assert stride * 8 % 128 == 0                             # a row begins a 128-byte line of its own
    rows = [lib.hsf_row_of(b) for b in range(5 * S + 3)]
    assert rows == [b % S for b in range(5 * S + 3)]
    assert lib.hsf_row_of(2**32 - 1) == (2**32 - 1) % S


@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5, 7, 8, 63, 64, 65])
def test_fold_against_numpy(lib, rows):
    rng = np.random.default_rng(100 + rows)
    stride, cols = lib.hsf_stride(), lib.hsf_cols()
    part = np.zeros((rows, stride), dtype=np.uint64)
    part[:, :cols] = rng.integers(0, 2**40, size=(rows, cols), dtype=np.uint64)
    part[rng.random(rows) < 0.4, :] = 0                      # rows no workgroup added to
    part[:, cols:] = rng.integers(1, 2**40, size=(rows, stride - cols), dtype=np.uint64)      # padding: never read
    want_cols = part[:, :cols].sum(axis=0, dtype=np.uint64)
    for c in range(cols):
        assert lib.hsf_column_sum(part.ctypes.data, rows, stride, c) == int(want_cols[c])
    counters = rng.integers(0, 2**50, size=11, dtype=np.uint64)      # an earlier launch's sums; kernel_ms / call_ms slots behind
    before = counters.copy()
    _fold(lib, part, counters, cols)
    assert (counters[:cols] == before[:cols] + want_cols).all()
    assert (counters[cols:] == before[cols:]).all()
    assert not part.any()                                    # the block is zero for the launch that draws it next


def test_all_rows_zero_changes_nothing(lib):
    stride, cols, S = lib.hsf_stride(), lib.hsf_cols(), lib.hsf_rows()
    part = np.zeros((S, stride), dtype=np.uint64)
    counters = np.arange(1, 10, dtype=np.uint64)
    _fold(lib, part, counters, cols)
    assert counters.tolist() == list(range(1, 10))


def test_sums_wrap_like_the_atomics_that_fill_the_block(lib):
    stride, cols = lib.hsf_stride(), lib.hsf_cols()
    part = np.zeros((8, stride), dtype=np.uint64)
    part[:, 0] = np.uint64(2**62)                            # 8 x 2^62 = 2^65 = 0 (mod 2^64)
    part[:, 1] = np.uint64(2**61)                            # 8 x 2^61 = 2^64 = 0 (mod 2^64)
    part[:3, 2] = np.uint64(2**63)                           # 3 x 2^63 = 2^63 (mod 2^64)
    counters = np.zeros(9, dtype=np.uint64)
    counters[1] = 5
    _fold(lib, part, counters, cols)
    assert counters.tolist() == [0, 5, 2**63, 0, 0, 0, 0, 0, 0]


def test_two_folds_accumulate(lib):
    rng = np.random.default_rng(7)
    stride, cols, S = lib.hsf_stride(), lib.hsf_cols(), lib.hsf_rows()
    counters = np.zeros(9, dtype=np.uint64)
    total = np.zeros(9, dtype=np.uint64)
    for _ in range(2):
        part = np.zeros((S, stride), dtype=np.uint64)
        part[:, :cols] = rng.integers(0, 2**33, size=(S, cols), dtype=np.uint64)
        total += part[:, :cols].sum(axis=0, dtype=np.uint64)
        _fold(lib, part, counters, cols)
    assert (counters == total).all()
