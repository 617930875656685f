"""The live-first tile order's partition (gr_tile_order.hpp) compiled for the host with g++ (tests/host_harness_tile_order.cpp):
the permutation is a bijection of [0, tiles), the tiles with a clear flag come first and the tiles with a set flag last, each class
in ascending tile index (a stable partition, against numpy); the flag patterns all clear, all set, alternating and a single set
flag; tile counts that are no multiple of the workgroup size, smaller than it, one and zero; one tile per thread as on the device;
threads placing their chunks in any order give the same permutation."""
import ctypes as C

import numpy as np
import pytest

import hostbuild

SENTINEL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    L = hostbuild.load("host_harness_tile_order.cpp")
    L.hto_chunk_lo.restype = C.c_int64
    L.hto_chunk_lo.argtypes = [C.c_int64, C.c_int, C.c_int]
    L.hto_partition.restype = C.c_uint32
    L.hto_partition.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.hto_chunk_place.restype = None
    L.hto_chunk_place.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, C.c_void_p]
    return L


def _partition(lib, flags, threads):
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    perm = np.full(flags.size + 2, SENTINEL, dtype=np.uint32)      # two guard words behind: never written
    zeros = lib.hto_partition(flags.ctypes.data, flags.size, threads, perm.ctypes.data)
    assert (perm[flags.size:] == SENTINEL).all()
    return perm[:flags.size], int(zeros)


def _check(flags, perm, zeros):
    flags = np.asarray(flags, dtype=np.uint8)
    n = flags.size
    assert zeros == int(np.sum(flags == 0))
    assert np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint32))          # a bijection of [0, tiles)
    assert not flags[perm[:zeros]].any() and flags[perm[zeros:]].all()           # class 0 first, class 1 last
    assert (np.diff(perm[:zeros].astype(np.int64)) > 0).all()                    # each class ascending
    assert (np.diff(perm[zeros:].astype(np.int64)) > 0).all()
    want = np.concatenate([np.flatnonzero(flags == 0), np.flatnonzero(flags != 0)]).astype(np.uint32)
    assert np.array_equal(perm, want)


def _patterns(n, rng):
    alt = (np.arange(n) & 1).astype(np.uint8)
    out = {"all0": np.zeros(n, np.uint8), "all1": np.ones(n, np.uint8), "alt01": alt, "alt10": 1 - alt,
           "random": (rng.random(n) < 0.61).astype(np.uint8), "nonzero-bytes": (rng.integers(0, 256, n) * (rng.random(n) < 0.5)).astype(np.uint8)}
    for name, k in (("single-first", 0), ("single-mid", n // 2), ("single-last", n - 1)):
        if n:
            f = np.zeros(n, np.uint8)
            f[k] = 1
            out[name] = f
            out[name + "-clear"] = 1 - f
    return out


def test_constants_and_chunks(lib):
    T = lib.hto_threads()
    assert T >= 64 and T % 64 == 0 and T <= 1024                  # whole waves, one workgroup
    assert lib.hto_class_lanes() == 4
    # the corners of a tile: lane = column * rows + row, 8 x 8 and 16 x 4
    assert [lib.hto_class_lane(3, k) for k in range(4)] == [0, 7, 56, 63]
    assert [lib.hto_class_lane(4, k) for k in range(4)] == [0, 15, 48, 63]
    for tiles in (0, 1, 63, T - 1, T, T + 1, 3 * T + 17, 65536, 2**21 + 5):
        los = [lib.hto_chunk_lo(tiles, T, t) for t in range(T + 1)]
        assert los[0] == 0 and los[-1] == tiles
        assert all(a <= b for a, b in zip(los[:-1], los[1:]))
        assert max(b - a for a, b in zip(los[:-1], los[1:])) == -(-tiles // T)


@pytest.mark.parametrize("tiles", [0, 1, 2, 63, 64, 65, 512, 1023, 1024, 1025, 2047, 2049, 3 * 1024 + 17, 65536, 65536 + 999])
def test_partition_patterns(lib, tiles):
    rng = np.random.default_rng(1000 + tiles)
    T = lib.hto_threads()
    for name, flags in _patterns(tiles, rng).items():
        perm, zeros = _partition(lib, flags, T)
        _check(flags, perm, zeros)


@pytest.mark.parametrize("threads", [1, 2, 3, 64, 100, 256, 1024])
def test_any_workgroup_size_gives_the_same_order(lib, threads):
    rng = np.random.default_rng(threads)
    for tiles in (1, threads - 1, threads, threads + 1, 5 * threads + 3, 4099):
        if tiles <= 0:
            continue
        flags = (rng.random(tiles) < 0.4).astype(np.uint8)
        perm, zeros = _partition(lib, flags, threads)
        _check(flags, perm, zeros)


@pytest.mark.parametrize("tiles", [1, 7, 8, 9, 1000, 1024, 1025, 4099, 65536])
def test_one_tile_per_thread_in_whole_workgroups(lib, tiles):
    """The device's shape: as many threads as tiles, rounded up to whole workgroups."""
    rng = np.random.default_rng(tiles)
    T = lib.hto_threads()
    threads = -(-tiles // T) * T
    assert [lib.hto_chunk_lo(tiles, threads, t) for t in (0, 1, tiles - 1, tiles, threads)] == [0, min(1, tiles), tiles - 1, tiles, tiles]
    for flags in _patterns(tiles, rng).values():
        perm, zeros = _partition(lib, flags, threads)
        _check(flags, perm, zeros)


def test_chunks_placed_in_any_order(lib):
    """The threads of the workgroup run in no particular order: each places its chunk from the scan's two numbers alone."""
    rng = np.random.default_rng(5)
    T, tiles = lib.hto_threads(), 3 * lib.hto_threads() + 333
    flags = (rng.random(tiles) < 0.61).astype(np.uint8)
    los = [lib.hto_chunk_lo(tiles, T, t) for t in range(T + 1)]
    ones = np.array([int(flags[a:b].sum()) for a, b in zip(los[:-1], los[1:])])
    before = np.concatenate([[0], np.cumsum(ones)[:-1]])
    zeros = tiles - int(ones.sum())
    perm = np.full(tiles, SENTINEL, dtype=np.uint32)
    for t in rng.permutation(T):
        lib.hto_chunk_place(flags.ctypes.data, los[t], los[t + 1], int(before[t]), zeros, perm.ctypes.data)
    _check(flags, perm, zeros)
