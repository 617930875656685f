"""ctypes binding of tests/host_harness_planegrid.cpp: the pair criterion and the filled image of an adaptive image plane
(gr_planegrid.hpp) compiled for the host with g++, on the arrays of a grids.AdaptiveGrid and the points of an AdaptivePlane."""
import ctypes as C

import numpy as np

import hostbuild

CRIT_LEVEL, CRIT_PLANE = 3, 4


class hpg_grid(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("level", C.c_void_p), ("children", C.c_void_p), ("neighbours", C.c_void_p), ("parent", C.c_void_p),
                ("location", C.c_void_p), ("n", C.c_int64), ("limits", C.c_double * 4)]


def lib():
    return hostbuild.load("host_harness_planegrid.cpp", flags=["-ffp-contract=off", "-Wno-attributes"])


class Plane:
    """The arrays of a plane's grid and its points, contiguous and kept alive; `points` may be replaced"""

    FIELDS = ("pos", "level", "children", "neighbours", "parent", "location")

    def __init__(self, sky):
        grid = sky.grid
        self.n, self.limits = grid.n, grid.limits
        for f in self.FIELDS:
            setattr(self, f, np.ascontiguousarray(getattr(grid, f)[:grid.n + 1]))
        self.points = np.ascontiguousarray(sky.values).copy()
        assert self.points.shape[0] == self.n + 1 and self.points.dtype.itemsize == 152

    def c(self):
        h = hpg_grid()
        for f in self.FIELDS:
            setattr(h, f, getattr(self, f).ctypes.data)
        h.n = self.n
        (x1, x2), (y1, y2) = self.limits
        h.limits[:] = [x1, x2, y1, y2]
        return h


def need_refine(p, i1, i2, percentage=20, kind=CRIT_PLANE, level=0, points=None):
    """gr_planegrid::need_refine over index arrays -> bool array; `points`: other rows than the plane's"""
    i1, i2 = np.ascontiguousarray(i1, dtype=np.int64), np.ascontiguousarray(i2, dtype=np.int64)
    points = p.points if points is None else np.ascontiguousarray(points)
    out = np.zeros(i1.size, dtype=np.uint8)
    lib().hpg_need_refine(C.byref(p.c()), C.c_void_p(points.ctypes.data), C.c_int(kind), C.c_int(level), C.c_double(percentage / 100),
                          C.c_void_p(i1.ctypes.data), C.c_void_p(i2.ctypes.data), C.c_int64(i1.size), C.c_void_p(out.ctypes.data))
    return out.astype(bool)


def fill(p, val, x_grid, y_grid):
    """(out[β, α], lower cell[β, α], upper cell[β, α], cells recorded per column)"""
    x_grid, y_grid = np.ascontiguousarray(x_grid, dtype=np.float64), np.ascontiguousarray(y_grid, dtype=np.float64)
    val = np.ascontiguousarray(val, dtype=np.float64)
    assert val.size == p.n + 1
    out = np.empty((y_grid.size, x_grid.size))
    cells = np.empty((y_grid.size, x_grid.size, 2), dtype=np.int64)
    counts = np.zeros(x_grid.size, dtype=np.int64)
    lib().hpg_fill(C.byref(p.c()), C.c_void_p(p.points.ctypes.data), C.c_void_p(val.ctypes.data), C.c_void_p(x_grid.ctypes.data),
                   C.c_int64(x_grid.size), C.c_void_p(y_grid.ctypes.data), C.c_int64(y_grid.size), C.c_void_p(out.ctypes.data),
                   C.c_void_p(cells.ctypes.data), C.c_void_p(counts.ctypes.data))
    return out, cells[..., 0].copy(), cells[..., 1].copy(), counts


def top_neighbours(limits, x_periodic):
    limits = np.ascontiguousarray(limits, dtype=np.float64)
    out = np.zeros((10, 4), dtype=np.int64)
    lib().hpg_top_neighbours(C.c_void_p(limits.ctypes.data), C.c_int(int(x_periodic)), C.c_void_p(out.ctypes.data))
    return out
