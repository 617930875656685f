"""ctypes binding of tests/host_harness_skygrid.cpp: gr_skygrid.hpp -- the tree logic of a resident adaptive sky (the k_sky_*
kernels call the same functions per cell) -- compiled for the host with g++, on the arrays of a grids.AdaptiveGrid."""
import ctypes as C

import numpy as np

import hostbuild


class hsg_grid(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("level", C.c_void_p), ("children", C.c_void_p), ("neighbours", C.c_void_p), ("parent", C.c_void_p),
                ("location", C.c_void_p), ("n", C.c_int64), ("limits", C.c_double * 4)]


def lib():
    L = hostbuild.load("host_harness_skygrid.cpp", flags=["-ffp-contract=off"])
    L.hsg_top.restype = L.hsg_pairs.restype = L.hsg_find_need_refine.restype = L.hsg_bins.restype = C.c_int64
    return L


class Grid:
    """The six arrays of a grid, owned here (a copy of an AdaptiveGrid's, or the nine top cells), with room to grow"""

    FIELDS = ("pos", "level", "children", "neighbours", "parent", "location")

    def __init__(self, grid=None, limits=None, x_periodic=True, room=0):
        if grid is not None:
            self.n, self.limits = grid.n, grid.limits
            for f in self.FIELDS:
                a = getattr(grid, f)[:grid.n + 1]
                b = np.zeros((grid.n + 1 + room,) + a.shape[1:], dtype=a.dtype)
                b[:grid.n + 1] = a
                setattr(self, f, b)
        else:
            self.n, self.limits = 0, limits
            shapes = {"pos": ((2,), np.float64), "level": ((), np.int32), "children": ((9,), np.int64), "neighbours": ((4,), np.int64),
                      "parent": ((), np.int64), "location": ((), np.int8)}
            for f, (shape, dt) in shapes.items():
                setattr(self, f, np.zeros((10 + room,) + shape, dtype=dt))
            self.n = int(lib().hsg_top(C.byref(self.c()), C.c_int(int(x_periodic))))

    def c(self):
        h = hsg_grid()
        for f in self.FIELDS:
            setattr(h, f, getattr(self, f).ctypes.data)
        h.n = self.n
        (x1, x2), (y1, y2) = self.limits
        h.limits[:] = [x1, x2, y1, y2]
        return h

    def room(self, extra):
        for f in self.FIELDS:
            a = getattr(self, f)
            if a.shape[0] < self.n + 1 + extra:
                b = np.zeros((self.n + 1 + extra,) + a.shape[1:], dtype=a.dtype)
                b[:a.shape[0]] = a
                setattr(self, f, b)

    def arrays(self):
        return {f: getattr(self, f)[:self.n + 1] for f in self.FIELDS}


def pairs(g):
    h = g.c()
    n = int(lib().hsg_pairs(C.byref(h), None, None, C.c_int64(0)))
    assert n >= 0
    i1, i2 = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    assert lib().hsg_pairs(C.byref(h), C.c_void_p(i1.ctypes.data), C.c_void_p(i2.ctypes.data), C.c_int64(n)) == n
    return i1, i2


def _rows(values):
    rows = np.ascontiguousarray(values).view(np.float64).reshape(-1, 6)
    return rows


def find_need_refine(g, values, criterion):
    rows = _rows(values)
    assert rows.shape[0] == g.n + 1
    out = np.empty(g.n + 1, dtype=np.int64)
    m = int(lib().hsg_find_need_refine(C.byref(g.c()), C.c_void_p(rows.ctypes.data), C.byref(criterion), C.c_void_p(out.ctypes.data)))
    assert m >= 0
    return out[:m].copy()


def refine(g, cells, rows=None):
    """0, or the refusal code with the grid untouched"""
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    g.room(9 * cells.size)
    h = g.c()
    rc = int(lib().hsg_refine(C.byref(h), C.c_void_p(cells.ctypes.data), C.c_int64(cells.size),
                              None if rows is None else C.c_void_p(rows.ctypes.data)))
    g.n = int(h.n)
    return rc


def parent_index(g, x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    out = np.empty(x.size, dtype=np.int64)
    lib().hsg_parent_index(C.byref(g.c()), C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data), C.c_int64(x.size), C.c_void_p(out.ctypes.data))
    return out


def bins(g, values, r_bins, ϕ_bins, Γ=2):
    """(leaves, r index, ϕ index, counts[r, ϕ]) of the leaves that land in a bin"""
    rows = _rows(values)
    r_bins, ϕ_bins = np.ascontiguousarray(r_bins, dtype=np.float64), np.ascontiguousarray(ϕ_bins, dtype=np.float64)
    leaf, ri, pi = (np.empty(g.n + 1, dtype=np.int64) for _ in range(3))
    counts = np.zeros((r_bins.size, ϕ_bins.size), dtype=np.int64)
    m = int(lib().hsg_bins(C.byref(g.c()), C.c_void_p(rows.ctypes.data), C.c_void_p(r_bins.ctypes.data), C.c_int64(r_bins.size),
                           C.c_void_p(ϕ_bins.ctypes.data), C.c_int64(ϕ_bins.size), C.c_int(Γ is not None), C.c_double(0.0 if Γ is None else Γ),
                           C.c_void_p(leaf.ctypes.data), C.c_void_p(ri.ctypes.data), C.c_void_p(pi.ctypes.data), C.c_void_p(counts.ctypes.data)))
    return leaf[:m].copy(), ri[:m].copy(), pi[:m].copy(), counts
