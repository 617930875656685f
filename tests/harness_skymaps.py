"""ctypes binding of tests/host_harness_skymaps.cpp: what gr_sky_bin_grid, gr_sky_fill and gr_disc_area_factor run per leaf, per
column and per radius (gr_skygrid.hpp, gr_lagbin.hpp, disc_area_factor of gr_device.hpp), compiled for the host with g++ on the
arrays of a grids.AdaptiveGrid and the rows of an AdaptiveSky."""
import ctypes as C

import numpy as np

import hostbuild

MAPS = {"emissivity": 0, "redshift": 1, "time": 2}


class hsm_grid(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("level", C.c_void_p), ("children", C.c_void_p), ("neighbours", C.c_void_p), ("parent", C.c_void_p),
                ("location", C.c_void_p), ("n", C.c_int64), ("limits", C.c_double * 4)]


def lib():
    L = hostbuild.load("host_harness_skymaps.cpp", flags=["-ffp-contract=off", "-Wno-attributes"])
    L.hsm_fill.restype = C.c_int64
    return L


class Sky:
    """The arrays of a sky's grid and its rows, contiguous and kept alive; `rows` may be replaced (a NaN row)"""

    FIELDS = ("pos", "level", "children", "neighbours", "parent", "location")

    def __init__(self, sky):
        grid = sky.grid
        self.n, self.limits = grid.n, grid.limits
        for f in self.FIELDS:
            setattr(self, f, np.ascontiguousarray(getattr(grid, f)[:grid.n + 1]))
        self.rows = np.ascontiguousarray(sky.values).view(np.float64).reshape(-1, 6).copy()
        assert self.rows.shape[0] == self.n + 1

    def c(self):
        h = hsm_grid()
        for f in self.FIELDS:
            setattr(h, f, getattr(self, f).ctypes.data)
        h.n = self.n
        (x1, x2), (y1, y2) = self.limits
        h.limits[:] = [x1, x2, y1, y2]
        return h


def bin_grid(s, what, r_bins, ϕ_bins, Γ=None, area=None, order=None):
    """(return code, map[r, ϕ], Σ ΔΩ[r, ϕ]); `order`: the cells in the order they are visited (default 1 ... n); `area`: γA per cell"""
    r_bins, ϕ_bins = np.ascontiguousarray(r_bins, dtype=np.float64), np.ascontiguousarray(ϕ_bins, dtype=np.float64)
    order = np.arange(1, s.n + 1, dtype=np.int64) if order is None else np.ascontiguousarray(order, dtype=np.int64)
    out, solid = np.zeros((r_bins.size, ϕ_bins.size)), np.zeros((r_bins.size, ϕ_bins.size))
    if area is not None:
        area = np.ascontiguousarray(area, dtype=np.float64)
        assert area.size == s.n + 1
    rc = lib().hsm_bin_grid(C.byref(s.c()), C.c_void_p(s.rows.ctypes.data), C.c_void_p(order.ctypes.data), C.c_int64(order.size),
                            C.c_int(MAPS[what]), C.c_void_p(r_bins.ctypes.data), C.c_int64(r_bins.size), C.c_void_p(ϕ_bins.ctypes.data),
                            C.c_int64(ϕ_bins.size), C.c_int(Γ is not None), C.c_double(0.0 if Γ is None else Γ),
                            None if area is None else C.c_void_p(area.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(solid.ctypes.data))
    return int(rc), out, solid


def fill(s, ϕ_grid, θ_grid, chunk=256):
    """(rows[θ, ϕ] as six doubles, lower cell[θ, ϕ], upper cell[θ, ϕ], the compacted column of cells per ϕ, the number of columns
    whose θ do not ascend): the column loop of k_sky_fill in chunks of `chunk` points"""
    ϕ_grid, θ_grid = np.ascontiguousarray(ϕ_grid, dtype=np.float64), np.ascontiguousarray(θ_grid, dtype=np.float64)
    cosθ = np.ascontiguousarray(np.cos(θ_grid))
    nθ, nϕ = θ_grid.size, ϕ_grid.size
    out = np.empty((nθ, nϕ, 6))
    cells = np.empty((nθ, nϕ, 2), dtype=np.int64)
    counts = np.zeros(nϕ, dtype=np.int64)
    compacted = np.zeros((nϕ, nθ), dtype=np.int64)
    bad = lib().hsm_fill(C.byref(s.c()), C.c_void_p(s.rows.ctypes.data), C.c_void_p(ϕ_grid.ctypes.data), C.c_int64(nϕ),
                         C.c_void_p(θ_grid.ctypes.data), C.c_void_p(cosθ.ctypes.data), C.c_int64(nθ), C.c_int64(chunk),
                         C.c_void_p(out.ctypes.data), C.c_void_p(cells.ctypes.data), C.c_void_p(counts.ctypes.data),
                         C.c_void_p(compacted.ctypes.data))
    return out, cells[..., 0].copy(), cells[..., 1].copy(), [compacted[k, :counts[k]].copy() for k in range(nϕ)], int(bad)


def area_factor(G, m, r, r_isco, table):
    """disc_area_factor at the radii `r` for the metric `m`, the ISCO and the plunging table given (None: Kerr's analytic plunge)"""
    from gradus_jl_amd.pointfunctions import GR_PF_REDSHIFT, PointFunction
    from gradus_jl_amd.rendering import abi_pointfunction

    cfg = G._lib.gr_config()
    cfg.metric_id = m.metric_id
    for i, p in enumerate(m.abi_params()):
        cfg.params[i] = float(p)
    pf, keep = abi_pointfunction(PointFunction(None, device_pf=GR_PF_REDSHIFT, extra={"r_isco": r_isco, "plunge": table}))
    r = np.ascontiguousarray(r, dtype=np.float64)
    out = np.empty(r.size)
    rc = lib().hsm_area_factor(C.byref(cfg), C.byref(pf), C.c_void_p(r.ctypes.data), C.c_int64(r.size), C.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    del keep
    return out
