"""ctypes binding of tests/host_harness_lagbin.cpp: gr_lagbin.hpp -- the per-hit arithmetic and the fixed-point sums of the
lag-energy bins (k_lag_extrema / k_lag_bin) -- compiled for the host with g++, and `binflux` around it exactly as
reverberation._binflux_device puts it around the library's calls."""
import ctypes as C

import numpy as np

import hostbuild


def lib():
    return hostbuild.load("host_harness_lagbin.cpp", flags=["-ffp-contract=off"])


def _rows(rows):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    assert rows.ndim == 2 and rows.shape[1] == 4
    return rows


def extrema(lp, rows):
    """((E_min, E_max, t_min, t_max), Σf, hits) of rows (g, ρ, t, area) under the gr_lagprofile `lp`."""
    rows = _rows(rows)
    lims, flux_sum, hits = np.zeros(4), C.c_double(0.0), C.c_int64(0)
    rc = lib().hlb_extrema(C.byref(lp), C.c_void_p(rows.ctypes.data), C.c_int64(rows.shape[0]), C.c_void_p(lims.ctypes.data),
                           C.byref(flux_sum), C.byref(hits))
    assert rc == 0
    return lims, flux_sum.value, hits.value


def bins(lp, rows, eb, tb):
    """raw Σf per cell, (len(eb), len(tb))"""
    rows = _rows(rows)
    eb, tb = np.ascontiguousarray(eb, dtype=np.float64), np.ascontiguousarray(tb, dtype=np.float64)
    out = np.zeros((eb.size, tb.size))
    rc = lib().hlb_bin(C.byref(lp), C.c_void_p(rows.ctypes.data), C.c_int64(rows.shape[0]), C.c_void_p(eb.ctypes.data), C.c_int64(eb.size),
                       C.c_void_p(tb.ctypes.data), C.c_int64(tb.size), C.c_void_p(out.ctypes.data))
    assert rc == 0
    return out


def hit(lp, row):
    """(E, t, f) of one row, or None if it is no hit"""
    row = np.ascontiguousarray(row, dtype=np.float64)
    etf = np.zeros(3)
    return etf if lib().hlb_hit(C.byref(lp), C.c_void_p(row.ctypes.data), C.c_void_p(etf.ctypes.data)) else None


def bucket(edges, v):
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    return int(lib().hlb_bucket(C.c_void_p(edges.ctypes.data), C.c_int64(edges.size), C.c_double(v)))


def sep_rows(nr, nt, tiled, n, first=0, block=0, stride=0):
    """radius index of the local rays 0 .. n-1 of a separable ray set (gr_lag::sep_row, what k_lag_prepare reads r_i² by)"""
    out = np.zeros(n, dtype=np.int64)
    lib().hlb_sep_rows(C.c_int64(nr), C.c_int64(nt), C.c_int(int(tiled)), C.c_int64(first), C.c_int64(block), C.c_int64(stride),
                       C.c_int64(n), C.c_void_p(out.ctypes.data))
    return out


def binflux(RV, rows, profile, coronal_geodesics, *, E0=6.4, t0, **kwargs):
    """reverberation._binflux_device with the harness in place of the library: the same profile marshalling
    (reverberation._lag_profile) and the same tail (reverberation._binflux_reduce)."""

    class _TF:
        pass

    tf = _TF()
    tf.coronal_geodesics = coronal_geodesics
    lp, keep = RV._lag_profile(tf, profile, E0)
    return RV._binflux_reduce(lambda: extrema(lp, rows)[:2], lambda eb, tb: bins(lp, rows, eb, tb), t0=t0, **kwargs)
