"""ctypes binding of tests/host_harness_tfint.cpp -- gr_tfint.hpp, the arithmetic of gr_tf_lineprofile / gr_tf_lagtransfer,
compiled for the host with g++ -- and what the CPU and the GPU tests of the integration share: synthetic ragged branches, a
disc profile, an independent scalar restatement of the two integrals, and the comparison rules."""
import bisect
import ctypes as C
import math

import numpy as np

import hostbuild

TOL = 1e-12          # of the peak: the bound of every comparison between two routes of the same integral


def lib():
    L = hostbuild.load("host_harness_tfint.cpp", flags=["-ffp-contract=off"])
    L.htf_lineprofile.restype = L.htf_lagtransfer.restype = C.c_int64
    L.htf_bin.restype = C.c_double
    return L


class Calls:
    """The harness with the argument lists transfer_functions._tf_run gives its `call`; counts the deposits."""

    def __init__(self):
        self.deposits = 0

    def line(self, sets, n, quad, g, n_g, out):
        self.deposits = lib().htf_lineprofile(sets, C.c_int64(n), quad, C.c_void_p(g), C.c_int64(n_g), C.c_void_p(out))

    def lag(self, sets, n, quad, g, n_g, t, n_t, out):
        self.deposits = lib().htf_lagtransfer(sets, C.c_int64(n), quad, C.c_void_p(g), C.c_int64(n_g), C.c_void_p(t), C.c_int64(n_t),
                                              C.c_void_p(out))


def harness_lineprofile(TF, ε, tfs, g_grid, **kw):
    c = Calls()
    flux = TF.integrate_lineprofiles([ε], [tfs], g_grid, ensemble=None, _call=c.line, **kw)[0]
    return flux, c.deposits


def harness_lagtransfer(TF, prof, tfs, g_grid, t_grid, *, rmin=None, rmax=None, g_scale=1.0, h=1e-8, n_radii=1000,
                        quadrature_points=7, t0=0.0):
    c = Calls()
    flux = TF._integrate_lagtransfer_device(prof, tfs, g_grid, t_grid, rmin=rmin, rmax=rmax, g_scale=g_scale, h=h, n_radii=n_radii,
                                            quadrature_points=quadrature_points, t0=t0, call=c.lag)
    return flux, c.deposits


def integrate_bin(TF, tfs, r_int, ia, mode, lo, hi, *, h=1e-8, quadrature_points=7):
    """(integrate_bin of annulus ia, (gmin, gmax, weight)) from the header; ε = 1"""
    from gradus_jl_amd import _lib as L

    r_int = np.ascontiguousarray(r_int, dtype=np.float64)
    s, keep = TF._tf_set(tfs, r_int, np.ones(r_int.size), np.zeros(r_int.size), r_int[0], 1.0)
    X, W = np.polynomial.legendre.leggauss(quadrature_points)
    q = L.gr_tfquad(float(h), X.size, X.ctypes.data, W.ctypes.data)
    ann = np.zeros(3)
    v = lib().htf_bin(C.byref(s), C.byref(q), C.c_int64(ia), C.c_int(mode), C.c_double(lo), C.c_double(hi), C.c_void_p(ann.ctypes.data))
    return v, ann


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def synthetic_branches(TF, *, n_r=23, knots=(12, 16), r_lims=(1.3, 50.0), seed=7, knots_of=None, constant_g=False, shared_knots=None,
                       nan_f=()):
    """Ragged branches as interpolate_branches leaves them: per radius a lower and an upper branch on knot sets of their
    own (g✶ from 0 to 1, `knots[0]` ... `knots[1]` of them; `knots_of = {(radius index, 'lower' | 'upper'): n}` overrides),
    smooth positive f, smooth t, gmin / gmax varying with r (or the same for every radius: constant_g).  `shared_knots`: one
    knot array for every branch (what a CunninghamTransferGrid holds); `nan_f`: (radius index, side, knot index) whose f is NaN."""
    rng = np.random.default_rng(seed)
    radii = r_lims[0] * (r_lims[1] / r_lims[0]) ** (np.arange(n_r) / (n_r - 1))
    out = []
    for k, r in enumerate(radii):
        u = 1.0 - r_lims[0] / r
        gmin, gmax = (0.45, 1.2) if constant_g else (0.2 + 0.55 * u, 1.35 - 0.3 * u)
        arrs = {}
        for side in ("lower", "upper"):
            n = int(rng.integers(knots[0], knots[1] + 1))
            n = (knots_of or {}).get((k, side), n)
            g = np.concatenate([[0.0], np.sort(rng.uniform(2e-3, 1.0 - 2e-3, n - 2)), [1.0]])
            if shared_knots is not None:
                g = np.asarray(shared_knots, dtype=np.float64)
            if side == "lower":
                f = (0.3 + 2.0 * g * (1.0 - g) + 0.2 * g) * (1.0 + 0.1 * math.sin(r))
                t = 40.0 + r * (1.0 - 0.6 * np.cos(math.pi * g))
            else:
                f = (0.5 + 1.2 * np.sqrt(g * (1.0 - g)) + 0.1 * (1.0 - g)) * (1.0 + 0.1 * math.cos(r))
                t = 40.0 + r * (1.0 + 0.8 * np.sin(math.pi * g) - 0.6 * np.cos(math.pi * g))
            for kk, ss, i in nan_f:
                if kk == k and ss == side:
                    f[i] = np.nan
            arrs[side] = (g, f, t)
        out.append(TF.TransferBranches(*arrs["upper"], *arrs["lower"], gmin, gmax, float(r)))
    return TF.InterpolatingTransferBranches.from_branches(out)


class Profile:
    """emissivity_at / coordtime_at of a lamp post at height 5 with ε = r^-3"""

    def emissivity_at(self, r):
        return np.asarray(r, dtype=np.float64) ** -3.0

    def coordtime_at(self, r):
        return np.sqrt(np.asarray(r, dtype=np.float64) ** 2 + 25.0)


def emissivity(r):
    return r ** -3.0


G_GRID = np.linspace(0.1, 1.5, 61)                           # 60 g bins
T_GRID = math.sqrt(2.0) + 44.0 + np.linspace(0.0, 120.0, 97)      # 96 t bins from an irrational offset


# ---------------------------------------------------------------------------------------------------------------
# the third voice: integration.jl:74-200,336-453 restated scalar by scalar, with NaNLinearInterpolator's formula
# ---------------------------------------------------------------------------------------------------------------
def _nan_lerp(t, u, x):
    idx = min(max(bisect.bisect_right(t, x), 1), len(t) - 1) - 1
    w = (x - t[idx]) / (t[idx + 1] - t[idx])
    y = (1 - w) * u[idx] + w * u[idx + 1]
    if math.isnan(y):
        y = u[idx] if w < 0.5 else u[idx + 1]
        y = 0.0 if math.isnan(y) else y
    return y


def _branch_at(tfs, r):
    radii = tfs.radii.tolist()
    idx = min(max(bisect.bisect_right(radii, r), 1), len(radii) - 1) - 1
    θ = (r - radii[idx]) / (radii[idx + 1] - radii[idx])
    b1, b2 = tfs.branches[idx], tfs.branches[idx + 1]
    lists = {}
    for key in ("lower_g", "lower_f", "lower_t", "upper_g", "upper_f", "upper_t"):
        lists[key] = (getattr(b1, key).tolist(), getattr(b2, key).tolist())

    def field(side, what):
        (g1, g2), (y1, y2) = lists[side + "_g"], lists[side + "_" + what]
        return lambda x: (1 - θ) * _nan_lerp(g1, y1, x) + θ * _nan_lerp(g2, y2, x)

    gmin = (1 - θ) * tfs.gmin[idx] + θ * tfs.gmin[idx + 1]
    gmax = (1 - θ) * tfs.gmax[idx] + θ * tfs.gmax[idx + 1]
    return float(gmin), float(gmax), {(s, w): field(s, w) for s in ("lower", "upper") for w in ("f", "t")}


def _zin(v):
    return 0.0 if math.isnan(v) else v


def _sqrt(v):
    return math.sqrt(v) if v >= 0 else math.nan


def _div(a, b):
    return a / b if b != 0 else (math.nan if a == 0 or math.isnan(a) else math.copysign(math.inf, a))


def _ref_integrate_bin(S, lo, hi, gmin, gmax, h, X, W):
    glo, ghi = min(max(lo, gmin), gmax), min(max(hi, gmin), gmax)
    if glo == ghi:
        return 0.0
    span = gmax - gmin
    slo, shi = (lo - gmin) / span, (hi - gmin) / span

    def edge(lim, lim_gs):
        gh = span * lim_gs + gmin
        return S(gh) * abs(_sqrt(gh) - _sqrt(lim)) * math.sqrt(h)

    lum = 0.0
    if slo < h:
        if shi > h:
            lum += edge(glo, h)
            glo = span * h + gmin
        else:
            return edge(glo, shi)
    if shi > 1 - h:
        if slo < 1 - h:
            lum += edge(ghi, 1 - h)
            ghi = span * (1 - h) + gmin
        else:
            return edge(ghi, slo)
    half = (ghi - glo) / 2
    acc = 0.0
    for x, w in zip(X, W):
        acc += S((x + 1) * half + glo) * w
    return lum + acc * half


def _ref_S(fields, sides, gmin, gmax):
    def S(g):
        gs = (g - gmin) / (gmax - gmin)
        f = sum(_zin(fields[(s, "f")](gs)) for s in sides)
        return _div(g * g * f * g, _sqrt(gs * (1 - gs)))
    return S


def _finite(v):
    return v if math.isfinite(v) else 0.0


def restated_lineprofile(tfs, ε, g_grid, *, n_radii, h=1e-8, quadrature_points=7):
    """integrate_lineprofile without any of the package's code but the grid: raw sums, then _normalize!"""
    X, W = (a.tolist() for a in np.polynomial.legendre.leggauss(quadrature_points))
    lo_r, hi_r = float(tfs.radii[0]), float(tfs.radii[-1])
    radii = [1.0 / x for x in np.linspace(1.0 / hi_r, 1.0 / lo_r, n_radii)][::-1]
    out = [0.0] * len(g_grid)
    r_prev = lo_r - (radii[1] - lo_r)
    for r in radii:
        gmin, gmax, fields = _branch_at(tfs, r)
        S = _ref_S(fields, ("lower", "upper"), gmin, gmax)
        θ = (r - r_prev) * r * ε(r) * math.pi / (gmax - gmin)
        r_prev = r
        for j in range(len(g_grid) - 1):
            out[j] += _finite(_ref_integrate_bin(S, float(g_grid[j]), float(g_grid[j + 1]), gmin, gmax, h, X, W)) * θ
    flux = np.array(out)
    flux[:-1] /= g_grid[1:] + g_grid[:-1]
    return flux / flux[:-1].sum()


def restated_lagtransfer(tfs, prof, g_grid, t_grid, *, n_radii, h=1e-8, quadrature_points=7, t0=0.0):
    X, W = (a.tolist() for a in np.polynomial.legendre.leggauss(quadrature_points))
    lo_r, hi_r = float(tfs.radii[0]), float(tfs.radii[-1])
    K = (hi_r / lo_r) ** (1.0 / (n_radii - 1))
    radii = [lo_r * K ** i for i in range(n_radii)]
    edges = t_grid.tolist()
    out = np.zeros((len(g_grid), len(t_grid)))
    n_dep = 0
    r_prev = lo_r - (radii[1] - lo_r)
    for r in radii:
        gmin, gmax, fields = _branch_at(tfs, r)
        S1, S2 = _ref_S(fields, ("lower",), gmin, gmax), _ref_S(fields, ("upper",), gmin, gmax)
        θ = (r - r_prev) * r * float(prof.emissivity_at(r)) * math.pi / (gmax - gmin)
        tsd = float(prof.coordtime_at(r)) - t0
        r_prev = r

        def times(gs):
            gs = min(max(gs, 0.0), 1.0)
            tl, tu = fields[("lower", "t")], fields[("upper", "t")]
            if gs < h:
                ω, a, b = gs / h, tl(h), tu(h)
            elif gs > 1 - h:
                ω, a, b = 1 - (1 - gs) / h, tl(1 - h), tu(1 - h)
            else:
                return tl(gs), tu(gs)
            return a * ω + (1 - ω) * b, b * ω + (1 - ω) * a

        for j in range(len(g_grid) - 1):
            glo, ghi = min(max(float(g_grid[j]), gmin), gmax), min(max(float(g_grid[j + 1]), gmin), gmax)
            if glo == ghi:
                continue
            k1 = _finite(_ref_integrate_bin(S1, glo, ghi, gmin, gmax, h, X, W))
            k2 = _finite(_ref_integrate_bin(S2, glo, ghi, gmin, gmax, h, X, W))
            (tl1, tu1), (tl2, tu2) = times((glo - gmin) / (gmax - gmin)), times((ghi - gmin) / (gmax - gmin))
            for k, tm in ((k1, (tl1 + tl2) / 2 + tsd), (k2, (tu1 + tu2) / 2 + tsd)):
                i = bisect.bisect_left(edges, tm)
                if i < len(edges):
                    out[j, i] += k * θ
                    n_dep += 1
    out[:-1, :] /= (g_grid[1:] + g_grid[:-1])[:, None]
    return out / out[:-1, :].sum(), n_dep


# ---------------------------------------------------------------------------------------------------------------
# comparison rules
# ---------------------------------------------------------------------------------------------------------------
def line_error(got, want):
    """largest difference in units of the peak"""
    assert got.shape == want.shape and np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def lag_error(got, want, n_deposits, tol=TOL):
    """(largest difference in units of the peak outside moved deposits, number of moved deposits).  A cell may differ by
    more than `tol` only as one of an adjacent pair in the same g row whose sum agrees within `tol` -- one deposit that a
    rounding of its arrival time put on the other side of a t edge -- and at most one such pair per 10⁵ deposits (rounded
    up) may occur; anything else fails here."""
    assert got.shape == want.shape and np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    peak = float(np.max(np.abs(want)))
    d = (got - want) / peak
    bad = np.abs(d) > tol
    pairs = 0
    for j, i in zip(*np.nonzero(bad)):
        if not bad[j, i]:
            continue                                      # the partner of a pair already counted
        assert i + 1 < d.shape[1] and bad[j, i + 1], f"cell ({j}, {i}) differs by {d[j, i]:.3e} of the peak with no moved neighbour"
        assert abs(d[j, i] + d[j, i + 1]) <= tol, f"cells ({j}, {i}), ({j}, {i + 1}): pair sum differs by {d[j, i] + d[j, i + 1]:.3e}"
        bad[j, i] = bad[j, i + 1] = False
        d[j, i] = d[j, i + 1] = 0.0
        pairs += 1
    assert pairs <= math.ceil(n_deposits / 1e5), f"{pairs} moved deposits among {n_deposits}"
    return float(np.max(np.abs(d))), pairs
