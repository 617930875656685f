"""ctypes binding of tests/host_harness_tftd.cpp -- gr_tftd.hpp, the arithmetic of gr_tf_lagtransfer_td, compiled for the host
with g++ -- and what the CPU and the GPU tests of the time-dependent lag integral share: synthetic ring and disc profiles from
closed forms, an independent scalar restatement of ring.jl:857-950 over radial.jl:171-324, the shapes, and the host route's
results on them (computed once per process)."""
import bisect
import ctypes as C
import functools
import math

import numpy as np

import harness_tfint as H
import hostbuild

TOL = H.TOL
N_RADII = 37                                                  # annuli: neither a multiple of the wave count nor of the chunk


def lib():
    L = hostbuild.load("host_harness_tftd.cpp", flags=["-ffp-contract=off"])
    L.htftd_lagtransfer.restype = C.c_int64
    L.htftd_rank.restype = C.c_int
    L.htftd_time_sample.restype = C.c_double
    return L


class Call:
    """The harness with the argument list transfer_functions._integrate_lagtransfer_td_device gives its `call`"""

    def __init__(self):
        self.deposits = 0

    def __call__(self, s, p, q, g, n_g, t, n_t, upscale, n_time, t0, out, em):
        self.deposits = lib().htftd_lagtransfer(s, p, q, C.c_void_p(g), C.c_int64(n_g), C.c_void_p(t), C.c_int64(n_t), C.c_int64(upscale),
                                                C.c_int64(n_time), C.c_double(t0), C.c_void_p(out), C.c_void_p(em))


def harness_lagtransfer(TF, prof, tfs, g_grid, t_grid, *, t0, g_grid_upscale, n_time_steps, n_radii=N_RADII, h=1e-8, quadrature_points=7):
    """(flux, number of deposits, em table) from the g++ build of the header"""
    c, em = Call(), []
    flux = TF._integrate_lagtransfer_td_device(prof, tfs, g_grid, t_grid, rmin=None, rmax=None, g_scale=1.0, h=h, n_radii=n_radii,
                                               quadrature_points=quadrature_points, t0=t0, g_grid_upscale=g_grid_upscale,
                                               n_time_steps=n_time_steps, call=c, em_out=em)
    return flux, c.deposits, em[0]


def host_lagtransfer(TF, prof, tfs, g_grid, t_grid, *, t0, g_grid_upscale, n_time_steps, n_radii=N_RADII):
    """(flux, number of deposits) of the host route"""
    n = []
    flux = TF._integrate_lagtransfer_td(prof, tfs, g_grid, t_grid, rmin=None, rmax=None, g_scale=1.0, h=1e-8, n_radii=n_radii,
                                        quadrature_points=7, t0=t0, g_grid_upscale=g_grid_upscale, n_time_steps=n_time_steps, _deposits=n)
    return flux, n[0]


# ---------------------------------------------------------------------------------------------------------------
# inputs: closed forms.  A ring of radius R at height 5 lights the disc point (ρ, azimuth β away) after
# t = sqrt(25 + ρ² + R² - 2 ρ R cos β); a slice is that curve on a few knots of ρ, its ε a smooth positive function.
# ---------------------------------------------------------------------------------------------------------------
HEIGHT = 5.0


def _curve(R, β, r_lo, r_hi, n_knots):
    ρ = r_lo * (r_hi / r_lo) ** (np.arange(n_knots) / (n_knots - 1))
    t = np.sqrt(HEIGHT ** 2 + ρ ** 2 + R ** 2 - 2.0 * ρ * R * np.cos(β))
    ε = (1.0 + 0.3 * np.cos(β)) * (HEIGHT ** 2 + ρ ** 2) ** -1.5
    return ρ, t, ε


def _arm(G, R, side, ranges, tie=None):
    """an arm of len(ranges) slices; slice j covers ranges[j] = (r_lo, r_hi) on 5 + j % 4 knots.  tie = (j, k): slice k gets
    slice j's (ρ, t) curve with another ε"""
    n = len(ranges)
    βs = (np.arange(n) + 0.5) / n * math.pi + (math.pi if side == "right" else 0.0)
    curves = [_curve(R, β, lo, hi, 5 + j % 4) for j, (β, (lo, hi)) in enumerate(zip(βs, ranges))]
    if tie is not None:
        j, k = tie
        curves[k] = (curves[j][0].copy(), curves[j][1].copy(), 1.7 * curves[j][2])
    return G.TimeDependentRadialDiscProfile(np.ones(n), [c[0] for c in curves], [c[1] for c in curves], [c[2] for c in curves])


def ring_profile(G):
    """one ring: an arm of 2 slices and one of 70 (past a wave).  Every slice covers the whole disc but slice 41 of the
    right arm, which ends at ρ = 30: beyond it that arm is switched off by a single missing slice."""
    right = [(1.0, 60.0)] * 70
    right[41] = (1.0, 30.0)
    return G.RingCoronaProfile(_arm(G, 3.0, "left", [(1.0, 60.0)] * 2), _arm(G, 3.0, "right", right))


def delay(radius):
    return 0.35 * radius + 0.125


@functools.lru_cache(maxsize=None)
def _disc_profile(G):
    ring0 = ring_profile(G)
    # ring 1: an arm of 1024 slices (the most an arm may have) and one of 5; no slice reaches below ρ = 3 or beyond 25, so
    # there every slice of the ring is missing and its limits are (0, 0)
    ring1 = G.RingCoronaProfile(_arm(G, 4.5, "left", [(3.0, 20.0 + 5.0 * (j % 7) / 7.0) for j in range(1024)]),
                                _arm(G, 4.5, "right", [(3.0, 21.0 + j) for j in range(5)]))
    # ring 2: ragged ranges, and two slices of the left arm with the same (ρ, t) curve: a tie in t, a knot interval of width 0
    ring2 = G.RingCoronaProfile(_arm(G, 6.0, "left", [(1.0 + 0.1 * j, 40.0 - j) for j in range(9)], tie=(3, 4)),
                                _arm(G, 6.0, "right", [(1.2, 55.0 - 2.0 * j) for j in range(12)]))
    return G.DiscCoronaProfile(np.array([3.0, 4.5, 6.0]), [ring0, ring1, ring2], delay)


def disc_profile(G):
    """three rings with nonzero delays; arms of 2, 70, 1024, 5, 9 and 12 slices.  Read-only."""
    return _disc_profile(G)


# shapes: (g grid, t grid).  20 x 48 bins: the accumulators fit LDS; 70 x 40 = 2800 cells > 2560: global accumulators and more
# g bins than a wave has lanes; a t grid that ends at 75, before the latest arrivals: deposits are dropped
T0 = 3.0
G_SMALL, T_SMALL = np.linspace(0.3, 1.3, 21), math.sqrt(2.0) + 44.0 + np.linspace(0.0, 120.0, 49)
G_WIDE, T_WIDE = np.linspace(0.1, 1.5, 71), math.sqrt(2.0) + 44.0 + np.linspace(0.0, 120.0, 41)
T_EARLY = math.sqrt(2.0) + 44.0 + np.linspace(0.0, 30.0, 49)
GRIDS = {"20x48": (G_SMALL, T_SMALL), "70x40": (G_WIDE, T_WIDE), "early": (G_SMALL, T_EARLY)}
# (grid, n_time, g_upscale): n_time 2, 33 and 100, g_upscale 1 and 3, on both sides of the accumulators' threshold
CASES = [("20x48", 100, 1), ("20x48", 33, 3), ("70x40", 33, 1), ("70x40", 2, 3), ("early", 33, 1)]


@functools.lru_cache(maxsize=None)
def branches(TF):
    return H.synthetic_branches(TF)


@functools.lru_cache(maxsize=None)
def host_case(G, kind, grid, n_time, upscale):
    """(flux, deposits) of the host route for a profile kind ('disc' | 'ring') and a case.  Read-only."""
    TF = G.transfer_functions
    prof = disc_profile(G) if kind == "disc" else ring_profile(G)
    g, t = GRIDS[grid]
    flux, n = host_lagtransfer(TF, prof, branches(TF), g, t, t0=T0, g_grid_upscale=upscale, n_time_steps=n_time)
    flux.setflags(write=False)
    return flux, n


@functools.lru_cache(maxsize=None)
def host_table(G, kind, n_time):
    TF = G.transfer_functions
    prof = disc_profile(G) if kind == "disc" else ring_profile(G)
    tfs = branches(TF)
    radii = np.asarray(G.GeometricGrid()(tfs.inner_radius(), tfs.outer_radius(), N_RADII))
    table = TF.time_dependent_emissivity_table(prof, radii, n_time)
    table.setflags(write=False)
    return radii, table


def coverage(G, prof, radii):
    """what the slices' ranges do at the annuli, from the host route's types alone: (annuli where both arms of some ring are
    active, annuli where an arm is switched off by exactly one missing slice, annuli where every slice of some ring is missing)"""
    rings = prof.rings if hasattr(prof, "rings") else [prof]
    both = one_missing = ring_missing = 0
    for ρ in radii:
        b = o = m = False
        for ring in rings:
            nans = [int(np.isnan(arm._knots(ρ)[0]).sum()) for arm in (ring.left_arm, ring.right_arm)]
            sizes = [len(arm.radii) for arm in (ring.left_arm, ring.right_arm)]
            b |= nans == [0, 0]
            o |= 1 in nans
            m |= nans == sizes
            if nans == sizes:
                assert ring.emissivity_interp_limits(ρ) == (0.0, 0.0)
            for arm, n in zip((ring.left_arm, ring.right_arm), nans):
                if n:                                        # an arm with a missing slice is 0 at every time
                    f = arm.emissivity_interp(ρ)
                    assert np.isnan(f.t[-1])
        both, one_missing, ring_missing = both + b, one_missing + o, ring_missing + m
    return both, one_missing, ring_missing


def em_error(got, want):
    """(limits equal bit for bit?, largest relative difference of the ε(time) values; a 0 of the table has to be 0)"""
    assert got.shape == want.shape and np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    same = got[:, :2].tobytes() == want[:, :2].tobytes()
    a, b = got[:, 2:], want[:, 2:]
    zero = b == 0.0
    assert np.all(a[zero] == 0.0)
    return same, float(np.max(np.abs(a[~zero] / b[~zero] - 1.0))) if np.any(~zero) else 0.0


# ---------------------------------------------------------------------------------------------------------------
# the third voice: radial.jl:171-324 and ring.jl:857-950 restated scalar by scalar from the profile's raw arrays
# ---------------------------------------------------------------------------------------------------------------
def _arm_knots(arm, ρ):
    ts, es = [], []
    for r, t, e in zip(arm.radii, arm.t, arm.ε):
        r = r.tolist()
        if r[0] <= ρ <= r[-1]:
            ts.append(H._nan_lerp(r, t.tolist(), ρ))
            es.append(H._nan_lerp(r, e.tolist(), ρ))
        else:
            ts.append(math.nan)
            es.append(math.nan)
    J = sorted(range(len(ts)), key=lambda i: (math.isnan(ts[i]), 0.0 if math.isnan(ts[i]) else ts[i]))      # stable, NaN last
    return [ts[i] for i in J], [es[i] for i in J]


def _arm_value(knots, x):
    ts, es = knots
    if x >= ts[0] and x <= ts[-1]:
        return _lerp_zero_width(ts, es, x)
    return 0.0


def _lerp_zero_width(t, u, x):
    """H._nan_lerp, with IEEE division where two knots coincide (python raises there)"""
    idx = min(max(bisect.bisect_right(t, x), 1), len(t) - 1) - 1
    w = H._div(x - t[idx], t[idx + 1] - t[idx])
    y = (1 - w) * u[idx] + w * u[idx + 1]
    if math.isnan(y):
        y = u[idx] if w < 0.5 else u[idx + 1]
        y = 0.0 if math.isnan(y) else y
    return y


def _arm_limits(knots):
    ts = [t for t in knots[0] if not math.isnan(t)]
    return (min(ts), max(ts)) if ts else (0.0, 0.0)


def restated_lagtransfer(prof, tfs, g_grid, t_grid, *, n_radii, t0, g_grid_upscale, n_time_steps, h=1e-8, quadrature_points=7):
    """(normalised flux, number of deposits): none of the package's code but np.linspace and the profile's arrays"""
    X, W = (a.tolist() for a in np.polynomial.legendre.leggauss(quadrature_points))
    lo_r, hi_r = float(tfs.radii[0]), float(tfs.radii[-1])
    K = (hi_r / lo_r) ** (1.0 / (n_radii - 1))
    radii = [lo_r * K ** i for i in range(n_radii)]
    if hasattr(prof, "rings"):
        rings = prof.rings
        δr = float(prof.radii[1]) - float(prof.radii[0])
        weights = [float(R) * δr for R in prof.radii]
        delays = [float(prof.propagation_velocity(float(R))) for R in prof.radii]
    else:
        rings, weights, delays = [prof], [1.0], [0.0]
    edges = t_grid.tolist()
    out = np.zeros((len(g_grid), len(t_grid)))
    n_dep = 0
    r_prev = lo_r - (radii[1] - lo_r)
    for r in radii:
        gmin, gmax, fields = H._branch_at(tfs, r)
        S = [H._ref_S(fields, ("lower",), gmin, gmax), H._ref_S(fields, ("upper",), gmin, gmax)]
        θ = (r - r_prev) * r * math.pi / (gmax - gmin)
        r_prev = r
        knots = [(_arm_knots(ring.left_arm, r), _arm_knots(ring.right_arm, r)) for ring in rings]
        a = b = None
        for (left, right), dt in zip(knots, delays):
            (l0, l1), (r0, r1) = _arm_limits(left), _arm_limits(right)
            lo, hi = min(l0, r0) + dt, max(l1, r1) + dt
            a, b = (lo, hi) if a is None else (min(a, lo), max(b, hi))
        δt = (b - a) / n_time_steps
        sample = np.linspace(a, b, n_time_steps).tolist()
        em = []
        for x in sample:
            total = 0.0
            for (left, right), dt, w in zip(knots, delays, weights):
                total += (_arm_value(left, x - dt) + _arm_value(right, x - dt)) * w
            em.append(total)

        def times(gs):
            gs = min(max(gs, 0.0), 1.0)
            tl, tu = fields[("lower", "t")], fields[("upper", "t")]
            if gs < h:
                ω, p, q = gs / h, tl(h), tu(h)
            elif gs > 1 - h:
                ω, p, q = 1 - (1 - gs) / h, tl(1 - h), tu(1 - h)
            else:
                return tl(gs), tu(gs)
            return p * ω + (1 - ω) * q, q * ω + (1 - ω) * p

        for j in range(len(g_grid) - 1):
            glo, ghi = min(max(float(g_grid[j]), gmin), gmax), min(max(float(g_grid[j + 1]), gmin), gmax)
            if glo == ghi:
                continue
            Δg = (ghi - glo) / g_grid_upscale
            for i in range(1, g_grid_upscale + 1):
                flo = glo + (i - 1) * Δg
                fhi = flo + Δg
                ks = [H._finite(H._ref_integrate_bin(S[c], flo, fhi, gmin, gmax, h, X, W)) for c in (0, 1)]
                (tl1, tu1), (tl2, tu2) = times((flo - gmin) / (gmax - gmin)), times((fhi - gmin) / (gmax - gmin))
                for k, tb in zip(ks, ((tl1 + tl2) / 2, (tu1 + tu2) / 2)):
                    for time, e in zip(sample, em):
                        cell = bisect.bisect_left(edges, tb + time - t0)
                        if cell < len(edges):
                            v = k * θ * e * δt
                            out[j, cell] += v
                            n_dep += v != 0.0
    out[:-1, :] /= (g_grid[1:] + g_grid[:-1])[:, None]
    return out / out[:-1, :].sum(), n_dep
