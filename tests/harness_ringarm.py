"""ctypes binding of tests/host_harness_ringarm.cpp -- gr_ringarm.hpp, the arithmetic of gr_ring_rays / gr_ring_arms, compiled for
the host with g++ -- and what the CPU and the GPU tests of the ring-arm producer share: the scenes, a tracer built on the oracle
(`tracer(ring, slice, angles) -> rows`, the signature corona_arms' lock-step route drives) and the flat-space closed form."""
import ctypes as C
import functools
import math

import numpy as np

import hostbuild
from test_flat_space_exact import cartesian

HIT = 2


def lib():
    L = hostbuild.load("host_harness_ringarm.cpp", flags=["-ffp-contract=off"])
    L.hring_invphi.restype = C.c_double
    L.hring_bracket.restype = C.c_int
    L.hring_update.restype = C.c_int
    return L


def form_rays(frame, β, θ):
    """(v (n, 4), f (n,)) from the header"""
    frame, θ = np.ascontiguousarray(frame, dtype=np.float64), np.ascontiguousarray(θ, dtype=np.float64)
    v, f = np.zeros((θ.size, 4)), np.zeros(θ.size)
    lib().hring_form_rays(C.c_void_p(frame.ctypes.data), C.c_double(β), C.c_void_p(θ.ctypes.data), C.c_int64(θ.size), C.c_void_p(v.ctypes.data),
                          C.c_void_p(f.ctypes.data))
    return v, f


def bracket(rows, angles, target):
    """(a, b, best) from the header, or None"""
    rows, angles = np.ascontiguousarray(rows, dtype=np.float64), np.ascontiguousarray(angles, dtype=np.float64)
    out = np.zeros(3)
    ok = lib().hring_bracket(C.c_void_p(rows.ctypes.data), C.c_void_p(angles.ctypes.data), C.c_int(angles.size), C.c_int(target),
                             C.c_void_p(out.ctypes.data))
    return tuple(out.tolist()) if ok else None


class HarnessSearch:
    """gr_ring::Search through the harness, with GoldenSearch's interface (corona.py)"""

    def __init__(self, a, b, best, target):
        self.state = np.array([a, b, best, 0.0, 0.0, 0.0, 0.0])
        self.target = target

    def probes(self):
        cd = np.zeros(2)
        lib().hring_probes(C.c_void_p(self.state.ctypes.data), C.c_void_p(cd.ctypes.data))
        return float(cd[0]), float(cd[1])

    def update(self, extrema_iter, c_status, c_ρ, d_status, d_ρ):
        return lib().hring_update(C.c_void_p(self.state.ctypes.data), C.c_int(self.target), C.c_int(extrema_iter), C.c_int(c_status),
                                  C.c_double(c_ρ), C.c_int(d_status), C.c_double(d_ρ))

    def astuple(self):
        s = self.state
        return (float(s[0]), float(s[1]), float(s[2]), int(s[3]), int(s[4]), bool(s[5]), bool(s[6]))


def state_of(search):
    """a GoldenSearch as HarnessSearch.astuple gives it"""
    return (search.a, search.b, search.best, search.n, search.iters, bool(search.too_many), bool(search.done))


# ---------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------
KERR_A = 0.9


def kerr_scene(G, radii=(8.0,), h=3.0, r_out=200.0):
    """(metric, disc, [RingCorona ...]): co-rotating rings above a Kerr a = 0.9 hole"""
    m = G.KerrMetric(1.0, KERR_A)
    return m, G.ThinDisc(0.0, r_out), [G.RingCorona(G.SourceVelocities.co_rotating, r, h) for r in radii]


def flat_scene(G):
    """flat space (M = 0), a stationary ring (r = 8, h = 6): every ray is a straight line"""
    m = G.KerrMetric(0.0, 0.0)
    return m, G.ThinDisc(0.0, 200.0), [G.RingCorona(G.SourceVelocities.stationary, 8.0, 6.0)], G.PolarChart(0.0, 12000.0)


FLAT_βS = np.array([0.0, 0.7, 2.0])
FLAT_LAMBDA = 1_000_000.0


class OracleTracer:
    """`tracer(ring, slice, angles) -> rows (g, ρ, t, status)` on the CPU oracle: rays formed in numpy (corona.ring_velocities), traced
    by oracle.trace, g = energy_ratio against the ring's source velocity and `disc_velocity` in numpy.  Keeps what it traced."""

    def __init__(self, G, oracle, m, ocfg, models, βs, disc_velocity=None):
        self.G, self.oracle, self.m, self.ocfg, self.βs = G, oracle, m, ocfg, np.asarray(βs, dtype=np.float64)
        _, self.xs, self.v_src = G.corona.ring_frames(m, models)
        self.disc_velocity = disc_velocity
        self.calls = []                                    # (ring, slice, angles, formed velocities, oracle points) per call

    def __call__(self, ring, slice_, angles):
        K = self.G.corona
        ring, slice_, angles = np.asarray(ring), np.asarray(slice_), np.asarray(angles, dtype=np.float64)
        vs = np.zeros((angles.size, 4))
        for r in np.unique(ring):
            for s in np.unique(slice_[ring == r]):
                sel = (ring == r) & (slice_ == s)
                vs[sel] = K.ring_velocities(self.m, self.xs[r], self.v_src[r], self.βs[s], angles[sel])
        pts = self.oracle.trace(self.ocfg, np.ascontiguousarray(self.xs[ring]), vs)
        rows = np.zeros((angles.size, 4))
        hit = pts["status"] == HIT
        rows[:, 0] = np.nan
        if self.disc_velocity is not None and hit.any():
            with np.errstate(all="ignore"):
                rows[hit, 0] = K.energy_ratio(self.m, pts[hit], self.v_src[ring[hit]], self.disc_velocity(pts["x"][hit]))
        rows[:, 1] = pts["x"][:, 1] * np.abs(np.sin(pts["x"][:, 2]))
        rows[:, 2] = pts["x"][:, 0]
        rows[:, 3] = pts["status"]
        self.calls.append((ring, slice_, angles, vs, pts))
        return rows


def oracle_disc_velocity(G, oracle, m, ocfg):
    """_keplerian_velocity_projector with the ORACLE's plunging table (the package traces its own on the device)"""
    return G.corona.keplerian_velocity_projector(m, plunging=oracle.plunging_table(ocfg, m.isco()))


def flat_closed_form(x, v, gtol=1e-2, disc=(0.0, 200.0), lam_max=FLAT_LAMBDA):
    """The thin-disc event of straight lines in flat space: from position x (n, 4) along the formed velocity v (n, 4) to the first
    crossing of the |cos θ| = gtol cone -- the quadratic of tests/test_flat_space_exact.py::check_straight_lines on that file's
    `cartesian`.  Returns (ρ, t, usable): usable = the crossing exists inside the disc's radial range and before λmax, and the segment
    from the source to it stays more than 1 away from the z axis."""
    X0, V0 = cartesian(x, v, 0.0)
    g2 = gtol * gtol
    A = V0[:, 2] ** 2 - g2 * np.sum(V0 * V0, axis=1)
    B = 2 * (X0[:, 2] * V0[:, 2] - g2 * np.sum(X0 * V0, axis=1))
    Cq = X0[:, 2] ** 2 - g2 * np.sum(X0 * X0, axis=1)
    disc_ = B * B - 4 * A * Cq
    with np.errstate(invalid="ignore", divide="ignore"):
        r1 = (-B - np.sqrt(disc_)) / (2 * A)
        r2 = (-B + np.sqrt(disc_)) / (2 * A)
        lo, hi = np.minimum(r1, r2), np.maximum(r1, r2)
        first = np.where(lo > 0, lo, hi)
        Xh = X0 + V0 * first[:, None]
        ρ = np.hypot(Xh[:, 0], Xh[:, 1])
        # closest approach of the segment [0, first] to the z axis
        D2 = np.sum(V0[:, :2] ** 2, axis=1)
        s = np.clip(-np.sum(X0[:, :2] * V0[:, :2], axis=1) / D2, 0.0, first)
        P = X0[:, :2] + V0[:, :2] * s[:, None]
        clear = np.hypot(P[:, 0], P[:, 1]) > 1.0
        usable = (disc_ > 0) & (first > 0) & (first < lam_max) & (ρ >= disc[0]) & (ρ <= disc[1]) & clear
    # dt/dλ = v^t of the null ray = |V|
    return ρ, x[:, 0] + np.linalg.norm(V0, axis=1) * first, usable


@functools.lru_cache(maxsize=None)
def flat_base_angles(G):
    a = G.corona.ring_base_angles(100, 10)
    a.setflags(write=False)
    return a


def check_flat_rows(G, rows, x, v, rtol=2e-7):
    """ρ and t of the rows that hit against the closed form; returns the number compared"""
    ρ, t, usable = flat_closed_form(x, v)
    sel = usable & (rows[:, 3].astype(int) == HIT)
    np.testing.assert_allclose(rows[sel, 1], ρ[sel], rtol=rtol)
    np.testing.assert_allclose(rows[sel, 2], t[sel], rtol=rtol)
    return int(sel.sum())
