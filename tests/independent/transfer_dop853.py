#!/usr/bin/env python3
"""Covariant radiative transfer through an optically thick disc by an integrator that shares NOTHING with the package:
the yardstick of TraceRadiativeTransfer on the device (tests/test_transfer_host.py, tests/test_gpu_transfer.py).  The
reference records no value for this trace (src/tracing/radiative-transfer-problem.jl has no test with numbers).

What is independent here (the precedent is tests/independent/thick_disc_dop853.py):
  * equations of motion: Hamilton's equations in COVARIANT momenta for Kerr in Boyer-Lindquist coordinates,
    2 Σ H = Δ p_r² + p_θ² + (L - a E sin²θ)² / sin²θ - ((r² + a²) E - a L)² / Δ, hand-differentiated -- not the
    second-order Christoffel form;
  * stepper: scipy's DOP853, rtol = atol = 1e-12, dense output -- not Tsit5;
  * surface crossings: the distance to the disc is scanned on the dense output every Δλ = 0.002 and EVERY sign change
    is closed by brentq -- not the 8-samples-per-step search;
  * the intensity is integrated piecewise between crossings, dI/dλ = s (-a_ν I + j_ν / ν³) on the geodesic's dense
    output, again with DOP853 at 1e-12, and is constant outside the disc;
  * the fluid: Kerr's circular orbits in closed form, Ω = 1 / (ρ^(3/2) + a), u^t = (-g_tt - 2 g_tϕ Ω - g_ϕϕ Ω²)^(-1/2),
    and s = -p_μ u^μ = E u^t - L u^ϕ -- not the metric-Jacobian route of CircularOrbits.  Every kept ray stays outside
    the ISCO while it is inside the disc (asserted), so the plunging branch of fluid_velocity is never asked;
  * initial conditions: the zero-angular-momentum observer's tetrad of Kerr written out by hand.

Scene A: Schwarzschild, observer r = 100, θ = 85°, λ1 = 200, the torus ThickDisc(ρ -> sqrt(1 - (ρ - 10)²) on [9, 11]),
         rays α in linspace(-14, 14, 16) + 1e-3, β in linspace(-5, 5, 16) + 1e-3.
Scene B: Kerr a = 0.9, ShakuraSunyaev(m) (Ṁ/Ṁ_Edd = 0.3, η = 1 - E_isco), observer r = 100, θ = 75°, λ1 = 200,
         rays α in linspace(-12, 12, 12) + 1e-3, β in linspace(-8, 8, 12) + 1e-3.
Media (ν₀ = 1): emission only, absorption only, both with pa = pj = 1, and an equilibrium medium (sj = sa - 3,
pj = pa: dI/dλ = s a_ν (S - I), S = j0 / a0).

A ray is kept as a fixture if it never crosses, or if its crossing count is even, every crossing has |dc/dλ| > 0.05
and its chord inside the disc exceeds 0.2 in λ.  Run:  python tests/independent/transfer_dop853.py
(writes tests/golden/transfer_independent.json; a few minutes on 8 cores).
"""
from __future__ import annotations

import json
import math
import os
import sys
from multiprocessing import Pool

import numpy as np
from scipy.integrate import solve_ivp
from scipy.optimize import brentq

MEDIA = {
    "emission": dict(nu0=1.0, I0=0.0, a0=0.0, j0=0.1, pa=0.0, pj=0.0, sa=0.0, sj=0.0),
    "absorption": dict(nu0=1.0, I0=1.0, a0=0.3, j0=0.0, pa=0.0, pj=0.0, sa=0.0, sj=0.0),
    "both": dict(nu0=1.0, I0=0.5, a0=0.3, j0=0.1, pa=1.0, pj=1.0, sa=0.0, sj=0.0),
    "equilibrium": dict(nu0=1.0, I0=1.0, a0=0.3, j0=0.1, pa=1.0, pj=1.0, sa=2.0, sj=-1.0),
}
MEDIA_ORDER = ("emission", "absorption", "both", "equilibrium")
MIN_SLOPE, MIN_CHORD = 0.05, 0.2
SCAN = 0.002


def kerr_isco(a):
    z1 = 1.0 + (1.0 - a * a) ** (1.0 / 3.0) * ((1.0 + a) ** (1.0 / 3.0) + (1.0 - a) ** (1.0 / 3.0))
    z2 = math.sqrt(3.0 * a * a + z1 * z1)
    return 3.0 + z2 - math.sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2))


def make_scene(name):
    if name == "A":
        a = 0.0
        sc = dict(a=a, r_obs=100.0, th_obs=math.radians(85.0), lambda1=200.0, disc="torus",
                  alpha=(np.linspace(-14.0, 14.0, 16) + 1e-3).tolist(), beta=(np.linspace(-5.0, 5.0, 16) + 1e-3).tolist())
    else:
        a = 0.9
        sc = dict(a=a, r_obs=100.0, th_obs=math.radians(75.0), lambda1=200.0, disc="shakura_sunyaev",
                  alpha=(np.linspace(-12.0, 12.0, 12) + 1e-3).tolist(), beta=(np.linspace(-8.0, 8.0, 12) + 1e-3).tolist())
    isco = kerr_isco(a)
    sc["isco"] = isco
    sc["r_inner"] = 1.01 * (1.0 + math.sqrt(1.0 - a * a))      # the chart: 1.01 r₊
    e_isco = (1.0 - 2.0 / isco + a / isco ** 1.5) / math.sqrt(1.0 - 3.0 / isco + 2.0 * a / isco ** 1.5)
    sc["inv_eta"], sc["mdot"] = 1.0 / (1.0 - e_isco), 0.3
    return sc


def height(sc, rho):
    """cross_section of the scene's disc (<= 0: no disc there)"""
    rho = np.asarray(rho, dtype=np.float64)
    if sc["disc"] == "torus":
        x = rho - 10.0
        return np.where((rho < 9.0) | (rho > 11.0), -1.0, np.sqrt(np.maximum(1.0 - x * x, 0.0)))
    isco = sc["isco"]
    return np.where(rho < isco, -0.0, 3.0 * sc["inv_eta"] * sc["mdot"] * (1.0 - np.sqrt(isco / np.maximum(rho, 1e-300))))


def distance(sc, r, th):
    """distance_to_disc of a thick disc: 1 where the cross section is <= 0, else r |cos θ| - height"""
    rho = r * np.abs(np.sin(th))
    h = height(sc, rho)
    return np.where(h <= 0.0, 1.0, r * np.abs(np.cos(th)) - h)


# ---- Kerr, M = 1, in covariant momenta: y = (t, r, θ, ϕ, p_r, p_θ); p_t = -E, p_ϕ = L constant ----
def rhs(_, y, a, E, L):
    r, th, pr, pth = y[1], y[2], y[4], y[5]
    s, c = math.sin(th), math.cos(th)
    s2 = s * s
    r2a2 = r * r + a * a
    Sig = r * r + a * a * c * c
    Del = r2a2 - 2.0 * r
    W = L - a * E * s2
    P = r2a2 * E - a * L
    N = Del * pr * pr + pth * pth + W * W / s2 - P * P / Del
    dN_dr = 2.0 * (r - 1.0) * pr * pr - (4.0 * r * E * P * Del - P * P * 2.0 * (r - 1.0)) / (Del * Del)
    dN_dth = -2.0 * c * W * (L + a * E * s2) / (s2 * s)
    dS_dr, dS_dth = 2.0 * r, -2.0 * a * a * s * c
    return [(a * W + P * r2a2 / Del) / Sig, Del * pr / Sig, pth / Sig, (W / s2 + a * P / Del) / Sig,
            -dN_dr / (2.0 * Sig) + N * dS_dr / (2.0 * Sig * Sig), -dN_dth / (2.0 * Sig) + N * dS_dth / (2.0 * Sig * Sig)]


def metric_lower(a, r, th):
    s2, c2 = np.sin(th) ** 2, np.cos(th) ** 2
    Sig = r * r + a * a * c2
    Del = r * r - 2.0 * r + a * a
    gtt = -(1.0 - 2.0 * r / Sig)
    gtp = -2.0 * a * r * s2 / Sig
    gpp = (r * r + a * a + 2.0 * a * a * r * s2 / Sig) * s2
    return gtt, Sig / Del, Sig, gpp, gtp


def initial_state(sc, alpha, beta):
    """local_momentum (-1, p_r, β p_r / r, α p_r / r) through the zero-angular-momentum observer's tetrad, then the null
    constraint for v^t: returns y0, E, L."""
    a, r, th = sc["a"], sc["r_obs"], sc["th_obs"]
    gtt, grr, gthth, gpp, gtp = metric_lower(a, r, th)
    om = -gtp / gpp
    lapse = math.sqrt(-gtt + gtp * gtp / gpp)
    aa, bb = alpha / r, beta / r
    pr_loc = -1.0 / math.sqrt(1.0 + aa * aa + bb * bb)
    vr = pr_loc / math.sqrt(grr)
    vth = bb * pr_loc / math.sqrt(gthth)
    vph = aa * pr_loc / math.sqrt(gpp) - om / lapse
    # g_tt v^t² + 2 g_tϕ v^t v^ϕ + (g_rr v^r² + g_θθ v^θ² + g_ϕϕ v^ϕ²) = 0, the future-pointing root
    rest = grr * vr * vr + gthth * vth * vth + gpp * vph * vph
    vt = (-gtp * vph - math.sqrt(gtp * gtp * vph * vph - gtt * rest)) / gtt
    E = -(gtt * vt + gtp * vph)
    L = gtp * vt + gpp * vph
    return [0.0, r, th, 0.0, grr * vr, gthth * vth], E, L


def fluid_s(sc, r, th, E, L):
    """ds/dλ = -p_μ u^μ for the circular orbit at ρ = r |sin θ| in the equatorial plane, and ρ"""
    a = sc["a"]
    rho = r * abs(math.sin(th))
    Om = 1.0 / (rho ** 1.5 + a)
    gtt = -(1.0 - 2.0 / rho)
    gtp = -2.0 * a / rho
    gpp = rho * rho + a * a + 2.0 * a * a / rho
    ut = 1.0 / math.sqrt(-gtt - 2.0 * gtp * Om - gpp * Om * Om)
    return E * ut - L * Om * ut, rho


def trace_one(args):
    name, alpha, beta = args
    sc = make_scene(name)
    a = sc["a"]
    y0, E, L = initial_state(sc, alpha, beta)

    def horizon(_, y, *rest):
        return y[1] - sc["r_inner"]

    horizon.terminal = True
    horizon.direction = -1
    sol = solve_ivp(rhs, (0.0, sc["lambda1"]), y0, method="DOP853", rtol=1e-12, atol=1e-12, dense_output=True,
                    events=horizon, args=(a, E, L))
    lam_end = float(sol.t[-1])
    lam = np.arange(0.0, lam_end, SCAN)
    if lam.size == 0 or lam[-1] < lam_end:
        lam = np.append(lam, lam_end)
    Y = sol.sol(lam)
    c = distance(sc, Y[1], Y[2])

    def g(x):
        yy = sol.sol(x)
        return float(distance(sc, np.array([yy[1]]), np.array([yy[2]]))[0])

    sgn = np.sign(c)
    crossings = []
    for k in np.nonzero(sgn[1:] * sgn[:-1] < 0)[0]:
        lo, hi = float(lam[k]), float(lam[k + 1])
        glo, ghi = g(lo), g(hi)
        if abs(glo) == 1.0 or abs(ghi) == 1.0:
            s0 = np.sign(glo)      # the condition jumps (edge of the radial range): bisect on the sign alone
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                if np.sign(g(mid)) == s0:
                    lo = mid
                else:
                    hi = mid
            crossings.append(0.5 * (lo + hi))
        else:
            crossings.append(float(brentq(g, lo, hi, xtol=1e-14, rtol=1e-15)))
    slopes = [abs(g(x + 1e-5) - g(x - 1e-5)) / 2e-5 for x in crossings]
    out = {"alpha": alpha, "beta": beta, "lambda_end": lam_end, "captured": bool(sol.status == 1), "crossings": crossings,
           "min_slope": min(slopes) if slopes else None, "started_inside": bool(c[0] < 0.0)}
    # the inside segments: between crossing 2k and 2k + 1 (the ray starts outside)
    chord = 0.0
    I = np.array([MEDIA[mname]["I0"] for mname in MEDIA_ORDER])
    min_rho_inside = float("inf")
    ok = len(crossings) % 2 == 0 and not out["started_inside"]
    if ok:
        for k in range(0, len(crossings), 2):
            l0, l1 = crossings[k], crossings[k + 1]
            chord += l1 - l0

            def dI(x, Iv):
                yy = sol.sol(x)
                s, rho = fluid_s(sc, yy[1], yy[2], E, L)
                res = []
                for q, mname in enumerate(MEDIA_ORDER):
                    md = MEDIA[mname]
                    nu = md["nu0"] * s
                    an = md["a0"] * rho ** (-md["pa"]) * nu ** (-md["sa"])
                    jn = md["j0"] * rho ** (-md["pj"]) * nu ** (-md["sj"])
                    res.append(s * (-an * Iv[q] + jn / nu ** 3))
                return res

            seg = solve_ivp(dI, (l0, l1), I, method="DOP853", rtol=1e-12, atol=1e-12)
            I = seg.y[:, -1]
            xs = np.linspace(l0, l1, 64)
            yy = sol.sol(xs)
            min_rho_inside = min(min_rho_inside, float(np.min(yy[1] * np.abs(np.sin(yy[2])))))
    out["chord"] = chord
    out["min_rho_inside"] = min_rho_inside if crossings else None
    out["I"] = {mname: float(I[q]) for q, mname in enumerate(MEDIA_ORDER)} if ok else None
    out["kept"] = bool(len(crossings) == 0 or (ok and out["min_slope"] > MIN_SLOPE and chord > MIN_CHORD))
    return out


def main():
    out = {"generator": "tests/independent/transfer_dop853.py",
           "integrator": "scipy DOP853 rtol=atol=1e-12, Hamiltonian form; crossings by scan + brentq; I piecewise between crossings",
           "media": MEDIA, "media_order": MEDIA_ORDER, "min_slope": MIN_SLOPE, "min_chord": MIN_CHORD, "scenes": {}}
    for name, need, need4 in (("A", 40, 8), ("B", 30, 0)):
        sc = make_scene(name)
        jobs = [(name, float(al), float(be)) for al in sc["alpha"] for be in sc["beta"]]
        with Pool(min(8, os.cpu_count() or 1)) as pool:
            rays = pool.map(trace_one, jobs, chunksize=4)
        kept = [r for r in rays if r["kept"]]
        crossing = [r for r in kept if r["crossings"]]
        four = [r for r in crossing if len(r["crossings"]) >= 4]
        for r in crossing:
            assert r["min_rho_inside"] > sc["isco"], "a kept ray goes inside the ISCO while inside the disc"
        print(f"scene {name}: {len(rays)} rays, {sum(1 for r in rays if r['crossings'])} cross, kept {len(kept)} "
              f"({len(crossing)} crossing, {len(four)} with four or more crossings, "
              f"{sum(1 for r in crossing if r['captured'])} captured afterwards), "
              f"min |dc/dλ| kept {min(r['min_slope'] for r in crossing):.3f}, min chord {min(r['chord'] for r in crossing):.3f}")
        assert len(crossing) >= need and len(four) >= need4, (name, len(crossing), len(four))
        out["scenes"][name] = {"scene": sc, "n_traced": len(rays), "rays": kept}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "transfer_independent.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
