"""The scenes, media, rays and bounds that pin TraceRadiativeTransfer -- the ray that carries an intensity THROUGH a thick disc --
against an independent integration (tests/independent/transfer_dop853.py -> tests/golden/transfer_independent.json), for the host
build of the kernel text (tests/test_transfer_host.py over tests/host_harness_transfer.cpp) and for the device
(tests/test_gpu_transfer.py).  One table for both, so that the device is held to exactly what the CPU proved.

Scene A: Schwarzschild, observer r = 100, θ = 85°, λ1 = 200, the torus ThickDisc(ρ -> sqrt(1 - (ρ - 10)²) on [9, 11]).
Scene B: Kerr a = 0.9, ShakuraSunyaev(m), observer r = 100, θ = 75°, λ1 = 200 -- g_tϕ in the dot product and in the fluid velocity.
The rays of a scene are EVERY ray the generator kept (its selection rule is its own: even crossing count, every crossing with
|dc/dλ| > 0.05, chord > 0.2, and every ray that never crosses); no test leaves one out.

BOUNDS.  None is taken from the issue; each is ten times a figure measured on the host build at abstol = reltol = 1e-9 and written
down in DESIGN_measurements.md (§M40), and GOLDEN_BOUND may not exceed 1e-5:
  GOLDEN_BOUND       largest deviation(I, I_golden) over every ray, medium and scene: measured 6.9e-7 (scene A, emission only;
                     per scene and medium between 1.3e-8 and 6.9e-7 -- the size of the project's end-point bound, 1e-6: I follows
                     the chord, the chord the crossing points)
  SUPERPOSITION_BOUND largest deviation from I = S + (I0 - S) I_abs / I0_abs, relative to S: measured 5.3e-11 (scene B; A: 2.1e-12)
deviation() is relative, |I - I_g| / |I_g|, down to |I_g| = INTENSITY_FLOOR = 1e-3 and on the absolute scale 1e-3 below it.  Why:
the integrator -- the reference's as much as this one -- controls the local error of I on the scale abstol + reltol |I| =
1e-9 (1 + |I|), so an intensity of size |I| < 1 is resolved relatively to 1e-9 / |I| per step only, and not at all once it is below
abstol.  Scene B's absorption-only medium (a0 = 0.3 through a disc several M thick) takes 61 of its 139 rays below 1e-3, down to
e^-27 = 1.7e-12: their PURE relative deviation reaches 4.5e-3 there (2.3e-5 at I = 9e-10, 3.3e-8 at I = 2.5e-3), their absolute
deviation stays below 5.3e-10.  No ray is left out: the faint ones are held to 1e-3 GOLDEN_BOUND absolute.
The torus is handed to the device as a table of 2^20 samples over [9, 11] (linear interpolation: its height is off by at most
(Δρ)² f'' / 8 = 5e-13 f''), so that the table is no part of what the bounds measure.
"""
import ctypes as C
import json
import math
import os

import numpy as np

import hostbuild

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "transfer_independent.json")
TOL = 1e-9
GOLDEN_MEASURED = 6.9e-7
GOLDEN_BOUND = 10 * GOLDEN_MEASURED
assert GOLDEN_BOUND <= 1e-5
SUPERPOSITION_MEASURED = 5.3e-11
SUPERPOSITION_BOUND = 10 * SUPERPOSITION_MEASURED
EQUILIBRIUM_BOUND = 1e-12          # I0 = S: dI/dλ = s a_ν (S - I) is zero to rounding all the way
MAX_CROSSINGS = 64                 # Ray::kMaxCrossings
GR_FLAG_MAXITERS, GR_FLAG_NAN = 1, 4
TORUS_SAMPLES = 1 << 20
INTENSITY_FLOOR = 1e-3


def deviation(I, ref):
    """|I - ref| / max(|ref|, INTENSITY_FLOOR) per ray (the module's docstring says why there is a floor); NaN counts as inf"""
    d = np.abs(np.asarray(I) - np.asarray(ref)) / np.maximum(np.abs(ref), INTENSITY_FLOOR)
    return np.where(np.isnan(d), np.inf, d)

_cache = {}


def golden():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = json.load(f)
    return _cache["golden"]


def rays(name):
    """(α, β) of every fixture ray of scene `name`, and the golden's records in the same order"""
    rs = golden()["scenes"][name]["rays"]
    return np.array([r["alpha"] for r in rs]), np.array([r["beta"] for r in rs]), rs


def golden_intensity(name, medium):
    return np.array([r["I"][medium] if r["crossings"] else golden()["media"][medium]["I0"] for r in rays(name)[2]])


def _torus(rho):
    return math.sqrt(max(1.0 - (rho - 10.0) ** 2, 0.0)) if 9.0 <= rho <= 11.0 else -1.0


def setup(G, name):
    """(metric, observer position, geometry, λ1) of a scene: built once per session, read-only"""
    key = ("setup", name)
    if key not in _cache:
        sc = golden()["scenes"][name]["scene"]
        m = G.KerrMetric(1.0, sc["a"])
        x = np.array([0.0, sc["r_obs"], sc["th_obs"], 0.0])
        if name == "A":
            d = G.ThickDisc(_torus, ρ_range=(9.0, 11.0), samples=TORUS_SAMPLES)
        else:
            d = G.ShakuraSunyaev.for_metric(m)
        _cache[key] = (m, x, d, sc["lambda1"])
    return _cache[key]


def medium_trace(G, md):
    """TraceRadiativeTransfer of a medium given as the golden's dict (nu0, I0, a0, j0, pa, pj, sa, sj)"""
    return G.TraceRadiativeTransfer(ν=md["nu0"], I0=md["I0"],
                                    medium=G.PowerLawMedium(a0=md["a0"], j0=md["j0"], pa=md["pa"], pj=md["pj"], sa=md["sa"], sj=md["sj"]))


def configuration(G, name, trace, alpha, beta, **kw):
    """the tracing configuration of rays (α, β) of a scene under `trace` (None: the plain trace)"""
    from gradus_jl_amd.tracing import map_impact_parameters

    m, x, d, lam = setup(G, name)
    v = map_impact_parameters(m, x, np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64))
    kw.setdefault("abstol", TOL)
    kw.setdefault("reltol", TOL)
    return G.tracing_configuration(m, x, v, d, lam, trace=trace, **kw)


# ---- the host build of the flavour (tests/host_harness_transfer.cpp) ----
def lib():
    L = hostbuild.load("host_harness_transfer.cpp")
    L.hhr_transfer_endpoints.restype = C.c_int64
    L.hhr_transfer_render.restype = C.c_int64
    return L


def host_endpoints(G, config):
    """(records, intensities, passes through the step loop, crossings) per ray, from the host build"""
    cfg, tr = config.abi_config(), config.abi_transfer()
    v = np.ascontiguousarray(config.velocity, dtype=np.float64)
    x = np.ascontiguousarray(config.position, dtype=np.float64)
    n = v.shape[0]
    out = np.zeros(n, dtype=G._lib.POINT_DTYPE)
    inten, iters, ncross = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
    rc = lib().hhr_transfer_endpoints(C.byref(cfg), C.byref(tr), C.c_void_p(x.ctypes.data), C.c_int64(0), C.c_void_p(v.ctypes.data),
                                      C.c_int64(n), C.c_void_p(out.ctypes.data), C.c_void_p(inten.ctypes.data),
                                      C.c_void_p(iters.ctypes.data), C.c_void_p(ncross.ctypes.data))
    assert rc >= 0, rc
    return out, inten, iters, ncross


def host_scene(G, name, md):
    """host_endpoints of every fixture ray of a scene under a medium: computed once per (scene, medium), read-only"""
    key = ("host", name, json.dumps(md, sort_keys=True))
    if key not in _cache:
        al, be, _ = rays(name)
        _cache[key] = host_endpoints(G, configuration(G, name, medium_trace(G, md), al, be))
    return _cache[key]


def superposition_media(S=1.0 / 3.0):
    """an equilibrium medium (sj = sa - 3, pj = pa, S = j0 / a0) started off equilibrium, and the absorption-only medium of the
    same a_ν: the linear equation dI/dλ = s a_ν (S - I) gives I = S + (I0 - S) I_abs / I0_abs"""
    a0 = 0.3
    eq = dict(nu0=1.0, I0=1.0, a0=a0, j0=S * a0, pa=1.0, pj=1.0, sa=2.0, sj=-1.0)
    ab = dict(nu0=1.0, I0=0.8, a0=a0, j0=0.0, pa=1.0, pj=0.0, sa=2.0, sj=0.0)
    return eq, ab, S


def grazing_beta(G, alpha=1e-3):
    """β of the ray at `alpha` of scene A that is TANGENT to the torus, by bisection on "does the host build see a crossing": the
    upper edge of the torus's silhouette on that column.  Returns (β just crossing, β just missing), one ulp-scale bracket apart."""
    key = ("graze", alpha)
    if key not in _cache:
        trace = G.TraceRadiativeTransfer(I0=1.0)

        def crosses(b):
            return int(host_endpoints(G, configuration(G, "A", trace, [alpha], [b]))[3][0]) > 0

        grid = np.linspace(0.0, 6.0, 61)
        hit = [crosses(b) for b in grid]
        k = max(i for i in range(len(grid) - 1) if hit[i] and not hit[i + 1])
        lo, hi = float(grid[k]), float(grid[k + 1])
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if mid <= lo or mid >= hi:
                break
            if crosses(mid):
                lo = mid
            else:
                hi = mid
        _cache[key] = (lo, hi)
    return _cache[key]


def grazing_rays(G, alpha=1e-3):
    """rays around the tangent one: the bracket itself and steps of 1e-13 ... 1e-6 to both sides of it"""
    lo, hi = grazing_beta(G, alpha)
    offs = [0.0] + [s * 10.0 ** e for e in range(-13, -5) for s in (-1.0, 1.0)]
    be = np.array([lo + o for o in offs] + [hi + o for o in offs])
    return np.full(be.shape, alpha), be
