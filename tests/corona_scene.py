"""The sources, the reference and the criteria that pin a corona's energy ratio g = energy_ratio(source frame -> disc frame)
against the oracle (tests/test_corona_energy_host.py on the reference alone and on the host build of the kernel logic,
tests/test_gpu_corona_energy.py on the device): one table for both, so that the device is asked what the host was.

Two device paths form g (the third, the ring arms, is pinned by tests/test_gpu_ringarm.py):
  * one source velocity for the launch (pf->has_u_src; finalize in gr_device.hpp): RingCorona's representative point,
    BeamedPointSource -- here in motion, and in a metric that is not Kerr;
  * a source without one position (DiscCorona): 28 doubles per sample (gr_rayset.sky_rows), the static-observer ratio from the trace
    kernel times f = (u_cov . v) / (g_tμ v^μ) per ray (sky_sample, k_sky_scale_g).

The reference side has not been near the device: positions, directions and source velocities by corona.py's numpy
(sample_position_direction_velocity, pinned to the reference's goldens by tests/test_corona_host.py), the rays by the CPU oracle from
per-ray start positions, g by corona.energy_ratio against keplerian_velocity_projector with the ORACLE's plunging table -- the
construction of tests/test_corona_host.py::kerr_setup -- so that hits inside the ISCO are part of the comparison.  The device's point
function is handed the same table (`pointfunction`): inside the ISCO the comparison tests the kernel's reading of a table, not the
table's origin (the device-traced table is pinned by tests/test_gpu_redshift_metrics.py).

Criteria, none taken from the code under test:
  * MAX_STATUS_DIFF rays may end in another class (the cap of test_corona_rows_equal_oracle_traced_rays_and_their_energy_ratio on
    its 3000 rays; the host build of the kernel logic shows 0 on these rays); a set of more than 3000 rays is allowed the same
    share, 2 in 3000 (`max_status_diff`);
  * RTOL = 1e-6, the project's parity bar, on ρ, t and g of every common hit; hits inside the ISCO are a group of their own so that a
    failure there names the table path.  The reference's own spread inside the ISCO (oracle / its no-FMA build / host build of the
    kernel logic, tests/test_corona_energy_host.py) stays below INSIDE_SPREAD_LIMIT = 1e-7, so the same 1e-6 holds there;
  * MEDIAN_BOUND = 1e-9 on the median deviation of g: the README's every-pixel median against the oracle is 4.3e-11, the worst
    median between the kernel logic and the oracle on these rays is 1.5e-12; a wrong row or factor is an O(1) error and a factor
    from the neighbouring sample moves the median by per cent;
  * MIN_HITS / MIN_INSIDE hits per case, a spread of source radii and a sample next to the axis for the disc cases keep the
    comparisons from being vacuous.
"""
import numpy as np

N = 1500
DISC = (0.0, 200.0)
LAMBDA_MAX = 3000.0
HIT = 2                                       # StatusCodes.IntersectedWithGeometry
RTOL = 1e-6                                   # the project's parity bar (tests/test_gpu_parity.py)
MEDIAN_BOUND = 1e-9
MAX_STATUS_DIFF = 2
MIN_HITS, MIN_INSIDE = 600, 10
INSIDE_SPREAD_LIMIT = 1e-7                    # above it the inside-ISCO bar would be ten times the spread, and written down
STEADY_BOUND = 1e-8                           # oracle / no-FMA oracle / host build of the kernel logic: g from their end points
DECOMPOSITION_RTOL = 1e-12
CLOSEST_APPROACH = 1.000001                   # chart of the plunge (orbit-solving.jl:137-167)
F32_TOL = 1e-5

KERR = ("kerr", "KerrMetric", dict(M=1.0, a=0.9))
JOHANNSEN = ("johannsen", "JohannsenMetric", dict(M=1.0, a=0.6, alpha13=0.5, eps3=0.3))
# (id, (oracle name, class of the package, its arguments), source): a fresh model per call, so that both sides see the same draws
CASES = [
    ("disc-kerr-corotating", KERR, lambda G: G.DiscCorona(G.SourceVelocities.co_rotating, 6.0, 4.0, seed=17)),
    ("disc-kerr-stationary", KERR, lambda G: G.DiscCorona(G.SourceVelocities.stationary, 6.0, 4.0, seed=17)),
    ("disc-johannsen-corotating", JOHANNSEN, lambda G: G.DiscCorona(G.SourceVelocities.co_rotating, 8.0, 5.0, seed=3)),
    ("ring-kerr-corotating", KERR, lambda G: G.RingCorona(G.SourceVelocities.co_rotating, 8.0, 3.0)),
    ("beamed-johannsen", JOHANNSEN, lambda G: G.BeamedPointSource(8.0, 0.3)),
]
CASE_IDS = [c[0] for c in CASES]
DISC_CASES = [c for c in CASES if c[0].startswith("disc-")]
DISC_CASE_IDS = [c[0] for c in DISC_CASES]
CASE = {c[0]: c for c in CASES}

_cache = {}


def metric(G, case):
    _, cls, kw = case[1]
    return getattr(G, cls)(**kw)


def sampler(G):
    return G.EvenSampler(G.BothHemispheres(), G.GoldenSpiralGenerator())


def is_disc(case):
    return case[0].startswith("disc-")


def oracle_config(oracle, G, case, tol=None):
    tols = {} if tol is None else dict(abstol=tol, reltol=tol)
    return oracle.make_config(case[1][0], tuple(metric(G, case).abi_params()), disc=DISC, lambda_max=LAMBDA_MAX, upper_hemisphere=True, **tols)


def oracle_table(G, oracle, case):
    """(ISCO, plunging table) of the case's metric by the oracle: once per session, read-only."""
    key = ("table", case[1][0])
    if key not in _cache:
        m = metric(G, case)
        pcfg = oracle.make_config(case[1][0], tuple(m.abi_params()), mu=1.0, closest_approach=CLOSEST_APPROACH, lambda_max=50000.0)
        table = tuple(oracle.plunging_table(pcfg, m.isco()))
        for a in table:
            a.setflags(write=False)
        _cache[key] = (m.isco(), table)
    return _cache[key]


def samples(G, case, n):
    """(xs, vs, source velocities), each (n, 4), by the host sampler from a fresh model: once per session, read-only."""
    key = ("samples", case[0], n)
    if key not in _cache:
        out = G.corona.sample_position_direction_velocity(metric(G, case), case[2](G), sampler(G), n)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def energy_ratio(G, oracle, case, pts, vsrc):
    """g per ray (NaN where the ray did not meet the disc) from end-point records `pts`: corona.energy_ratio against `vsrc` (n, 4)
    and the disc velocity of keplerian_velocity_projector with the oracle's table."""
    K = G.corona
    m = metric(G, case)
    _, table = oracle_table(G, oracle, case)
    g = np.full(pts.shape[0], np.nan)
    hit = pts["status"] == HIT
    if hit.any():
        g[hit] = K.energy_ratio(m, pts[hit], np.asarray(vsrc)[hit], K.keplerian_velocity_projector(m, plunging=table)(pts["x"][hit]))
    return g


def summarise(G, oracle, case, pts, vsrc):
    """End-point records -> what a row of gr_ray_summary holds: status, ρ, t, g."""
    out = dict(status=pts["status"].astype(int), rho=pts["x"][:, 1] * np.abs(np.sin(pts["x"][:, 2])), t=pts["x"][:, 0].copy(),
               g=energy_ratio(G, oracle, case, pts, vsrc), pts=pts)
    for a in out.values():
        a.setflags(write=False)
    return out


def reference(G, oracle, case, n=N, tol=None, nofma=False):
    """status, ρ, t and g_ref per ray by the oracle (by its no-FMA build if asked; at its default tolerance, or `tol`): once per
    session, read-only."""
    key = ("reference", case[0], n, tol, nofma)
    if key not in _cache:
        xs, vs, vsrc = samples(G, case, n)

        def run():
            return oracle.trace(oracle_config(oracle, G, case, tol), np.ascontiguousarray(xs), np.ascontiguousarray(vs))

        if nofma:
            with oracle.nofma_library():
                pts = run()
        else:
            pts = run()
        _cache[key] = summarise(G, oracle, case, pts, vsrc)
    return _cache[key]


def pointfunction(G, oracle, case):
    """The device's redshift point function with the ORACLE's ISCO and table on its `extra`."""
    from gradus_jl_amd.pointfunctions import GR_PF_REDSHIFT, PointFunction

    isco, table = oracle_table(G, oracle, case)
    return PointFunction(None, device_pf=GR_PF_REDSHIFT, extra={"r_isco": isco, "plunge": table})


def launch(G, oracle, case, n, ens=None, tol=None, m=None):
    """What a device call of the case takes: (gr_config, gr_rayset, gr_pointfunction, keep-alive, the sampler's rows or None).
    Disc cases bring rows and leave has_u_src at 0; the others set u_src.  `m`: another metric object for the same source (a
    TabulatedMetric of the case's metric)."""
    from gradus_jl_amd.rendering import abi_pointfunction
    from gradus_jl_amd.tracing import tracing_configuration

    base = metric(G, case)
    m = base if m is None else m
    rs, keep, x, v_src = G.corona.sky_rayset(m, case[2](G), sampler(G), n)
    tols = {} if tol is None else dict(abstol=tol, reltol=tol)
    config = tracing_configuration(m, x, np.zeros((1, 4)), G.ThinDisc(*DISC), (0.0, LAMBDA_MAX), callback=G.domain_upper_hemisphere(),
                                   ensemble=ens, **tols)
    pf, keep_pf = abi_pointfunction(pointfunction(G, oracle, case))
    if np.ndim(v_src) == 1:
        pf.has_u_src = 1
        for q in range(4):
            pf.u_src[q] = v_src[q]
    rows = None if keep is None else keep[1]
    assert (rows is not None) == is_disc(case)
    cfg = config.abi_config()
    return cfg, rs, pf, (keep, keep_pf, config, v_src), rows


def device_rows(G, oracle, case, n, ens, kernel=2, precision=64, tol=None):
    """The (g, ρ, t, status) rows of gr_ray_summary for the case."""
    import ctypes as C

    from gradus_jl_amd import _lib

    ens.set("kernel", kernel).set("precision", precision)
    cfg, rs, pf, keep, _ = launch(G, oracle, case, n, ens, tol)
    rows = np.zeros((n, 4))
    _lib.check(_lib.load().gr_ray_summary(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), rows.ctypes.data, None))
    del keep
    return rows


def rel(a, b):
    return np.abs(a - b) / np.abs(b)


def compare(got, ref, isco):
    """`got` -- rows (g, ρ, t, status) or a dict of `summarise` -- against the reference: rays whose class differs, and over the
    common hits, inside and outside the ISCO (by the reference's ρ), the largest and the median relative deviation of g, ρ, t."""
    if not isinstance(got, dict):
        got = dict(g=got[:, 0], rho=got[:, 1], t=got[:, 2], status=got[:, 3].astype(int))
    hit = (got["status"] == HIT) & (ref["status"] == HIT)
    inside = hit & (ref["rho"] < isco)
    out = dict(status_diff=int(np.sum(got["status"] != ref["status"])), hits=int(hit.sum()), n_inside=int(inside.sum()),
               nan_g=int(np.isnan(got["g"][hit]).sum()), g_off_hits=int((~np.isnan(got["g"][got["status"] != HIT])).sum()))
    for name, sel in (("all", hit), ("inside", inside), ("outside", hit & ~inside)):
        for col in ("g", "rho", "t"):
            d = rel(got[col][sel], ref[col][sel])
            out[f"{col}_{name}_max"] = float(np.max(d)) if d.size else 0.0
            out[f"{col}_{name}_median"] = float(np.median(d)) if d.size else 0.0
    return out


def describe(label, s):
    parts = [f"{label}: statuses differ on {s['status_diff']}, common hits {s['hits']} ({s['n_inside']} inside the ISCO)"]
    for name in ("outside", "inside"):
        parts.append(f"    {name:8s}" + "  ".join(f"{col} max {s[f'{col}_{name}_max']:.3e} median {s[f'{col}_{name}_median']:.3e}" for col in ("g", "rho", "t")))
    return "\n".join(parts)


def max_status_diff(n):
    """MAX_STATUS_DIFF up to the 3000 rays of the test it comes from; the same share of a larger set."""
    return max(MAX_STATUS_DIFF, -(-MAX_STATUS_DIFF * n // 3000))


def check(s, label, n=N):
    """The criteria of the module docstring on a `compare` result over n rays."""
    print(describe(label, s))
    assert s["status_diff"] <= max_status_diff(n), label
    assert s["hits"] >= MIN_HITS - max_status_diff(n) and s["n_inside"] >= MIN_INSIDE - MAX_STATUS_DIFF, label
    assert s["nan_g"] == 0 and s["g_off_hits"] == 0, f"{label}: g is finite exactly on the hits"
    for col in ("rho", "t", "g"):
        assert s[f"{col}_outside_max"] <= RTOL, f"{label}: {col} outside the ISCO"
    for col in ("rho", "t", "g"):
        assert s[f"{col}_inside_max"] <= RTOL, f"{label}: {col} inside the ISCO (the plunging table's path)"
    assert s["g_all_median"] <= MEDIAN_BOUND, f"{label}: median deviation of g"


def f32_stats(g, status, ref, isco):
    """f32_scene's rule for g: (rays whose class differs from oracle@1e-9, median and 90th percentile of |g / g_ref - 1| over the
    common hits outside 1.05 r_ISCO, their number)."""
    hit = (status == HIT) & (ref["status"] == HIT) & (ref["rho"] > 1.05 * isco)
    d = rel(g[hit], ref["g"][hit])
    return dict(mism=int(np.sum(status != ref["status"])), median=float(np.median(d)), p90=float(np.percentile(d, 90)), hits=int(hit.sum()))
