"""The scene, the cases and the criteria that pin the REDSHIFT point function, the ISCO and the plunging table of every catalogue
metric that has an ISCO against the oracle (tests/test_redshift_metrics_host.py on the host builds of the kernel text,
tests/test_gpu_redshift_metrics.py on the device): one table for both, so that the device is asked what the host was.

The end-point tests (test_gpu_parity.py, test_gpu_f32_metrics.py) run the fused right-hand side `m.rhs` of each metric.  The
redshift runs on other code: `redshift_pf` -> `circular_fourvelocity` -> `metric_eval` -> `m.eval` (g, ∂ᵣg, g⁻¹) outside the
ISCO, and inside it a table made by a chain of its own (metrics.py `_components` -> generic_isco -> plunging_fourvelocity -> a
μ = 1 geodesic by k_trace_path -> LDS or global memory -> nan_linear_interp).  The scene reaches inside the ISCO of every case.

Criteria (each asserted by the tests, none taken from the code under test):
  * MIN_INSIDE / MIN_OUTSIDE common hits inside / outside the ISCO keep a comparison from being vacuous (the oracle alone has
    29 / 81 / 161 / 62 / 60 / 219 / 57 inside, in case order, and 1713 .. 2531 outside);
  * a rim ray that meets the disc at another crossing is a class flip of the kind DESIGN.md §4 describes: its end radius differs
    by more than R_AGREE, its redshift by up to 0.46.  `stats` leaves such pixels out AND counts them: at most MAX_LEFT_OUT of
    the common hits; the NaN pattern may differ in at most MAX_NAN_DIFF of the pixels (worst measured: Bumblebee, 13 of 4096);
  * outside the ISCO the project's RTOL (1e-6; Kerr-refractive 2e-4, the bound test_remaining_metrics_on_device_vs_oracle
    documents for its unresolved index step); inside it 10 x the oracle against its own `nofma` build (two roundings of one
    algorithm) with a floor of 1e-6: `nofma_floor`.  For Bumblebee that figure is 9e-2 (the stall of its table at
    the g_rr pole) and bounds nothing, so the same rule is applied once more to the hits on the table's clean
    rows (ρ >= R_FROM x the table's first radius), for every case.
"""
import math

import numpy as np

# (oracle name, parameters, class of the package); parameters of f32_scene.CASES where the case exists there
CASES = [
    ("kerr", (1.0, 0.9), "KerrMetric"),                                   # through the TABLE route; ROUTES adds the analytic one
    ("johannsen", (1.0, 0.7, 1.0, 0.5, -0.5, 1.0), "JohannsenMetric"),
    ("bumblebee", (1.0, 0.2, 0.3), "BumblebeeMetric"),
    ("kerr-newman", (1.0, 0.6, 0.5), "KerrNewmanMetric"),
    ("johannsen-psaltis", (1.0, 0.6, 1.0), "JohannsenPsaltisMetric"),
    ("dilaton-axion", (1.0, 0.5, 0.2, 0.8), "DilatonAxion"),
    ("kerr-refractive", (1.0, 0.6, 1.2, 20.0), "KerrRefractive"),
]
CASE_IDS = [c[0] for c in CASES]
# (id, case, reads the table): every case through interpolate_redshift's table, Kerr through its analytic plunge beside it
ROUTES = [(c[0], c, True) for c in CASES] + [("kerr-analytic", CASES[0], False)]
ROUTE_IDS = [r[0] for r in ROUTES]
# single precision at 1e-5: Kerr-refractive is left out because both the kernel text and the oracle@1e-5 sit at a median
# relative error of 0.30 against oracle@1e-9 there (nobody resolves the 2.5e-4-wide index step at that tolerance): "at most
# 1.5 x the baseline" would compare two wrong images
F32_CASES = [c for c in CASES if c[0] != "kerr-refractive"]
F32_CASE_IDS = [c[0] for c in F32_CASES]
# the two metrics whose g_rr has its pole ABOVE inner_radius(m) as the reference defines it: the plunge never gets
# to the chart's inner boundary, it stalls at the pole
STALLS = ("bumblebee", "dilaton-axion")

X_OBS = np.array([0.0, 1000.0, math.radians(70), 0.0])
DISC = (0.0, 25.0)
LAMBDA_MAX = 2000.0
W = H = 64
ALIMS, BLIMS = (-25.0, 25.0), (-15.0, 15.0)
TOL = 1e-9
F32_TOL = 1e-5
MIN_INSIDE, MIN_OUTSIDE = 25, 1500
MIN_INSIDE_F32 = 8
R_AGREE = 1e-3
MAX_LEFT_OUT = 0.01
MAX_NAN_DIFF = 0.01
RTOL = 1e-6                                  # the project's end-point bound (tests/test_gpu_parity.py)
OUTSIDE_BOUND = {"kerr-refractive": 2e-4}    # ... and its documented exception
SAME_POINTS_RTOL = 1e-12
CLOSEST_APPROACH = 1.000001                  # chart of the plunge (orbit-solving.jl:137-167)
R_FROM = 1.02                                # x inner_radius: the rows the table invariants are asserted on
TABLE_E_L_BOUND, TABLE_NORM_BOUND = 5e-8, 5e-9

_cache = {}


def metric(G, cls, params):
    return getattr(G, cls)(*params)


def render_kwargs(tol=TOL):
    return dict(image_width=W, image_height=H, alpha_lims=ALIMS, beta_lims=BLIMS, abstol=tol, reltol=tol)


def flat(img):
    """An H x W image (image[y, x]) in ray order i = x H + y, the order of the end-point records."""
    img = np.asarray(img)
    return img.T.ravel() if img.ndim == 2 else img


def oracle_config(oracle, name, params, tol=TOL):
    return oracle.make_config(name, params, disc=DISC, lambda_max=LAMBDA_MAX, abstol=tol, reltol=tol)


def oracle_table(oracle, name, params):
    """(ISCO, plunging table) of the case by the oracle: computed once per session, read-only."""
    key = ("table", name)
    if key not in _cache:
        ocfg = oracle_config(oracle, name, params)
        isco = oracle.isco(ocfg)
        table = tuple(oracle.plunging_table(ocfg, isco))
        for a in table:
            a.setflags(write=False)
        _cache[key] = (isco, table)
    return _cache[key]


def oracle_points(oracle, name, params, tol=TOL, nofma=False):
    """End points of the scene's rays by the oracle at `tol` (by its `nofma` build if asked): once per session, read-only."""
    key = ("points", name, tol, nofma)
    if key not in _cache:
        def run():
            ocfg = oracle_config(oracle, name, params, tol)
            return oracle.trace(ocfg, X_OBS, oracle.render_velocities(ocfg, X_OBS, ALIMS, BLIMS, W, H))

        if nofma:
            with oracle.nofma_library():
                pts = run()
        else:
            pts = run()
        pts.setflags(write=False)
        _cache[key] = pts
    return _cache[key]


def oracle_redshift(oracle, name, params, pts, isco, table):
    """oracle.apply_pf of the redshift ∘ filter_intersected on `pts` (records in the oracle's dtype), in ray order; `table` None:
    Kerr's analytic plunge."""
    ocfg = oracle_config(oracle, name, params)
    return oracle.apply_pf(ocfg, np.ascontiguousarray(pts), LAMBDA_MAX, pf_id=oracle.PF_REDSHIFT,
                           filter_id=oracle.FILTER_INTERSECTED, r_isco=isco, plunge=table)


def oracle_image(oracle, route, tol=TOL, nofma=False):
    """(redshift image in ray order, end points) of a ROUTES entry by the oracle's own trace, the table always the one of
    `oracle_table` (the main build at 1e-9)."""
    rid, (name, params, _), reads_table = route
    key = ("image", rid, tol, nofma)
    if key not in _cache:
        isco, table = oracle_table(oracle, name, params)
        pts = oracle_points(oracle, name, params, tol, nofma)
        img = oracle_redshift(oracle, name, params, pts, isco, table if reads_table else None)
        img.setflags(write=False)
        _cache[key] = (img, pts)
    return _cache[key]


def pointfunction(G, isco, table):
    """The fusable redshift ∘ filter_intersected with a GIVEN ISCO and table on its `extra` (None: Kerr's analytic plunge)."""
    from gradus_jl_amd.pointfunctions import GR_PF_REDSHIFT, PointFunction

    pf = PointFunction(lambda *a, **k: None, device_pf=GR_PF_REDSHIFT, extra={"r_isco": isco, "plunge": table})
    return pf @ G.ConstPointFunctions.filter_intersected()


def to_oracle_points(oracle, rec):
    """Records of the package (gr_point) as the oracle's orc_point: the field names already match."""
    out = np.zeros(rec.shape, dtype=oracle.POINT_DTYPE)
    for f in oracle.POINT_DTYPE.names:
        out[f] = rec[f]
    return out


def to_device_points(G, pts):
    """... and back."""
    out = np.zeros(pts.shape, dtype=G._lib.POINT_DTYPE)
    for f in G._lib.POINT_DTYPE.names:
        out[f] = pts[f]
    return out


def rho_of(pts):
    return pts["x"][..., 1] * np.abs(np.sin(pts["x"][..., 2]))


def stats(img, ref, pts_a, pts_b, isco, rho_clean=0.0):
    """`img` (end points `pts_a`) against `ref` (end points `pts_b`), both in ray order or both H x W: the pixels whose NaN pattern
    differs; over the pixels where both hit AND the end radii agree to R_AGREE, the largest relative error inside and outside the
    ISCO (by `pts_b`'s ρ) and how many there are; the common hits left out because their radii differ (counted, not hidden).
    `clean`: the inside-ISCO figure over ρ >= rho_clean only (the part of the table host test 3 holds to the invariants)."""
    img, ref = flat(img), flat(ref)
    pts_a, pts_b = np.asarray(pts_a).ravel(), np.asarray(pts_b).ravel()
    both = ~np.isnan(img) & ~np.isnan(ref)
    agree = np.abs(pts_a["x"][:, 1] - pts_b["x"][:, 1]) <= R_AGREE * np.maximum(np.abs(pts_b["x"][:, 1]), 1.0)
    use = both & agree
    inside = use & (rho_of(pts_b) < isco)
    outside = use & ~inside
    clean = inside & (rho_of(pts_b) >= rho_clean)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(img / ref - 1.0)

    def worst(sel):
        return float(rel[sel].max()) if sel.any() else 0.0

    return dict(nan_diff=int((np.isnan(img) != np.isnan(ref)).sum()), pixels=int(img.size), common=int(both.sum()),
                left_out=int((both & ~agree).sum()), left_out_max=worst(both & ~agree), n_inside=int(inside.sum()),
                n_outside=int(outside.sum()), inside=worst(inside), outside=worst(outside), n_clean=int(clean.sum()),
                clean=worst(clean), mask=use)


def describe(label, s):
    return (f"{label}: NaN pattern differs in {s['nan_diff']} of {s['pixels']}, common hits {s['common']} "
            f"({s['left_out']} left out, worst of them {s['left_out_max']:.2e}), inside the ISCO {s['n_inside']} hits max rel "
            f"{s['inside']:.3e} ({s['n_clean']} of them on the table's clean rows: {s['clean']:.3e}), outside {s['n_outside']} hits "
            f"max rel {s['outside']:.3e}")


def check_population(s, min_inside=MIN_INSIDE):
    """The condition every comparison asserts first."""
    assert s["n_inside"] >= min_inside and s["n_outside"] >= MIN_OUTSIDE, (s["n_inside"], s["n_outside"])
    assert s["left_out"] <= MAX_LEFT_OUT * s["common"], (s["left_out"], s["common"])
    assert s["nan_diff"] <= MAX_NAN_DIFF * s["pixels"], (s["nan_diff"], s["pixels"])


def rho_clean(oracle, route):
    """R_FROM x the first radius of the oracle's table: above it the table meets the invariants (host test 3) for every case.
    Below it the Bumblebee table is the stall at its g_rr pole, where v^t runs away and a redshift is decided by
    the last bits of the end radius: the oracle differs from its own nofma build by 9e-2 there."""
    return R_FROM * float(oracle_table(oracle, route[1][0], route[1][1])[1][0][0])


def nofma_floor(oracle, route):
    """(bound inside the ISCO, bound outside it, bound on the table's clean rows, the oracle-against-its-nofma-build figures
    they come from) for a trace of the route's scene at TOL.  Inside the ISCO an end-point error is amplified by the slope of g
    towards the horizon, so the bound there is 10 x what two roundings of the oracle's own algorithm differ by on the same
    scene and mask, at least RTOL."""
    key = ("floor", route[0])
    if key not in _cache:
        name, params, _ = route[1]
        isco, _ = oracle_table(oracle, name, params)
        (img, pts), (img_n, pts_n) = oracle_image(oracle, route), oracle_image(oracle, route, nofma=True)
        s = stats(img_n, img, pts_n, pts, isco, rho_clean(oracle, route))
        _cache[key] = (max(10.0 * s["inside"], RTOL), OUTSIDE_BOUND.get(name, RTOL), max(10.0 * s["clean"], RTOL), s)
    return _cache[key]


START_SHIFTS = (1e-15, 1e-13, -1e-13, 1e-11, -1e-11, 1e-10)


def table_start_sensitivity(oracle, route):
    """How far the oracle's own redshift image moves inside the ISCO (clean rows, its own end points) when the radius its
    plunge starts from moves by parts in 1e15 .. 1e10: the largest relative change over START_SHIFTS.  The start, 1e-8 inside a
    marginally stable orbit, is the one place where the last bits of the ISCO and of the first steps are amplified: the
    nodes of the table move (every case: 1e-4 .. 3e-4, the linear-interpolation error) and, for dilaton-axion, the PHASE of the
    orbit's tilt against r flips between two states (2.05e-2, or ~1e-5 when it does not flip)."""
    key = ("sensitivity", route[0])
    if key not in _cache:
        name, params, _ = route[1]
        isco, table = oracle_table(oracle, name, params)
        img, pts = oracle_image(oracle, route)
        ocfg = oracle_config(oracle, name, params)
        worst = 0.0
        for eps in START_SHIFTS:
            moved = tuple(oracle.plunging_table(ocfg, isco * (1.0 + eps)))
            s = stats(oracle_redshift(oracle, name, params, pts, isco, moved), img, pts, pts, isco,
                      R_FROM * max(float(table[0][0]), float(moved[0][0])))
            worst = max(worst, s["clean"])
        _cache[key] = worst
    return _cache[key]


def check_against_oracle_trace(oracle, route, img, pts, label):
    """`img` (in ray order or H x W, from end points `pts`) against the oracle's own trace of the route: the population, RTOL
    outside the ISCO, `nofma_floor` inside."""
    name, params, _ = route[1]
    isco, _ = oracle_table(oracle, name, params)
    ref, ref_pts = oracle_image(oracle, route)
    s = stats(img, ref, pts, ref_pts, isco, rho_clean(oracle, route))
    inside_bound, outside_bound, clean_bound, floor = nofma_floor(oracle, route)
    print(describe(f"{label} {route[0]} against the oracle's trace", s))
    print(describe(f"    oracle nofma against oracle, {route[0]}", floor)
          + f"  => bounds inside {inside_bound:.3e} (clean rows {clean_bound:.3e}), outside {outside_bound:.3e}")
    check_population(s)
    assert s["outside"] <= outside_bound
    assert s["inside"] <= inside_bound
    assert s["clean"] <= clean_bound
    return s


def against_ref_f32(img, ref):
    """f32_scene's rule for an image: (pixels whose NaN pattern differs, median relative error over the common hits, common hits)."""
    img, ref = flat(img), flat(ref)
    both = ~np.isnan(img) & ~np.isnan(ref)
    return int((np.isnan(img) != np.isnan(ref)).sum()), float(np.median(np.abs(img[both] / ref[both] - 1.0))), int(both.sum())


def check_f32(oracle, case, img, label, min_inside=MIN_INSIDE_F32):
    """A single-precision redshift image at F32_TOL against oracle@TOL: the NaN-pattern difference and the median relative error
    are each at most 1.5 x what oracle@F32_TOL shows (tests/f32_scene.py), with at least `min_inside` hits inside the ISCO."""
    route = (case[0], case, True)
    isco, _ = oracle_table(oracle, case[0], case[1])
    (ref, pts), (base, _) = oracle_image(oracle, route), oracle_image(oracle, route, tol=F32_TOL)
    (d, e, n), (d0, e0, n0) = against_ref_f32(img, ref), against_ref_f32(base, ref)
    n_in = int((~np.isnan(flat(img)) & ~np.isnan(ref) & (rho_of(pts) < isco)).sum())
    print(f"{label} {case[0]}: NaN pattern differs in {d} / {d0} pixels, median relative error {e:.3e} / {e0:.3e}, common hits "
          f"{n} / {n0}, of them inside the ISCO {n_in}  (f32 / oracle@{F32_TOL:g}, both against oracle@{TOL:g})")
    assert n_in >= min_inside and n >= MIN_OUTSIDE
    assert d <= 1.5 * d0
    assert e <= 1.5 * e0


def table_invariants(m, table, r_from):
    """What must hold along a timelike geodesic of a stationary axisymmetric metric, on the table's rows with r >= r_from, all
    evaluated in the equatorial plane (the table carries no θ) from m._components and CircularOrbits: E = -u_t and L = u_ϕ equal
    the ISCO orbit's (max |E / E₀ - 1|, max |L / L₀ - 1|), g(v, v) = -1 (max |g(v, v) + 1| over the sum of the absolute terms
    + 1); the rows that are not finite; the rows that are not monotone (r not above the row before, or v^r > 0 on a plunge)."""
    from gradus_jl_amd.special_radii import CircularOrbits

    r, vt, vr, vp = (np.asarray(a, dtype=np.float64) for a in table)
    finite = np.isfinite(r) & np.isfinite(vt) & np.isfinite(vr) & np.isfinite(vp)
    sel = (r >= r_from) & finite
    nonmono = int(((np.diff(r, prepend=-np.inf) <= 0.0) | (vr > 0.0))[sel].sum())
    r, vt, vr, vp = r[sel], vt[sel], vr[sel], vp[sel]
    g = [np.asarray(c, dtype=np.float64) + 0.0 * r for c in m._components(r, 1.0, 0.0)]          # tt, rr, θθ, ϕϕ, tϕ
    isco = m.isco()
    E0, L0 = float(CircularOrbits.energy(m, isco)), float(CircularOrbits.angmom(m, isco))
    E = -(g[0] * vt + g[4] * vp)
    L = g[4] * vt + g[3] * vp
    terms = [g[0] * vt * vt, 2.0 * g[4] * vt * vp, g[1] * vr * vr, g[3] * vp * vp]
    norm = np.abs(sum(terms) + 1.0) / (sum(np.abs(t) for t in terms) + 1.0)
    return dict(E=float(np.max(np.abs(E / E0 - 1.0))), L=float(np.max(np.abs(L / L0 - 1.0))), norm=float(np.max(norm)),
                nonfinite=int((~finite & ~(np.asarray(table[0]) < r_from)).sum()), nonmonotone=nonmono, rows=int(sel.sum()))


def g_rr_pole(m):
    """The largest radius at which 1 / g_rr of `m` changes sign in the equatorial plane, by bisection on m._components from
    20 M downwards: the coordinate singularity a plunge in these coordinates cannot cross."""
    def f(r):
        with np.errstate(all="ignore"):
            return float(1.0 / np.float64(m._components(np.float64(r), 1.0, 0.0)[1]))

    rs = np.linspace(20.0 * m.M, 0.05 * m.M, 8000)
    vals = np.array([f(float(r)) for r in rs])
    k = int(np.argmax(vals <= 0.0))
    assert vals[0] > 0.0 and k > 0
    hi, lo = float(rs[k - 1]), float(rs[k])
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if not (lo < mid < hi):
            break
        if f(mid) > 0.0:
            hi = mid
        else:
            lo = mid
    return hi
