"""The redshift point function, the ISCO and the plunging table of the seven catalogue cases that have an ISCO, on the host:
the kernel text compiled for the CPU (tests/harness.py in double, tests/harness_f32.py in single precision) and the Python
set-up code (metrics.py, special_radii.py) against the oracle, and the oracle's own tables against the conservation laws.
Runs without a GPU.  Scene, cases, criteria and their reasons: tests/redshift_scene.py; the device's turn:
tests/test_gpu_redshift_metrics.py; measured figures: DESIGN_measurements.md M29."""
import math

import numpy as np
import pytest

import harness as Hh
import harness_f32 as Hf
import redshift_scene as S

_host = {}


def _host_render(G, oracle, route, tol=S.TOL):
    """(fused image H x W, end-point records in the oracle's dtype) of a route by the double-precision host build, the oracle's
    ISCO and table on the point function: once per session."""
    if route[0] not in _host:
        rid, (name, params, cls), reads_table = route
        isco, table = S.oracle_table(oracle, name, params)
        cfg = G.render_configuration(S.metric(G, cls, params), S.X_OBS, G.ThinDisc(*S.DISC), S.LAMBDA_MAX, **S.render_kwargs(tol))
        pts = S.to_oracle_points(oracle, Hh.render_endpoints(G, cfg))
        img = Hh.render(G, cfg, S.pointfunction(G, isco, table if reads_table else None))
        img.setflags(write=False)
        pts.setflags(write=False)
        _host[route[0]] = (img, pts)
    return _host[route[0]]


@pytest.mark.parametrize("name,params,cls", S.CASES, ids=S.CASE_IDS)
def test_isco_equals_the_oracles(G, oracle, name, params, cls):
    """m.isco() (metrics.py `_components` on jets -> generic_isco, or the closed form) against orc_isco: two implementations of
    special-radii.jl:14-60 that share no code.  Measured: <= 3e-15."""
    mine, ref = S.metric(G, cls, params).isco(), oracle.isco(S.oracle_config(oracle, name, params))
    print(f"{name}: isco {mine!r} / {ref!r}  rel {abs(mine / ref - 1.0):.1e}")
    assert mine == pytest.approx(ref, rel=1e-12)


@pytest.mark.parametrize("name,params,cls", S.CASES, ids=S.CASE_IDS)
def test_oracle_table_ends_at_the_metrics_own_inner_radius(G, oracle, name, params, cls):
    """The plunge of orc_plunging_table runs in chart_for_metric(m; closest_approach = 1.000001) of the metric's OWN inner_radius
    (it used Kerr's M + sqrt(M² - a²) for every metric: 1.8043 for this Kerr-Newman whose horizon is at 1.6245, 1.866 for this
    dilaton-axion whose inner_radius is 3.551): the last step of the path is the one that crosses that radius.

    Two metrics cannot get there: the pole of g_rr as the reference writes it lies ABOVE its inner_radius (Bumblebee: Δ = (r² -
    2 M r) / (1 + l) vanishes at 2 M, inner_radius = M + sqrt(M² - a²) = 1.9798; dilaton-axion: Δ̂ = 0 at 3.58676, inner_radius
    3.55143, dilaton-axion-ad.jl:12 against :73), and no plunge crosses a coordinate singularity in these coordinates.  Their
    paths end within 1e-5 of that pole; `g_rr_pole` finds it from metrics.py, not from the table."""
    m = S.metric(G, cls, params)
    ocfg = S.oracle_config(oracle, name, params)
    r = oracle.plunging_path(ocfg, oracle.isco(ocfg))[0]
    r_inner, pole = m.inner_radius() * S.CLOSEST_APPROACH, S.g_rr_pole(m)
    _, table = S.oracle_table(oracle, name, params)
    print(f"{name}: path of {r.size} rows ends at {r[-2]!r}, {r[-1]!r}; chart's inner radius {r_inner!r}; pole of g_rr {pole!r}; "
          f"table starts at {table[0][0]!r}")
    assert (pole > r_inner) == (name in S.STALLS)
    if name in S.STALLS:
        assert abs(r.min() / pole - 1.0) < 1e-5 and r.min() > r_inner
    else:
        assert r[-1] <= r_inner < r[-2]                                    # ... within its last step
        assert np.all(np.diff(r) < 0.0)
        assert table[0][0] == r[-2]                                        # sortperm(r)[2:end]: the row below the chart is dropped


@pytest.mark.parametrize("name,params,cls", S.CASES, ids=S.CASE_IDS)
def test_oracle_table_is_a_timelike_geodesic_of_the_isco_orbit(G, oracle, name, params, cls):
    """On the rows with r >= 1.02 inner_radius the oracle's table keeps E and L of the ISCO orbit to 5e-8 and g(v, v) = -1 to
    5e-9 (measured: E <= 9.5e-9, L <= 1.7e-8, normalisation <= 5.3e-10), is finite and monotone.

    Dilaton-axion is held to the same bounds with θ and v^θ of the path (orc_plunging_table_ex) put into the identities: measured
    E 1.9e-9, L 3.2e-9, normalisation 1.0e-9.  Evaluated in the equatorial plane -- all a table without θ allows -- E appears to
    oscillate by 8.8e-3 and L by 2.7e-2, because the orbit LEAVES the plane (|θ - π/2| up to 0.233): with β != 0 this metric is
    not symmetric about it (Σ̂ carries -2 a R² (β / b) cos θ, W carries 2 (β / a b) cos θ; dilaton-axion-ad.jl:11,16), so ∂_θ g != 0
    at θ = π/2.  The reference builds the same table the same way; no defect.  Asserted: the plane leaves by > 0.1 rad, and the
    apparent oscillation is the offset between the two evaluation planes and nothing more.

    Bumblebee: below 1.02 inner_radius the table is the stall at the g_rr pole r = 2 M (test above): 1000-odd rows within 1e-6 of
    it, v^r changing sign at |v^r| ~ 1e-5.  A coordinate singularity of the metric as the reference defines it, not a defect."""
    from gradus_jl_amd.special_radii import CircularOrbits

    m = S.metric(G, cls, params)
    isco, table = S.oracle_table(oracle, name, params)
    r_from = S.R_FROM * m.inner_radius()
    inv = S.table_invariants(m, table, r_from)
    print(f"{name}: {inv}")
    assert inv["rows"] >= 300 and inv["nonfinite"] == 0 and inv["nonmonotone"] == 0
    if name != "dilaton-axion":
        assert inv["E"] <= S.TABLE_E_L_BOUND and inv["L"] <= S.TABLE_E_L_BOUND and inv["norm"] <= S.TABLE_NORM_BOUND
        return
    r, vt, vr, vp, th, vth = (a[::-1] for a in oracle.plunging_path(S.oracle_config(oracle, name, params), isco))
    sel = r >= r_from
    r, vt, vr, vp, th, vth = (a[sel] for a in (r, vt, vr, vp, th, vth))
    g = [np.asarray(c) + 0.0 * r for c in m._components(r, np.sin(th), np.cos(th))]
    gp = [np.asarray(c) + 0.0 * r for c in m._components(r, 1.0, 0.0)]
    E0, L0 = float(CircularOrbits.energy(m, isco)), float(CircularOrbits.angmom(m, isco))
    E, L = -(g[0] * vt + g[4] * vp), g[4] * vt + g[3] * vp
    Ep, Lp = -(gp[0] * vt + gp[4] * vp), gp[4] * vt + gp[3] * vp
    terms = [g[0] * vt * vt, 2.0 * g[4] * vt * vp, g[1] * vr * vr, g[2] * vth * vth, g[3] * vp * vp]
    norm = float(np.max(np.abs(sum(terms) + 1.0) / (sum(np.abs(t) for t in terms) + 1.0)))
    dE, dL, amp = float(np.max(np.abs(E / E0 - 1.0))), float(np.max(np.abs(L / L0 - 1.0))), float(np.max(np.abs(th - math.pi / 2)))
    off_E, off_L = float(np.max(np.abs(Ep / E - 1.0))), float(np.max(np.abs(Lp / L - 1.0)))
    print(f"{name} with θ of the path: E {dE:.2e}  L {dL:.2e}  normalisation {norm:.2e}  max |θ - π/2| {amp:.4f}; "
          f"offset of the plane evaluation E {off_E:.3e}  L {off_L:.3e}")
    assert dE <= S.TABLE_E_L_BOUND and dL <= S.TABLE_E_L_BOUND and norm <= S.TABLE_NORM_BOUND
    assert amp > 0.1
    assert inv["E"] <= off_E * (1.0 + 1e-6) + S.TABLE_E_L_BOUND and inv["L"] <= off_L * (1.0 + 1e-6) + S.TABLE_E_L_BOUND


@pytest.mark.parametrize("name,params,cls", S.CASES, ids=S.CASE_IDS)
def test_how_far_the_last_bits_of_the_isco_move_the_oracles_image(G, oracle, name, params, cls):
    """The oracle's own image inside the ISCO when the plunge starts parts in 1e15 .. 1e10 away (redshift_scene.START_SHIFTS):
    the table's nodes move, and with them the linear interpolation between them -- 1e-4 .. 3e-4 for six cases, under the 1e-3 a
    device-made table is held to against the oracle's.  Dilaton-axion moves by 2.05e-2: its table is the tilted orbit read as if
    it lay in the plane, and the phase of the tilt at a given r takes one of two values, chosen by the last bits of the start
    (a shift of 1e-13 flips it).  The oracle's ISCO and metrics.py's differ by 5 ulp, the device's table comes out in the other
    phase, and no bound below that figure can be asked of the whole chain for this metric (test_gpu_redshift_metrics.py)."""
    worst = S.table_start_sensitivity(oracle, (name, (name, params, cls), True))
    print(f"{name}: the oracle's image inside the ISCO moves by up to {worst:.3e} over start shifts {S.START_SHIFTS}")
    if name == "dilaton-axion":
        # above the cap of the other cases, and no more than two tables in opposite phases can differ by: twice the offset of
        # the plane evaluation (the larger of E's 8.8e-3 and L's 2.7e-2)
        m = S.metric(G, cls, params)
        inv = S.table_invariants(m, S.oracle_table(oracle, name, params)[1], S.R_FROM * m.inner_radius())
        assert 1e-3 < worst <= 2.0 * max(inv["E"], inv["L"])
    else:
        assert 1e-6 < worst < 1e-3


@pytest.mark.parametrize("route", S.ROUTES, ids=S.ROUTE_IDS)
def test_fused_image_equals_the_oracles_point_function_on_the_same_points(G, oracle, route):
    """redshift_pf of the kernel text (circular_fourvelocity on m.eval's g, ∂ᵣg, g⁻¹ outside the ISCO; the table inside) against
    orc_apply_pf on the SAME end-point records: no integration error in between, so identical NaN pattern and 1e-12, inside and
    outside the ISCO separately (measured <= 1.5e-14; a wrong ∂ᵣg_tϕ would show at 1e-3 and above)."""
    name, params, _ = route[1]
    isco, table = S.oracle_table(oracle, name, params)
    img, pts = _host_render(G, oracle, route)
    ref = S.oracle_redshift(oracle, name, params, pts, isco, table if route[2] else None)
    s = S.stats(img, ref, pts, pts, isco)
    print(S.describe(f"host {route[0]} on the same points", s))
    S.check_population(s)
    assert s["nan_diff"] == 0 and s["left_out"] == 0
    assert s["inside"] <= S.SAME_POINTS_RTOL and s["outside"] <= S.SAME_POINTS_RTOL


@pytest.mark.parametrize("route", S.ROUTES, ids=S.ROUTE_IDS)
def test_fused_image_against_the_oracles_own_trace(G, oracle, route):
    """The same image against oracle.rendergeodesics: 1e-6 outside the ISCO (Kerr-refractive 2e-4), inside it 10 x the oracle
    against its own nofma build with a floor of 1e-6 (redshift_scene.nofma_floor).  Measured, host / nofma floor, inside the
    ISCO: kerr 4.2e-8 / 4.4e-9, johannsen 2.4e-8 / 2.5e-8, bumblebee 4.5e-8 / 9.0e-2 (clean rows 4.5e-8 / 7.3e-9), kerr-newman
    1.3e-8 / 1.2e-8, johannsen-psaltis 1.4e-8 / 6.7e-9, dilaton-axion 3.6e-7 / 3.6e-7, kerr-refractive 2.3e-5 / 3.3e-5; outside:
    <= 9.9e-9 / 6.2e-9, kerr-refractive 1.8e-5 / 4.7e-5."""
    img, pts = _host_render(G, oracle, route)
    S.check_against_oracle_trace(oracle, route, img, pts, "host")


@pytest.mark.parametrize("name,params,cls", S.F32_CASES, ids=S.F32_CASE_IDS)
def test_f32_text_redshift_image(G, oracle, name, params, cls):
    """The single-precision text at 1e-5 with the oracle's table, by f32_scene's rule: against oracle@1e-9 the NaN pattern and
    the median relative error are each at most 1.5 x what oracle@1e-5 shows.  (Kerr-refractive: see redshift_scene.F32_CASES.)"""
    isco, table = S.oracle_table(oracle, name, params)
    cfg = G.render_configuration(S.metric(G, cls, params), S.X_OBS, G.ThinDisc(*S.DISC), S.LAMBDA_MAX, **S.render_kwargs(S.F32_TOL))
    S.check_f32(oracle, (name, params, cls), Hf.render(G, cfg, S.pointfunction(G, isco, table)), "host f32")


def test_dilaton_axion_refuses_a_coupling_it_divides_by(G):
    """With β != 0 the reference forms β / b, β / a, β / (a b) (dilaton-axion-ad.jl:25-27): b = 0 or a = 0 make them Inf and every
    component Inf or NaN.  DilatonAxion(1, 0.5, 0.2, 0).isco() raised ZeroDivisionError from inside `_components`; now the
    constructor says what is wrong.  β = 0 takes the reference's branch that never divides and stays valid for any a, b."""
    for a, b in ((0.5, 0.0), (0.0, 0.8), (0.0, 0.0)):
        with pytest.raises(ValueError, match="β != 0 needs b != 0 and a != 0"):
            G.DilatonAxion(1.0, a, 0.2, b)
    assert G.DilatonAxion(1.0, 0.5, 0.0, 0.0).isco() == pytest.approx(G.KerrMetric(1.0, 0.5).isco(), rel=1e-9)
    assert G.DilatonAxion(1.0, 0.0, 0.0, 0.0).isco() == pytest.approx(6.0, rel=1e-9)
    assert np.isfinite(G.DilatonAxion(1.0, 0.5, 0.2, 0.8).isco())
