"""The redshift point function, the plunging table and the whole ISCO -> table -> image chain of the seven catalogue cases that
have an ISCO, on the device, against the oracle: what tests/test_redshift_metrics_host.py asks of the host builds of the same
text, asked of the kernels.  The device build differs from those in sqrt_fast / rcp_full, in the compiler's contraction and in
where the table is read from (LDS up to 640 rows for one-wave workgroups and 2048 for larger ones, global memory beyond: the
cases' tables have 373 .. 4584 rows and take all three paths).  Scene, cases, criteria: tests/redshift_scene.py; measured figures:
DESIGN_measurements.md M29."""
import math

import numpy as np
import pytest

import redshift_scene as S

pytestmark = pytest.mark.gpu


def _device_render(G, ens, route, pf, kernel, lds=1, tol=S.TOL, precision=64, cache=True):
    """(fused image H x W, apply(pf, cache) H x W or None, the end-point records in ray order) by the device."""
    _, (name, params, cls), _ = route
    m = S.metric(G, cls, params)
    ens.set("kernel", kernel).set("lds", lds).set("precision", precision)
    try:
        _, _, img = G.rendergeodesics(m, S.X_OBS, G.ThinDisc(*S.DISC), S.LAMBDA_MAX, pf=pf, ensemble=ens, **S.render_kwargs(tol))
        if not cache:
            return img, None, None
        _, _, rc = G.prerendergeodesics(m, S.X_OBS, G.ThinDisc(*S.DISC), S.LAMBDA_MAX, ensemble=ens, **S.render_kwargs(tol))
        return img, G.apply(pf, rc), np.ascontiguousarray(rc.points.T).ravel()
    finally:
        ens.set("precision", 64).set("lds", 1).set("kernel", 2)


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("route", S.ROUTES, ids=S.ROUTE_IDS)
def test_fused_redshift_equals_the_oracles_point_function_on_the_same_points(G, oracle, ens, route, kernel, lds):
    """The fused image, with the oracle's ISCO and table on the point function and the table read out of LDS (lds = 1, where it
    fits) or out of global memory (lds = 0): the same bytes as `apply` on the end-point cache, and equal to orc_apply_pf on the
    device's OWN records -- identical NaN pattern, 1e-12 inside and outside the ISCO.  Two orders above the host build's 1.4e-14
    leave room for sqrt_fast / rcp_full, five orders stay below any wrong term of m.eval."""
    name, params, _ = route[1]
    isco, table = S.oracle_table(oracle, name, params)
    pf = S.pointfunction(G, isco, table if route[2] else None)
    img, applied, rec = _device_render(G, ens, route, pf, kernel, lds)
    ref = S.oracle_redshift(oracle, name, params, S.to_oracle_points(oracle, rec), isco, table if route[2] else None)
    s = S.stats(img, ref, rec, rec, isco)
    print(S.describe(f"device {route[0]} kernel {kernel} lds {lds} on the same points", s))
    assert img.tobytes() == applied.tobytes()
    S.check_population(s)
    assert s["nan_diff"] == 0 and s["left_out"] == 0
    assert s["inside"] <= S.SAME_POINTS_RTOL and s["outside"] <= S.SAME_POINTS_RTOL


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("route", S.ROUTES, ids=S.ROUTE_IDS)
def test_fused_redshift_against_the_oracles_own_trace(G, oracle, ens, route, kernel):
    """The same image against oracle.rendergeodesics with the bounds of the host test: 1e-6 outside the ISCO (Kerr-refractive
    2e-4), inside it 10 x the oracle against its own nofma build, floor 1e-6 -- bounds that come from the oracle, not from the
    device."""
    name, params, _ = route[1]
    isco, table = S.oracle_table(oracle, name, params)
    pf = S.pointfunction(G, isco, table if route[2] else None)
    img, _, rec = _device_render(G, ens, route, pf, kernel)
    S.check_against_oracle_trace(oracle, route, img, rec, f"device kernel {kernel}")


@pytest.mark.parametrize("name,params,cls", S.CASES, ids=S.CASE_IDS)
def test_device_plunging_table_is_a_timelike_geodesic_of_the_isco_orbit(G, oracle, ens, name, params, cls):
    """interpolate_plunging_velocities(m, ensemble=ens): metrics.py `_components` -> generic_isco -> plunging_fourvelocity -> the
    μ = 1 geodesic of k_trace_path with the metric's fused right-hand side.  It starts at or above the chart's inner radius, ends
    below the ISCO, and on its rows with r >= 1.02 inner_radius it is finite, strictly increasing in r, infalling, and keeps E,
    L and g(v, v) = -1 to 3 x what the oracle's table of the case does (both are Tsit5 at reltol 1e-9 on other step sequences).

    Bumblebee and dilaton-axion below 1.02 inner_radius: the stall at the pole of g_rr (host file), ties in r included, so the
    whole-table monotony is asked of the other five only.  Dilaton-axion: evaluated in the plane both tables show the offset of
    its tilted orbit (E 8.8e-3, L 2.7e-2; host file), so the device's own path is traced here once more with its θ and held to
    3 x the oracle's path on the identities with θ in them."""
    from gradus_jl_amd.special_radii import plunging_fourvelocity
    from gradus_jl_amd.tracing import PolarChart, tracegeodesic_path

    m = S.metric(G, cls, params)
    isco_o, table_o = S.oracle_table(oracle, name, params)
    table = tuple(G.interpolate_plunging_velocities(m, ensemble=ens))
    r = table[0]
    r_from = S.R_FROM * m.inner_radius()
    mine, ref = S.table_invariants(m, table, r_from), S.table_invariants(m, table_o, r_from)
    print(f"{name}: device table of {r.size} rows from {r[0]!r} to {r[-1]!r} (oracle: {table_o[0].size} rows from {table_o[0][0]!r})")
    print(f"    device {mine}\n    oracle {ref}")
    assert r[0] >= m.inner_radius() * S.CLOSEST_APPROACH and r[-1] < m.isco()
    assert mine["rows"] >= 300 and mine["nonfinite"] == 0 and mine["nonmonotone"] == 0
    if name not in S.STALLS:
        assert all(np.all(np.isfinite(a)) for a in table) and np.all(np.diff(r) > 0.0)
    for k in ("E", "L", "norm"):
        assert mine[k] <= 3.0 * ref[k], k
    if name != "dilaton-axion":
        return

    def with_theta(r_, vt, vr, vp, th, vth):
        sel = r_ >= r_from
        r_, vt, vr, vp, th, vth = (a[sel] for a in (r_, vt, vr, vp, th, vth))
        g = [np.asarray(c) + 0.0 * r_ for c in m._components(r_, np.sin(th), np.cos(th))]
        E, L = -(g[0] * vt + g[4] * vp), g[4] * vt + g[3] * vp
        terms = [g[0] * vt * vt, 2.0 * g[4] * vt * vp, g[1] * vr * vr, g[2] * vth * vth, g[3] * vp * vp]
        return (float(np.max(np.abs(E / E[0] - 1.0))), float(np.max(np.abs(L / L[0] - 1.0))),
                float(np.max(np.abs(sum(terms) + 1.0) / (sum(np.abs(t) for t in terms) + 1.0))), float(np.max(np.abs(th - math.pi / 2))))

    # the call of special_radii.interpolate_plunging_velocities, keeping the path
    u = np.array([0.0, m.isco() - 1e-8, math.pi / 2, 0.0])
    path = tracegeodesic_path(m, u, plunging_fourvelocity(m, m.isco()), (0.0, 50_000.0), μ=1.0, reltol=1e-9,
                              chart=PolarChart(m.inner_radius() * S.CLOSEST_APPROACH, 12000.0), ensemble=ens)
    dev = with_theta(path.x[:, 1], path.v[:, 0], path.v[:, 1], path.v[:, 3], path.x[:, 2], path.v[:, 2])
    orc = with_theta(*oracle.plunging_path(S.oracle_config(oracle, name, params), isco_o))
    print(f"    with θ of the path (drift of E, of L, normalisation, max |θ - π/2|): device {dev}  oracle {orc}")
    assert dev[0] <= 3.0 * orc[0] and dev[1] <= 3.0 * orc[1] and dev[2] <= 3.0 * orc[2]
    assert abs(dev[3] / orc[3] - 1.0) < 1e-3           # the same tilt of the orbit


def _chain_stats(oracle, route_ref, img, rec, first_radius):
    name, params, _ = route_ref[1]
    isco, table = S.oracle_table(oracle, name, params)
    ref, ref_pts = S.oracle_image(oracle, route_ref)
    return S.stats(img, ref, rec, ref_pts, isco, S.R_FROM * max(first_radius, float(table[0][0])))


@pytest.mark.parametrize("route", S.ROUTES, ids=S.ROUTE_IDS)
def test_whole_chain_on_the_device_against_the_oracles_whole_chain(G, oracle, ens, route):
    """ConstPointFunctions.redshift(m, x, ensemble=ens) -- the package's own ISCO, its own table traced on the device -- against
    the oracle with ITS ISCO and table; for Kerr that call is the analytic plunge, and `kerr` here is
    interpolate_redshift(interpolate_plunging_velocities(m)).  Inside the ISCO on ρ >= 1.02 x the larger of the two tables' first
    radii.  Two tables differ by their linear interpolation between other nodes: on the oracle Kerr's table image deviates from
    its analytic image by 2.8e-4, and the oracle's tables of the seven cases from those of its nofma build by 1.5e-6 .. 2.8e-4.
    So: Kerr's device table against the oracle's ANALYTIC image at most 2 x that first figure, computed here; the other cases a cap
    of 1e-3; Kerr's analytic route, which reads no table, and every case outside the ISCO: the bounds of the test above.
    Dilaton-axion: its table is a tilted orbit read as if it lay in the plane, and the last bits of the start decide between two
    phases of the tilt (host file): the oracle's own image moves by 2.05e-2 when its ISCO moves by 1e-13, the
    device's table (its ISCO is 5 ulp from the oracle's) comes out in the other phase and differs by that same 2.05e-2.  Bound:
    2 x what the oracle's image moves by over redshift_scene.START_SHIFTS, computed here from the oracle alone."""
    rid, (name, params, cls), reads_table = route
    m = S.metric(G, cls, params)
    CPF = G.ConstPointFunctions
    if rid == "kerr":
        pf = G.interpolate_redshift(G.interpolate_plunging_velocities(m, ensemble=ens), S.X_OBS) @ CPF.filter_intersected()
    else:
        pf = CPF.redshift(m, S.X_OBS, ensemble=ens) @ CPF.filter_intersected()
    assert (pf.extra["plunge"] is not None) == reads_table
    first = float(pf.extra["plunge"][0][0]) if reads_table else 0.0
    img, _, rec = _device_render(G, ens, route, pf, 1)
    inside_bound, outside_bound, clean_bound, _ = S.nofma_floor(oracle, route)
    if rid == "kerr":
        analytic = S.ROUTES[S.ROUTE_IDS.index("kerr-analytic")]
        s = _chain_stats(oracle, analytic, img, rec, first)
        (tab, pts), (ana, _) = S.oracle_image(oracle, route), S.oracle_image(oracle, analytic)
        own = S.stats(tab, ana, pts, pts, S.oracle_table(oracle, name, params)[0], S.R_FROM * first)
        print(S.describe("oracle kerr table image against its analytic image", own))
        clean_bound = 2.0 * own["clean"]
        assert 1e-5 < own["clean"] < 1e-3
    else:
        s = _chain_stats(oracle, route, img, rec, first)
        if reads_table:
            clean_bound = 1e-3
        if name == "dilaton-axion":
            clean_bound = max(clean_bound, 2.0 * S.table_start_sensitivity(oracle, route))
    print(S.describe(f"device {rid} whole chain", s) + f"  => bounds clean rows {clean_bound:.3e}, outside {outside_bound:.3e}")
    S.check_population(s)
    assert s["n_clean"] >= S.MIN_INSIDE
    assert s["outside"] <= outside_bound
    assert s["clean"] <= clean_bound


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("name,params,cls", S.F32_CASES, ids=S.F32_CASE_IDS)
def test_f32_kernels_redshift_image(G, oracle, ens, kernel, name, params, cls):
    """The fp32 kernel objects at 1e-5 with the oracle's table, by f32_scene's rule: against oracle@1e-9 the NaN pattern and
    the median relative error are each at most 1.5 x what oracle@1e-5 shows, with at least 8 hits inside the ISCO."""
    case = (name, params, cls)
    isco, table = S.oracle_table(oracle, name, params)
    img, _, _ = _device_render(G, ens, (name, case, True), S.pointfunction(G, isco, table), kernel, tol=S.F32_TOL, precision=32,
                               cache=False)
    S.check_f32(oracle, case, img, f"device f32 kernel {kernel}")
