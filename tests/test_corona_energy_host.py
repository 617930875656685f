"""The reference side of tests/test_gpu_corona_energy.py, on the CPU alone (tests/corona_scene.py holds the cases and the criteria):
the decomposition the device relies on for a source without one position, how steady the reference is on these rays (the oracle,
its build without FMA contraction, the host build of the kernel logic) and the conditions that keep the device test from being
vacuous."""
import numpy as np
import pytest

import corona_scene as S
import harness


@pytest.mark.parametrize("case", S.DISC_CASES, ids=S.DISC_CASE_IDS)
def test_static_observer_ratio_times_the_rows_factor_is_the_energy_ratio(G, oracle, case):
    """What sky_sample / k_sky_scale_g do with a row of gr_rayset.sky_rows: the ratio against the static observer u = (1, 0, 0, 0)
    -- what the trace kernel forms with has_u_src = 0 -- times (u_cov . v) / (g_tμ v^μ) IS energy_ratio against the sample's own
    source velocity, on the oracle's end points, the samples at the θ = 1e-3 clamp included."""
    K = G.corona
    ref = S.reference(G, oracle, case)
    xs, vs, vsrc = S.samples(G, case, S.N)
    rs, keep, x, v = K.sky_rayset(S.metric(G, case), case[2](G), S.sampler(G), S.N)
    rows = keep[1]
    np.testing.assert_array_equal(rows[:, 0:4], xs)
    np.testing.assert_array_equal(v, vsrc)
    assert np.min(xs[:, 2]) < 0.05
    static = S.energy_ratio(G, oracle, case, ref["pts"], np.tile([1.0, 0.0, 0.0, 0.0], (S.N, 1)))
    f = np.einsum("nq,nq->n", rows[:, 20:24], vs) / np.einsum("nq,nq->n", rows[:, 24:28], vs)
    hit = ref["status"] == S.HIT
    near_axis = hit & (xs[:, 2] < 0.05)
    dev = S.rel(static[hit] * f[hit], ref["g"][hit])
    print(f"{case[0]}: static-observer ratio x factor against energy_ratio: max {dev.max():.3e} median {np.median(dev):.3e} over {hit.sum()} hits, "
          f"{near_axis.sum()} of them from next to the axis; the factor spans {f[hit].min():.4f} ... {f[hit].max():.4f}")
    assert np.all(np.isfinite(f))
    assert np.ptp(f[hit]) > 0.05                     # a factor that matters: leaving it out, or taking a neighbour's, shows
    np.testing.assert_allclose(static[hit] * f[hit], ref["g"][hit], rtol=S.DECOMPOSITION_RTOL)


@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_the_reference_is_steady_on_these_rays(G, oracle, case):
    """The oracle, the oracle built without FMA contraction and the host build of the kernel logic on the same (x, v): the same
    statuses, g formed from their end points to STEADY_BOUND -- inside the ISCO too, where the spread decides the device's bar."""
    from gradus_jl_amd.tracing import tracing_configuration

    ref = S.reference(G, oracle, case)
    isco, _ = S.oracle_table(G, oracle, case)
    xs, vs, vsrc = S.samples(G, case, S.N)
    config = tracing_configuration(S.metric(G, case), np.ascontiguousarray(xs), np.ascontiguousarray(vs), G.ThinDisc(*S.DISC), (0.0, S.LAMBDA_MAX),
                                   callback=G.domain_upper_hemisphere())
    others = {"oracle without FMA": S.reference(G, oracle, case, nofma=True),
              "host build of the kernel logic": S.summarise(G, oracle, case, harness.trace_endpoints(G, config), vsrc)}
    for label, got in others.items():
        s = S.compare(got, ref, isco)
        print(S.describe(f"{case[0]}, {label} against the oracle", s))
        assert s["status_diff"] == 0, label
        assert s["g_all_max"] <= S.STEADY_BOUND and s["rho_all_max"] <= S.STEADY_BOUND and s["t_all_max"] <= S.STEADY_BOUND, label
        assert s["g_inside_max"] <= S.INSIDE_SPREAD_LIMIT, label          # so the device's bar inside the ISCO is RTOL as outside
        assert s["g_all_median"] <= S.MEDIAN_BOUND, label


@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_the_scene_reaches_what_it_is_meant_to_test(G, oracle, case):
    ref = S.reference(G, oracle, case)
    isco, table = S.oracle_table(G, oracle, case)
    hit = ref["status"] == S.HIT
    inside = hit & (ref["rho"] < isco)
    print(f"{case[0]}: {hit.sum()} hits, {inside.sum()} inside the ISCO at {isco:.4f} (the table has {table[0].size} rows from r = {table[0][0]:.4f})")
    assert hit.sum() >= S.MIN_HITS and inside.sum() >= S.MIN_INSIDE
    assert np.all(np.isfinite(ref["g"][hit])) and np.all(np.isnan(ref["g"][~hit]))
    assert ref["rho"][inside].min() >= table[0][0]                  # every inside hit is interpolated, none extrapolated
    if S.is_disc(case):
        xs, _, vsrc = S.samples(G, case, S.N)
        assert np.ptp(xs[:, 1]) > 1.0 and np.min(xs[:, 2]) < 0.05
        assert np.ptp(vsrc[:, 3]) > 0.0 or "stationary" in case[0]      # the source velocity differs from sample to sample
    else:
        xs, _, vsrc = S.samples(G, case, S.N)
        assert np.ptp(xs[:, 1]) == 0.0 and np.any(vsrc[0, 1:] != 0.0)   # one position, and a source that moves
