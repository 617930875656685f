"""The producer of ring and disc corona profiles (corona_arms, src/corona/models/ring.jl:1-485) on the CPU: gr_ringarm.hpp compiled
with g++ (tests/host_harness_ringarm.cpp) against the numpy transcription the lock-step route runs, bit for bit; ray formation
against sky_angles_to_velocity; the arm splitting of ring.jl:304-386 on hand-built sequences; the lock-step route end to end on
rays the oracle traces; and flat space against the closed form."""
import math
import os
import re

import numpy as np
import pytest

import harness_ringarm as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT, MISS = 2, 0


def test_constants_and_exports(G):
    from gradus_jl_amd import _lib

    K = G.corona
    assert R.lib().hring_invphi() == K.INVPHI == 0.6180339887498949          # (sqrt(5) - 1) / 2, ring.jl:1
    hdr = open(os.path.join(ROOT, "include", "gradus_mi355x.h")).read()
    for name in ("gr_ring_rays", "gr_ring_arms"):
        assert name in _lib.EXPORTS and re.search(r"int32_t " + name + r"\(gr_ctx\* ctx, const gr_config\* cfg, const gr_ringset\* rings,", hdr)
    assert _lib.C.sizeof(_lib.gr_ringset) == 56
    np.testing.assert_array_equal(G.DEFAULT_β_ANGLES(100), np.linspace(0.0, math.pi - math.pi / 100, 100))


def test_base_angles_and_the_reference_errors(G):
    K = G.corona
    a = K.ring_base_angles(1000, 80)
    assert a.size == 840 and np.all(np.diff(a) > 0) and a[0] == 1e-7 and a[-1] < 2 * math.pi
    np.testing.assert_allclose(a[420:], a[:420] + math.pi, rtol=1e-15)
    with pytest.raises(ValueError, match="Too few samples for selected method. Pass `n_samples` of more than 160"):
        K.ring_base_angles(160, 80)
    with pytest.raises(ValueError, match="must be an even number for this method \\(given 41\\)"):
        K.ring_base_angles(201, 80)


# ---------------------------------------------------------------------------------------------------------------
# bracket and golden-section update on synthetic objective tables
# ---------------------------------------------------------------------------------------------------------------
def objective(target, block, θ0):
    """ρ(θ) with a single extremum at θ0 -- 5 + 3 (θ - θ0)² (minima) or 50 - 3 (θ - θ0)² (maxima) -- and a block of misses
    0.05 ... 0.5 beside it on the `block` side ("left" | "right" | None): θ -> (status, ρ)"""
    def f(θ):
        ρ = 5.0 + 3.0 * (θ - θ0) ** 2 if target == 0 else 50.0 - 3.0 * (θ - θ0) ** 2
        off = θ - θ0
        missed = (block == "right" and 0.05 <= off <= 0.5) or (block == "left" and -0.5 <= off <= -0.05)
        return (MISS if missed else HIT), ρ
    return f


def base_table(f, N):
    angles = np.linspace(1e-7, 2 * math.pi - 1e-7, N)
    rows = np.zeros((N, 4))
    for i, θ in enumerate(angles):
        rows[i, 3], rows[i, 1] = f(θ)
    rows[:, 0] = np.where(rows[:, 3] == HIT, 1.0, np.nan)
    return angles, rows


def extremum_at(where, N):
    """"off": a quarter of a radian beside a base angle of the coarse table; "on": ON base angle N // 3, so that no probe can beat
    the initial estimate and only too_many_iters ends the search"""
    return 2.35 if where == "off" else float(np.linspace(1e-7, 2 * math.pi - 1e-7, N)[N // 3])


CASES = [(target, block, N, E, where) for target in (0, 1) for block in (None, "left", "right") for N in (10, 64) for E in (6, 20)
         for where in ("off", "on")]


@pytest.mark.parametrize("target,block,N,E,where", CASES)
def test_harness_equals_the_numpy_transcription_bit_for_bit(G, target, block, N, E, where):
    K = G.corona
    f = objective(target, block, extremum_at(where, N))
    angles, rows = base_table(f, N)
    want, got = K.determine_bracket(rows, angles, target), R.bracket(rows, angles, target)
    assert got is not None
    np.testing.assert_array_equal(np.array(got), np.array(want))
    δ = math.pi / (10 if N == 10 else 32)
    hits = rows[:, 3] == HIT
    i = int(np.argmin(np.where(hits, rows[:, 1], np.inf)) if target == 0 else np.argmax(np.where(hits, rows[:, 1], -np.inf)))
    lo = angles[i - 1] if not hits[i - 1] else angles[i]
    hi = angles[i + 1] if not hits[i + 1] else angles[i]
    assert want == (lo - 2.0 * δ, hi + 2.0 * δ, rows[i, 1])          # the two widenings, δ = π / min(N, 32)
    py, cc = K.GoldenSearch(*want, target), R.HarnessSearch(*want, target)
    kept_py, kept_cc = [], []
    for _ in range(2 * E + 1):
        if py.done:
            break
        probes = py.probes()
        np.testing.assert_array_equal(np.array(cc.probes()), np.array(probes))
        (cs, cρ), (ds, dρ) = f(probes[0]), f(probes[1])
        a_py, a_cc = py.update(E, cs, cρ, ds, dρ), cc.update(E, cs, cρ, ds, dρ)
        assert a_py == a_cc and R.state_of(py) == cc.astuple()
        if a_py:
            kept_py.append(probes[a_py - 1])
            kept_cc.append(cc_probe := probes[a_cc - 1])
            ρ_kept = f(cc_probe)[1]
            assert K._better(target, ρ_kept, want[2])          # only what beats the initial estimate is kept
    assert py.done and py.n == E and py.iters <= 2 * E + 1 and len(kept_py) <= E and kept_py == kept_cc


def test_both_endings_of_the_loop_occur(G):
    """extrema_iter = 6: somewhere too_many_iters decides the end (fewer than 6 probes kept, more than 6 iterations); 20: somewhere
    every iteration keeps a probe and the loop ends at n == extrema_iter without it"""
    K = G.corona
    endings = {}
    for target, block, N, E, where in CASES:
        f = objective(target, block, extremum_at(where, N))
        angles, rows = base_table(f, N)
        s, kept = K.GoldenSearch(*K.determine_bracket(rows, angles, target), target), 0
        while not s.done:
            c, d = s.probes()
            kept += 1 if s.update(E, *f(c), *f(d)) else 0
        endings[(target, block, N, E, where)] = (s.too_many, kept, s.iters)
    assert any(too_many and kept < E and iters > E for (_, _, _, E, _), (too_many, kept, iters) in endings.items() if E == 6)
    assert any(too_many and kept == 0 and iters == 2 * E + 1 for (_, _, _, E, _), (too_many, kept, iters) in endings.items() if E == 6)
    assert any(not too_many and kept == E == iters for (_, _, _, E, _), (too_many, kept, iters) in endings.items() if E == 20)


def test_a_slice_without_a_hit_has_no_bracket(G):
    angles = np.linspace(0.1, 6.0, 12)
    rows = np.zeros((12, 4))
    rows[:, 1], rows[:, 3] = 7.0, 3.0
    assert G.corona.determine_bracket(rows, angles, 0) is None and R.bracket(rows, angles, 1) is None


def test_three_iterations_by_hand(G):
    """_golden_bracket! (ring.jl:206-236) from a = 0, b = 1, best_estimate = 10, minima, extrema_iter = 3:
    1. c = 1 - INVPHI, d = INVPHI; ρ(c) = 8 < ρ(d) = 9 and 8 < 10: c is kept, n = 1, b = d.
    2. c misses -> takes the value 10; ρ(d) = 9.5: not 10 < 9.5, so the else arm: 9.5 < 10, d is kept, n = 2, a = c.
    3. ρ(c) = ρ(d) = 9.9: the strict comparison fails, the else arm again: d is kept, n = 3, a = c; the loop ends at n == 3."""
    for S in (G.corona.GoldenSearch, R.HarnessSearch):
        s = S(0.0, 1.0, 10.0, 0)
        state = lambda: R.state_of(s) if S is G.corona.GoldenSearch else s.astuple()
        assert s.probes() == (0.3819660112501051, 0.6180339887498949)
        assert s.update(3, HIT, 8.0, HIT, 9.0) == 1
        assert state() == (0.0, 0.6180339887498949, 10.0, 1, 1, False, False)
        assert s.probes() == (0.2360679774997897, 0.3819660112501052)
        assert s.update(3, MISS, 1.0, HIT, 9.5) == 2
        assert state() == (0.2360679774997897, 0.6180339887498949, 10.0, 2, 2, False, False)
        assert s.probes() == (0.38196601125010515, 0.47213595499957944)
        assert s.update(3, HIT, 9.9, HIT, 9.9) == 2
        assert state() == (0.38196601125010515, 0.6180339887498949, 10.0, 3, 3, False, True)


def test_lockstep_cache_layout_on_a_synthetic_tracer(G):
    """lockstep_arm_traces over an analytic tracer: base rows first, then what the minima search kept, then the maxima search's;
    a slice whose rays all miss reports (N, -1, -1)"""
    K = G.corona
    fs = {0: objective(0, "right", 2.35), 1: objective(1, None, 4.1)}

    def tracer(ring, slice_, angles):
        rows = np.zeros((len(angles), 4))
        for j, (s, θ) in enumerate(zip(slice_, angles)):
            if s == 2:
                rows[j] = (np.nan, 3.0, 0.0, 3.0)
                continue
            # one curve with a minimum (slice 0's) and a maximum (slice 1's objective, lifted)
            st0, ρ0 = fs[0](θ)
            rows[j] = (1.0, ρ0 + (10.0 - 3.0 * (θ - 4.1) ** 2 if s == 1 else 0.0), θ, st0)
        return rows

    base = K.ring_base_angles(40 + 12, 6)
    rows, counts = K.lockstep_arm_traces(tracer, 1, 3, base, 6)
    assert rows.shape == (1, 3, 52, 5) and counts.shape == (1, 3, 3)
    assert counts[0, 2].tolist() == [40, -1, -1] and np.all(rows[0, 2, 40:] == 0.0)
    for s in (0, 1):
        n, k_min, k_max = counts[0, s]
        assert n == 40 and 0 <= k_min <= 6 and 0 <= k_max <= 6 and k_min + k_max > 0
        np.testing.assert_array_equal(rows[0, s, :40, 0], base)
        hit = rows[0, s, :40, 4] == HIT
        est_min, est_max = rows[0, s, :40, 2][hit].min(), rows[0, s, :40, 2][hit].max()
        assert np.all(rows[0, s, 40:40 + k_min, 2] < est_min) and np.all(rows[0, s, 40 + k_min:40 + k_min + k_max, 2] > est_max)
        assert np.all(rows[0, s, 40 + k_min + k_max:] == 0.0)


# ---------------------------------------------------------------------------------------------------------------
# ray formation
# ---------------------------------------------------------------------------------------------------------------
ANGLES = np.concatenate([[-0.4, -1e-3, 1e-7, 2 * math.pi + 0.3, 7.5], np.linspace(0.05, 6.2, 11)])


@pytest.mark.parametrize("β", [0.0, 0.3, math.pi / 2, math.pi - math.pi / 100])
@pytest.mark.parametrize("ring", ["kerr r=8 h=3", "near-axis r=1e-2 h=5"])
def test_ray_formation_equals_sky_angles_to_velocity(G, ring, β):
    K = G.corona
    assert ANGLES.size == 16
    m = G.KerrMetric(1.0, R.KERR_A)
    model = G.RingCorona(G.SourceVelocities.co_rotating, 8.0, 3.0) if ring.startswith("kerr") else G.RingCorona(G.SourceVelocities.co_rotating, 1e-2, 5.0)
    frames, xs, vsrc = K.ring_frames(m, [model])
    want = K.ring_velocities(m, xs[0], vsrc[0], β, ANGLES)
    got, f = R.form_rays(frames[0], β, ANGLES)
    np.testing.assert_allclose(got, want, rtol=0.0, atol=1e-12 * np.abs(want).max())
    # the factor of g: (u_μ v^μ) / (g_tμ v^μ) of the formed velocity
    g = K._components_at(m, xs[0])
    u, stat = np.tile(vsrc[0], (16, 1)), np.tile([1.0, 0.0, 0.0, 0.0], (16, 1))
    np.testing.assert_allclose(f, K._dot(g, want, u) / K._dot(g, want, stat), rtol=1e-9)


# ---------------------------------------------------------------------------------------------------------------
# arm splitting (ring.jl:304-386): index lists are 1-based, as in the reference
# ---------------------------------------------------------------------------------------------------------------
def test_split_monotone_gives_one_list(G):
    assert G.corona._split_branches_further(list(range(1, 9)), np.arange(1.0, 9.0)) == [[1, 2, 3, 4, 5, 6, 7, 8]]


def test_split_v_shape(G):
    """minimum at index 5, maximum at index 9: r1 = 10:9 ++ 1:4, r2 = 6:9 (the minimum itself belongs to neither, ring.jl:380-381);
    each list in ascending ρ (canonical_orders!)"""
    ρ = np.array([5.0, 4.0, 3.0, 2.0, 1.0, 2.5, 3.5, 4.5, 5.5])
    assert G.corona._split_arms_indices(np.arange(9.0), ρ) == [[4, 3, 2, 1], [6, 7, 8, 9]]


def test_split_values_above_cutoff_r(G):
    """ρ > cutoff_r = 1e3 sets `increasing = false` without a split; the rise behind it splits at k - 1 = 6, which both pieces hold"""
    ρ = np.array([1.0, 2.0, 3.0, 2000.0, 3000.0, 1.5, 2.5, 3.5, 4.5, 5.5])
    assert G.corona._split_branches_further(list(range(1, 11)), ρ) == [[1, 2, 3, 4, 5, 6], [6, 7, 8, 9, 10]]
    # ... and when what follows the cutoff values is too short to stand alone it merges: one list
    ρ = np.array([1.0, 2.0, 2000.0, 3000.0, 3.0, 4.0])
    assert G.corona._split_branches_further(list(range(1, 7)), ρ) == [[1, 2, 3, 4, 5, 6]]


def test_split_short_pieces_merge(G):
    """a dip of one point: splits [1, 1, 5, 6, 11]; the piece 5:6 is shorter than min_length = 3 and joins the next"""
    ρ = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 4.5, 5.5, 6.5, 7.5, 8.5, 9.5])
    assert G.corona._split_branches_further(list(range(1, 12)), ρ) == [[1, 2, 3, 4, 5], [5, 6, 7, 8, 9, 10, 11]]
    # a dip smaller than delta = 0.01 does not split at all
    ρ[5] = 4.995
    assert G.corona._split_branches_further(list(range(1, 12)), ρ) == [list(range(1, 12))]


def test_first_two_of_three_lists(G):
    """minimum at 4, maximum at 8 of 16 points; r1 = 9:16 ++ 1:3 falls and rises again, so l1 has two lists and vcat(l1, l2) three:
    `r1, r2 = _split_arms_indices(...)` (ring.jl:415) takes the two of l1 and drops l2 = [[5, 6, 7, 8]]"""
    K = G.corona
    ρ = 10.0 * np.array([9.2, 9.4, 9.6, 1.0, 2.0, 3.0, 4.0, 10.0, 9.0, 8.0, 7.0, 6.0, 5.0, 6.5, 7.5, 8.5])
    θ = np.linspace(0.1, 6.0, 16)
    lists = K._split_arms_indices(θ, ρ)
    assert lists == [[13, 12, 11, 10, 9], [13, 14, 15, 16, 1, 2, 3], [5, 6, 7, 8]]
    m = G.KerrMetric(1.0, 0.5)
    rows = np.stack([θ, np.ones(16), ρ, 2.0 * ρ, np.full(16, 2.0)], axis=1)
    rows = np.concatenate([rows, [[3.0, np.nan, 55.0, 1.0, 3.0]]])          # a miss: masked
    arm = K.ring_arm(m, K.PowerLawSpectrum(2.0), np.array([1.2, 0.0, 0.0, 0.0]), K.keplerian_velocity_projector(m), 0.3, rows)
    np.testing.assert_array_equal(arm.left_r, ρ[[12, 11, 10, 9, 8]])
    np.testing.assert_array_equal(arm.right_r, ρ[[12, 13, 14, 15, 0, 1, 2]])
    np.testing.assert_array_equal(arm.left_t, 2.0 * arm.left_r)
    assert arm.β == 0.3 and np.all(arm.left_ε >= 0) and np.all(arm.right_ε >= 0) and np.all(np.isfinite(arm.right_ε))
    with pytest.raises(ValueError, match="ring 3, slice 1: .*fewer than 2"):
        K.ring_arm(m, K.PowerLawSpectrum(2.0), np.array([1.2, 0.0, 0.0, 0.0]), K.keplerian_velocity_projector(m), 0.3, rows[:1], where="ring 3, slice 1: ")


# ---------------------------------------------------------------------------------------------------------------
# end to end on the oracle's rays
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kerr_lockstep(G, oracle):
    """corona_arms(route="lockstep") with every row from the oracle: (model scene, tracer, arms)"""
    m, d, models = R.kerr_scene(G)
    ocfg = oracle.make_config("kerr", (1.0, R.KERR_A), disc=(0.0, 200.0), lambda_max=1_000_000.0, outer_radius=1_000_000.0, upper_hemisphere=True)
    dv = R.oracle_disc_velocity(G, oracle, m, ocfg)
    βs = np.array([0.0, 0.9, 2.2])
    tracer = R.OracleTracer(G, oracle, m, ocfg, models, βs, dv)
    kw = dict(n_samples=120, extrema_iter=10, route="lockstep", tracer=tracer, disc_velocity=dv)
    rows, counts, base = G.corona_arm_traces(m, d, models, βs, n_samples=120, extrema_iter=10, route="lockstep", tracer=tracer)
    return m, d, models[0], βs, kw, rows, counts, base


def test_lockstep_on_the_oracle_keeps_only_improvements(G, kerr_lockstep):
    m, d, model, βs, kw, rows, counts, base = kerr_lockstep
    assert base.size == 100 and rows.shape == (1, 3, 120, 5)
    for s in range(3):
        n, k_min, k_max = (int(c) for c in counts[0, s])
        assert n == 100 and 0 <= k_min <= 10 and 0 <= k_max <= 10
        hit = rows[0, s, :100, 4] == HIT
        assert hit.sum() > 20
        ρ0 = rows[0, s, :100, 2][hit]
        kept_min, kept_max = rows[0, s, 100:100 + k_min], rows[0, s, 100 + k_min:100 + k_min + k_max]
        assert np.all(kept_min[:, 4] == HIT) and np.all(kept_max[:, 4] == HIT)
        assert np.all(kept_min[:, 2] < ρ0.min()) and np.all(kept_max[:, 2] > ρ0.max())
        assert np.all(rows[0, s, 100 + k_min + k_max:] == 0.0)
    assert counts[0, :, 1:].sum() > 0


def test_profile_from_the_oracle_and_its_host_lag_transfer(G, kerr_lockstep):
    import harness_tftd as T

    m, d, model, βs, kw, *_ = kerr_lockstep
    arms = G.corona_arms(m, d, model, βs, **kw)
    assert len(arms) == 3 and all(isinstance(a, G.LongitudalArms) for a in arms)
    for a, β in zip(arms, βs):
        assert a.β == β
        for r, t, ε in ((a.left_r, a.left_t, a.left_ε), (a.right_r, a.right_t, a.right_ε)):
            assert r.size >= 2 and r.shape == t.shape == ε.shape
            assert np.all(np.diff(r) >= 0) and np.all(np.isfinite(ε)) and np.all(ε >= 0) and np.all(np.isfinite(t))
    prof = G.ring_corona_profile(m, d, model, βs, **kw)
    assert isinstance(prof, G.RingCoronaProfile) and len(prof.left_arm.radii) == 3 and np.all(prof.left_arm.weights == 0.0)
    same = G.emissivity_profile(m, d, model, time_dependent=True, βs=βs, **{k: v for k, v in kw.items() if k != "n_samples"}, n_samples=120)
    np.testing.assert_array_equal(same.right_arm.ε[1], prof.right_arm.ε[1])
    TF = G.transfer_functions
    lo = max(min(r[0] for r in prof.left_arm.radii), min(r[0] for r in prof.right_arm.radii))
    t_grid = np.linspace(0.0, 400.0, 81)
    flux = TF.integrate_lagtransfer(prof, T.branches(TF), T.G_SMALL, t_grid, n_radii=T.N_RADII, t0=0.0, n_time_steps=33)
    assert lo < 50.0 and np.all(np.isfinite(flux)) and np.all(flux >= 0.0) and flux.max() > 0.0


def test_disc_corona_profile_from_the_oracle(G, oracle):
    """disc_corona_profile: rings at linspace(1e-2, r, n_rings), all through one tracer"""
    m = G.KerrMetric(1.0, R.KERR_A)
    d, model = G.ThinDisc(0.0, 200.0), G.DiscCorona(G.SourceVelocities.co_rotating, 8.0, 3.0)
    radii = np.linspace(1e-2, 8.0, 2)
    models = [G.RingCorona(model.vf, float(r), model.h) for r in radii]
    ocfg = oracle.make_config("kerr", (1.0, R.KERR_A), disc=(0.0, 200.0), lambda_max=1_000_000.0, outer_radius=1_000_000.0, upper_hemisphere=True)
    dv = R.oracle_disc_velocity(G, oracle, m, ocfg)
    βs = np.array([0.4, 1.9])
    prof = G.disc_corona_profile(m, d, model, βs, n_rings=2, n_samples=120, extrema_iter=10, route="lockstep",
                                 tracer=R.OracleTracer(G, oracle, m, ocfg, models, βs, dv), disc_velocity=dv)
    assert isinstance(prof, G.DiscCoronaProfile) and len(prof.rings) == 2
    np.testing.assert_array_equal(prof.radii, radii)
    assert prof.propagation_velocity(3.0) == 0.0


def test_flat_space_base_rays_equal_the_closed_form(G, oracle):
    """M = 0: the base rays of 3 slices of a stationary ring (r = 8, h = 6) through the oracle; ρ and t of every hit whose straight line
    stays more than 1 away from the z axis against the closed form, rtol 2e-7 (tests/test_flat_space_exact.py's bar)."""
    m, d, models, chart = R.flat_scene(G)
    ocfg = oracle.make_config("kerr", (0.0, 0.0), disc=(0.0, 200.0), lambda_max=R.FLAT_LAMBDA, outer_radius=12000.0, upper_hemisphere=True)
    tracer = R.OracleTracer(G, oracle, m, ocfg, models, R.FLAT_βS)
    base = R.flat_base_angles(G)
    n = base.size
    rows = tracer(np.zeros(3 * n, dtype=int), np.repeat(np.arange(3), n), np.tile(base, 3))
    _, _, _, vs, pts = tracer.calls[-1]
    assert R.check_flat_rows(G, rows, pts["x_init"], vs) > 60
