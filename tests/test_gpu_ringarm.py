"""The producer of ring and disc corona profiles on the device: gr_ring_rays (kernel k_ring_rays + the ray-summary trace) against
rays the CPU oracle traces from numpy-formed velocities, and against the flat-space closed form; gr_ring_arms (k_ring_bracket,
k_ring_probe, k_ring_update, k_ring_pack) against the lock-step route, which runs the same logic in numpy over gr_ring_rays -- bit
for bit; a slice without a hit; and model -> DiscCoronaProfile -> integrate_lagtransfer on the device against the host integral."""
import math

import numpy as np
import pytest

import harness_ringarm as R
import harness_tfint as H
import harness_tftd as T

pytestmark = pytest.mark.gpu

βS3 = np.array([0.0, 0.9, 2.2])


@pytest.fixture(scope="module")
def two_rings(G, _ens_session, oracle):
    """2 rings (r = 4 and 8, h = 3, co-rotating, Kerr a = 0.9, ThinDisc(0, 300)), 3 slices, 500 angles each: 3000 rays through
    gr_ring_rays and through the oracle (which against itself at a tenfold tighter tolerance differs by 1e-8 in ρ, t and g and in no
    status on this scene)."""
    ens = _ens_session
    ens.set("kernel", 2).set("precision", 64)
    m, d, models = R.kerr_scene(G, radii=(4.0, 8.0), h=3.0, r_out=300.0)
    θ = (np.arange(500) + 0.5) / 500 * 2 * math.pi
    ring, sl, ang = np.repeat(np.arange(2), 1500), np.tile(np.repeat(np.arange(3), 500), 2), np.tile(θ, 6)
    tracer = G.corona.RingTracer(m, d, models, βS3, ensemble=ens)
    rows, v = tracer(ring, sl, ang, velocities=True)
    ocfg = oracle.make_config("kerr", (1.0, R.KERR_A), disc=(0.0, 300.0), lambda_max=1_000_000.0, outer_radius=1_000_000.0, upper_hemisphere=True)
    ref = R.OracleTracer(G, oracle, m, ocfg, models, βS3, R.oracle_disc_velocity(G, oracle, m, ocfg))
    want = ref(ring, sl, ang)
    return m, ring, rows, v, want, ref.calls[-1][3]


def test_ring_rays_equal_oracle_traced_rays(G, two_rings):
    m, ring, rows, _, want, _ = two_rings
    st, st_ref = rows[:, 3].astype(int), want[:, 3].astype(int)
    n_diff = int(np.sum(st != st_ref))
    print(f"statuses differ on {n_diff} of {st.size} rays")
    assert n_diff <= 0.002 * st.size
    for k in (0, 1):                       # each ring against its own source velocity
        hit = (ring == k) & (st == R.HIT) & (st_ref == R.HIT)
        out = hit & (want[:, 1] > 1.05 * m.isco())
        assert hit.sum() > 500 and out.sum() > 400
        for c in (1, 2):
            print(f"ring {k} column {c}: {np.max(np.abs(rows[hit, c] / want[hit, c] - 1.0)):.3e}")
        print(f"ring {k} g: {np.max(np.abs(rows[out, 0] / want[out, 0] - 1.0)):.3e}")
        np.testing.assert_allclose(rows[hit, 1], want[hit, 1], rtol=1e-6)
        np.testing.assert_allclose(rows[hit, 2], want[hit, 2], rtol=1e-6)
        np.testing.assert_allclose(rows[out, 0], want[out, 0], rtol=1e-6)
    assert np.all(np.isnan(rows[st != R.HIT, 0]))


def test_formed_velocities_equal_numpy(two_rings):
    _, _, _, v, _, v_numpy = two_rings
    err = np.abs(v - v_numpy).max()
    print(f"v_out - numpy: {err:.3e}, max |v| {np.abs(v_numpy).max():.3e}")
    np.testing.assert_allclose(v, v_numpy, rtol=0.0, atol=1e-12 * np.abs(v_numpy).max())


def test_flat_space_closed_form_through_ring_rays(G, ens):
    m, d, models, chart = R.flat_scene(G)
    tracer = G.corona.RingTracer(m, d, models, R.FLAT_βS, chart=chart, ensemble=ens)
    base = R.flat_base_angles(G)
    n = base.size
    rows, v = tracer(np.zeros(3 * n, dtype=int), np.repeat(np.arange(3), n), np.tile(base, 3), velocities=True)
    assert R.check_flat_rows(G, rows, np.tile(tracer.xs[0], (3 * n, 1)), v) > 60


SHAPES = {"2x5": ((5.0, 8.0), np.linspace(0.1, 2.9, 5)), "3x13": ((4.0, 6.5, 9.0), np.linspace(0.0, math.pi - math.pi / 13, 13))}


@pytest.mark.parametrize("extrema_iter", [6, 20])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ring_arms_equal_the_lockstep_route_bit_for_bit(G, ens, shape, extrema_iter):
    """2 rings x 5 slices = 20 searches (a partly filled wave), 3 x 13 = 78 (more than one); n_samples = 120"""
    K = G.corona
    radii, βs = SHAPES[shape]
    m, d, models = R.kerr_scene(G, radii=radii)
    tracer = K.RingTracer(m, d, models, βs, ensemble=ens)
    base = K.ring_base_angles(120, extrema_iter)
    rows, counts = tracer.arms(base, extrema_iter)
    searches = {}
    rows_ls, counts_ls = K.lockstep_arm_traces(tracer, len(models), βs.size, base, extrema_iter, searches_out=searches)
    assert np.all(counts[..., 0] == base.size) and np.all(counts[..., 1:] >= 0)
    np.testing.assert_array_equal(counts, counts_ls)
    assert rows.tobytes() == rows_ls.tobytes()
    assert len(searches) == 2 * len(models) * βs.size and all(s.done and s.n == extrema_iter for s in searches.values())
    if extrema_iter == 6:
        assert any(s.too_many for s in searches.values())              # ended by the too_many_iters arm
    else:
        assert any(not s.too_many for s in searches.values())          # ended at n == extrema_iter on kept probes alone
    print(f"{shape} E={extrema_iter}: kept {int(counts[..., 1:].sum())} probes, {tracer.launches} gr_ring_rays calls on the lock-step route, "
          f"{sum(s.too_many for s in searches.values())} of {len(searches)} searches past extrema_iter")
    if shape == "2x5":
        # the slices in another order: the same rows per slice
        perm = np.array([3, 0, 4, 2, 1])
        rows_p, counts_p = K.RingTracer(m, d, models, βs[perm], ensemble=ens).arms(base, extrema_iter)
        np.testing.assert_array_equal(counts_p, counts[:, perm])
        assert rows_p.tobytes() == np.ascontiguousarray(rows[:, perm]).tobytes()


def test_a_slice_without_a_hit_is_an_error_not_a_fault(G, ens):
    """a ThinDisc inside the horizon (r < 0.5): no ray of any slice reaches it"""
    K = G.corona
    m, _, models = R.kerr_scene(G)
    d = G.ThinDisc(0.0, 0.5)
    βs = np.array([0.3, 1.7])
    tracer = K.RingTracer(m, d, models, βs, ensemble=ens)
    base = K.ring_base_angles(52, 6)
    rows, counts = tracer.arms(base, 6)
    assert counts.reshape(-1, 3).tolist() == [[40, -1, -1], [40, -1, -1]]
    assert np.all(rows[:, :, :40, 4] != R.HIT) and np.all(rows[:, :, 40:] == 0.0)
    for route in ("device", "lockstep"):
        with pytest.raises(ValueError, match=r"no base ray met the disc in \(ring 0, slice 0\), \(ring 0, slice 1\)"):
            G.corona_arms(m, d, models[0], βs, n_samples=52, extrema_iter=6, ensemble=ens, route=route)
    # ... and any other geometry is refused by the library itself
    from gradus_jl_amd import _lib

    tracer.cfg.disc_id = 2
    with pytest.raises(_lib.GradusMI355XError) as ei:
        tracer.arms(base, 6)
    assert ei.value.code == -2


def test_model_to_profile_to_lag_transfer_on_the_device(G, ens):
    """disc_corona_profile -> integrate_lagtransfer(..., ensemble=) against the host integral of the same profile, at the bound
    tests/test_gpu_tftd.py holds that comparison to; ring_corona_profile and the emissivity_profile dispatch on the way"""
    TF = G.transfer_functions
    m = G.KerrMetric(1.0, R.KERR_A)
    d, model = G.ThinDisc(0.0, 200.0), G.DiscCorona(G.SourceVelocities.co_rotating, 8.0, 3.0)
    βs = np.array([0.2, 1.0, 1.9, 2.8])
    prof = G.disc_corona_profile(m, d, model, βs, n_rings=2, n_samples=120, extrema_iter=10, ensemble=ens)
    assert isinstance(prof, G.DiscCoronaProfile) and len(prof.rings) == 2 and len(prof.rings[0].left_arm.radii) == 4
    same = G.emissivity_profile(m, d, model, time_dependent=True, βs=βs, n_rings=2, n_samples=120, extrema_iter=10, ensemble=ens)
    assert all(np.array_equal(a, b) for a, b in zip(same.rings[1].right_arm.ε, prof.rings[1].right_arm.ε))
    ring = G.ring_corona_profile(m, d, G.RingCorona(model.vf, 8.0, model.h), βs, n_samples=120, extrema_iter=10, ensemble=ens)
    assert isinstance(ring, G.RingCoronaProfile)
    assert all(np.array_equal(a, b) for a, b in zip(ring.left_arm.radii, prof.rings[1].left_arm.radii))          # ring 1 of the disc is this ring
    t_grid = np.linspace(0.0, 400.0, 81)
    for p in (prof, ring):
        host, n_host = T.host_lagtransfer(TF, p, T.branches(TF), T.G_SMALL, t_grid, t0=0.0, g_grid_upscale=1, n_time_steps=33)
        dev = TF.integrate_lagtransfer(p, T.branches(TF), T.G_SMALL, t_grid, n_radii=T.N_RADII, t0=0.0, n_time_steps=33, ensemble=ens)
        assert np.all(np.isfinite(host)) and host.max() > 0.0
        err, moved = H.lag_error(dev, host, n_host)
        print(f"device - host {err:.3e} of the peak, {moved} of {n_host} deposits moved")
        assert err <= T.TOL
