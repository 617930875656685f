"""The 2-D lag-energy transfer function binned on the device (lagtransfer_device -> binflux: gr_lagtransfer_trace,
gr_lagtransfer_extrema, gr_lagtransfer_bin) against numpy on the rows the device keeps and against the host route
`lagtransfer` + `binflux` (152-byte end points, apply_pointfunction, np.add.at).

Reference: src/transfer-functions/transfer-functions-2d.jl:98-242, test/transfer-functions/test-2d.jl:4-33.

The parity tests print what they measure (edge distances of the input, non-empty cells, largest difference) before they assert.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def recorded_scene(G):
    """test-2d.jl:4-33 with a golden-spiral sampler: 337 hits of the observer's plane, 58 of the corona"""
    m = G.KerrMetric(M=1.0, a=0.998)
    x = np.array([0.0, 1e6, math.radians(30), 0.0])
    plane = G.PolarPlane(G.GeometricGrid(), Nr=20, Nθ=20)
    d = G.ThinDisc(m.isco(), 500.0)
    model = G.LampPostModel(h=10.0, θ=math.radians(0.0001))
    kw = dict(plane=plane, n_samples=100, sampler=G.EvenSampler(domain=G.BothHemispheres(), generator=G.GoldenSpiralGenerator()))
    return m, x, d, model, kw


def wide_scene(G):
    """64 x 64 rays: 4096 rows, 16 workgroups of 256 in the reductions"""
    m = G.KerrMetric(M=1.0, a=0.998)
    x = np.array([0.0, 1000.0, math.radians(60), 0.0])
    plane = G.PolarPlane(G.GeometricGrid(), Nr=64, Nθ=64, r_max=50.0)
    d = G.ThinDisc(m.isco(), 500.0)
    model = G.LampPostModel(h=10.0, θ=math.radians(0.0001))
    kw = dict(plane=plane, n_samples=1000, sampler=G.EvenSampler(domain=G.BothHemispheres(), generator=G.GoldenSpiralGenerator()))
    return m, x, d, model, kw


def edge_distance(values, lims, N):
    """smallest distance of a value inside the axis from an edge of linspace(*lims, N), in units of the axis range.  The
    values AT the limits are left out: where the limits are the extrema of the values, the first and the last edge are those
    very numbers (linspace returns its end points exactly), and a value equal to an edge has its cell without rounding."""
    edges = np.linspace(lims[0], lims[1], N)
    v = values[(values > lims[0]) & (values < lims[1])]
    return float(np.min(np.abs(v[:, None] - edges[None, :]))) / (lims[1] - lims[0])


def numpy_binflux(G, tf, profile=None, *, N_E, N_t, E0=6.4):
    """binflux on the rows read back from the device: E, t, f formed in numpy, binned by bin_transfer_function.  Asserts the
    precondition on the input first: no hit within 1e-9 of the axis range of an edge (one rounding could move its cell)."""
    RV = G.reverberation
    rows = RV.lag_rows(tf)
    assert rows.shape == (tf.n_rays, 4)
    hit = ~np.isnan(rows[:, 0])
    assert int(hit.sum()) == tf.n_hits
    g, ρ, t_obs, area = rows[hit].T
    profile = RV.AnalyticRadialDiscProfile(lambda r: r ** -3.0, tf.coronal_geodesics) if profile is None else profile
    E, t = g * E0, profile.coordtime_at(ρ) + t_obs
    f = g ** 3 * profile.emissivity_at(ρ) * area
    d_E, d_t = edge_distance(E, (E.min(), E.max()), N_E), edge_distance(t, (t.min(), t.max()), N_t)
    print(f"edge distance: E {d_E:.3e}, t {d_t:.3e} of the axis range ({N_E} x {N_t} cells, {hit.sum()} hits)")
    assert d_E > 1e-9 and d_t > 1e-9
    tb, eb, matrix = RV.bin_transfer_function(t, E, f / f.sum(), N_E=N_E, N_t=N_t)
    return tb - tf.x[1], eb, matrix


def assert_same_matrix(got, want, rel=1e-12):
    """same non-empty cells, every cell within `rel` (a few hundred additions of one rounding each against an exact sum)"""
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    full = ~np.isnan(want)
    err = float(np.max(np.abs(got[full] / want[full] - 1.0)))
    print(f"{int(full.sum())} non-empty cells, largest relative difference {err:.3e}")
    assert err <= rel


def assert_parity(G, tf, profile=None, *, N_E, N_t):
    t_ref, E_ref, f_ref = numpy_binflux(G, tf, profile, N_E=N_E, N_t=N_t)
    t_dev, E_dev, f_dev = G.binflux(tf, profile, N_E=N_E, N_t=N_t)
    assert t_dev.tobytes() == t_ref.tobytes() and E_dev.tobytes() == E_ref.tobytes()
    assert_same_matrix(f_dev, f_ref)
    return f_dev


def test_recorded_scene_hit_counts(G, ens):
    m, x, d, model, kw = recorded_scene(G)
    tf = G.lagtransfer_device(m, x, d, model, ensemble=ens, **kw)
    assert isinstance(tf, G.DeviceLagTransfer)
    assert tf.n_hits == 337 and tf.n_rays == 400 and len(tf.coronal_geodesics.geodesic_points) == 58
    assert tf.max_t == 2e6 and tf.ensemble is ens
    rows = G.reverberation.lag_rows(tf)
    # the area column: r_i² of the plane, for every ray
    assert rows[:, 3].tobytes() == np.ascontiguousarray(G.unnormalized_areas(kw["plane"]).ravel(order="F")).tobytes()


@pytest.mark.parametrize("N", [100, 8])          # 100 x 100: global atomics; 8 x 8: the histogram in LDS
def test_binning_is_numpys_on_the_same_rows(G, ens, N):
    m, x, d, model, kw = recorded_scene(G)
    tf = G.lagtransfer_device(m, x, d, model, ensemble=ens, **kw)
    f = assert_parity(G, tf, N_E=N, N_t=N)
    assert f.shape == (N, N)


def test_limits_given_by_the_caller_clamp_into_the_end_bins(G, ens):
    m, x, d, model, kw = recorded_scene(G)
    tf = G.lagtransfer_device(m, x, d, model, ensemble=ens, **kw)
    t, E, f = G.binflux(tf, N_E=8, N_t=8)
    elims = (E[0] + 0.25 * (E[-1] - E[0]), E[-1] - 0.25 * (E[-1] - E[0]))
    tlims = (t[0] + x[1] + 0.1 * (t[-1] - t[0]), t[-1] + x[1] - 0.4 * (t[-1] - t[0]))
    t2, E2, f2 = G.binflux(tf, N_E=12, N_t=12, energy_lims=elims, time_lims=tlims)
    assert E2[0] == elims[0] and E2[-1] == elims[1] and t2[0] + x[1] == pytest.approx(tlims[0], rel=1e-15)
    de, dt = E2[1] - E2[0], t2[1] - t2[0]
    assert float(np.nansum(f2)) * de * dt == pytest.approx(1.0, rel=1e-12)          # nothing lost: all hits are in a cell
    assert float(np.nansum(f2[[0, -1], :])) > 0.0 and float(np.nansum(f2[:, [0, -1]])) > 0.0


def test_route_parity_with_lagtransfer_and_binflux(G, ens):
    m, x, d, model, kw = recorded_scene(G)
    host = G.lagtransfer(m, x, d, model, ensemble=ens, **kw)
    t_h, E_h, f_h = G.binflux(host, ensemble=ens, N_E=100, N_t=100)
    tf = G.lagtransfer_device(m, x, d, model, ensemble=ens, **kw)
    t_d, E_d, f_d = G.binflux(tf, N_E=100, N_t=100)
    assert host.observer_to_disc.size == tf.n_hits == 337
    print(f"nansum: host route {np.nansum(f_h)!r}, device route {np.nansum(f_d)!r}")
    assert float(np.nansum(f_d)) == pytest.approx(float(np.nansum(f_h)), rel=1e-9)
    de, dt = E_d[1] - E_d[0], t_d[1] - t_d[0]
    assert float(np.nansum(f_d)) * de * dt == pytest.approx(1.0, rel=1e-12)
    assert float(np.nansum(f_d)) == pytest.approx(3.9126785201177956, abs=1e-2)          # test-2d.jl:33 and its tolerance


def test_more_than_one_workgroup(G, ens):
    m, x, d, model, kw = wide_scene(G)
    tf = G.lagtransfer_device(m, x, d, model, ensemble=ens, **kw)
    assert tf.n_rays == 4096 and tf.n_hits > 1024
    assert_parity(G, tf, N_E=16, N_t=16)


def test_same_bytes_on_every_run_and_launch_shape(G, ens):
    m, x, d, model, kw = wide_scene(G)
    tf = G.lagtransfer_device(m, x, d, model, ensemble=ens, **kw)
    first = [G.binflux(tf, N_E=16, N_t=16)[2], G.binflux(tf, N_E=100, N_t=100)[2]]
    again = [G.binflux(tf, N_E=16, N_t=16)[2], G.binflux(tf, N_E=100, N_t=100)[2]]
    ens.set("block", 128)
    tf2 = G.lagtransfer_device(m, x, d, model, ensemble=ens, **kw)
    other = [G.binflux(tf2, N_E=16, N_t=16)[2], G.binflux(tf2, N_E=100, N_t=100)[2]]
    for a, b, c in zip(first, again, other):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    with pytest.raises(RuntimeError, match="stale"):          # tf's rows are gone: the context holds tf2's
        G.binflux(tf, N_E=16, N_t=16)


def test_tabulated_profile_and_untouched_rows(G, ens):
    """A RadialDiscProfile (emissivity_profile: gr_corona_trace / gr_corona_bin on the SAME context, between the trace and
    the bins) gives ε and the coordtime as tables; the lag rows are left alone by it, and it by them."""
    m, x, d, model, kw = recorded_scene(G)
    tf = G.lagtransfer_device(m, x, d, model, ensemble=ens, **kw)
    before = G.binflux(tf, N_E=8, N_t=8)[2]
    sampler = G.EvenSampler(domain=G.BothHemispheres(), generator=G.GoldenSpiralGenerator())
    prof = G.emissivity_profile(m, d, model, n_samples=2000, sampler=sampler, N=40, ensemble=ens)
    assert isinstance(prof, G.corona.RadialDiscProfile)
    assert G.binflux(tf, N_E=8, N_t=8)[2].tobytes() == before.tobytes()
    assert_parity(G, tf, prof, N_E=8, N_t=8)
    again = G.emissivity_profile(m, d, model, n_samples=2000, sampler=sampler, N=40, ensemble=ens)
    assert again.ε.tobytes() == prof.ε.tobytes() and again.t.tobytes() == prof.t.tobytes()
    # an analytic profile with a power law other than the default, and one the device does not evaluate
    RV = G.reverberation
    assert_parity(G, tf, RV.AnalyticRadialDiscProfile(G.PowerLawEmissivity(2.0), tf.coronal_geodesics), N_E=8, N_t=8)
    with pytest.raises(NotImplementedError, match="lagtransfer \\+ binflux"):
        G.binflux(tf, RV.AnalyticRadialDiscProfile(lambda r: r ** -3.0, tf.coronal_geodesics))


def test_no_trace_and_no_hits_are_errors(G, ens):
    m, x, d, model, kw = recorded_scene(G)
    tf = G.lagtransfer_device(m, x, d, model, ensemble=ens, **kw)
    fresh = G.EnsembleMI355X(0)
    try:
        orphan = G.DeviceLagTransfer(tf.max_t, tf.x, tf.coronal_geodesics, fresh, tf.n_hits, tf.n_rays)
        with pytest.raises(G.GradusMI355XError, match="last gr_lagtransfer_trace: there is none"):
            G.binflux(orphan)
        # a plane that misses the disc: an annulus far outside a plane of radius 5
        small = G.PolarPlane(G.GeometricGrid(), Nr=20, Nθ=20, r_max=5.0)
        with pytest.raises(ValueError, match="reached the disc"):
            G.lagtransfer_device(m, x, G.ThinDisc(400.0, 500.0), model, ensemble=fresh, **dict(kw, plane=small))
        # ... its rows are there, with no hit among them: the library refuses to reduce them
        empty = G.DeviceLagTransfer(tf.max_t, tf.x, tf.coronal_geodesics, fresh, 0, 400)
        assert np.all(np.isnan(G.reverberation.lag_rows(empty)[:, 0]))
        with pytest.raises(G.GradusMI355XError, match="met the geometry"):
            G.binflux(empty)
    finally:
        fresh.ctx.close()
    assert G.binflux(tf, N_E=8, N_t=8)[2].shape == (8, 8)          # the session's context still holds its rows
    multi = G.EnsembleMI355X(devices=[0, 0])
    with pytest.raises(NotImplementedError, match="one context"):
        G.lagtransfer_device(m, x, d, model, ensemble=multi, **kw)
