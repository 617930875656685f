"""The (r, ϕ) maps and the filled image of a resident sky formed on the MI355X (gr_sky_bin_grid, gr_sky_fill,
gr_disc_area_factor; `route="device"` of gradus.jl_amd/adaptive.py) against the numpy route on the sky's mirror.  The scene of
tests/test_gpu_sky_resident.py: RingCorona r = 10, h = 4 over a Kerr hole with a = 0.998 and ThinDisc(0, ∞), trace_initial and
two steps, 40 995 cells; one resident sky for the module.  Tolerances and their reasons: tests/skymaps_scene.py; the same text on
the host: tests/test_skymaps_host.py."""
import ctypes as C
import math

import numpy as np
import pytest

import skymaps_scene as M
from test_gpu_sky_resident import assert_same, new_sky, scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(G, _ens_session):
    """the resident sky; `route="host"` reads its mirror"""
    _ens_session.set("tangent_pairs", 1)
    sky = new_sky(G, _ens_session, resident=True)
    _ens_session.set("tangent_pairs", 2)
    assert sky.resident and len(sky.grid) == 40995
    return sky


def grids(G, n_r, n_phi):
    return M.bins(scene(G)[0].isco(), 1000.0, n_r, n_phi)


@pytest.mark.parametrize("n_r,n_phi", M.BINS)
def test_the_three_maps_equal_the_host_route(G, dev, n_r, n_phi):
    m, _, d = scene(G)
    r_bins, ϕ_bins = grids(G, n_r, n_phi)
    n_max = int(dev.device_occupancy(r_bins, ϕ_bins, Γ=None).max())
    assert n_max > 20
    host = {"emissivity": G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, dev, route="host"),
            "redshift": G.bin_redshift_grid(r_bins, ϕ_bins, dev, route="host"), "time": G.bin_time_grid(r_bins, ϕ_bins, dev, route="host")}
    got = {"emissivity": G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, dev, route="device"),
           "redshift": G.bin_redshift_grid(r_bins, ϕ_bins, dev, route="device"), "time": G.bin_time_grid(r_bins, ϕ_bins, dev, route="device")}
    for what in ("redshift", "time", "emissivity"):
        assert got[what].shape == (n_r, n_phi) and 0 < np.count_nonzero(host[what]) < host[what].size
        M.assert_map(got[what], host[what], M.map_rtol(n_max, M.DELTA_F if what == "emissivity" else 0.0), f"{what} {n_r} x {n_phi}")
    # a second call gives the same bytes
    assert G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, dev, route="device").tobytes() == got["emissivity"].tobytes()
    assert G.bin_redshift_grid(r_bins, ϕ_bins, dev, route="device").tobytes() == got["redshift"].tobytes()
    assert G.bin_time_grid(r_bins, ϕ_bins, dev, route="device").tobytes() == got["time"].tobytes()
    # lit exactly where the census counts
    np.testing.assert_array_equal(got["emissivity"] != 0, dev.device_occupancy(r_bins, ϕ_bins) != 0)


def test_solid_angle_and_gamma_none(G, dev):
    m, _, d = scene(G)
    r_bins, ϕ_bins = grids(G, 37, 53)
    solid_ref, count = M.host_solid_angle(G, dev, r_bins, ϕ_bins)
    got, solid = dev.device_bin_grid("emissivity", r_bins, ϕ_bins, Γ=None, solid_angle=True)
    M.assert_map(solid, solid_ref, M.map_rtol(count.max()), "Σ ΔΩ")
    ref = G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, dev, Γ=None, route="host")
    M.assert_map(got, ref, M.map_rtol(count.max(), M.DELTA_F), "emissivity Γ=None")
    assert G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, dev, Γ=None, route="device").tobytes() == got.tobytes()
    np.testing.assert_array_equal(got != 0, dev.device_occupancy(r_bins, ϕ_bins, Γ=None) != 0)
    with_g = G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, dev, route="device")
    assert not np.array_equal(with_g, got)


def test_nan_terms_and_terms_below_the_resolution(G, dev):
    """What an integer sum cannot carry, through the kernels and the Python route (the rows of a resident sky cannot be written
    from outside, so the terms are bent through Γ).  Γ = NaN: every term g^Γ is NaN, every bin with a leaf is NaN on both routes,
    the others stay 0.  Γ = 400: g^Γ spans far more than the 2^86 the sums resolve below the largest term, bins of small g would
    read 0 where the census counts, and the call raises instead (GR_ERR_UNSUPPORTED) -- the sky stays usable."""
    m, _, d = scene(G)
    r_bins, ϕ_bins = grids(G, 37, 53)
    with np.errstate(invalid="ignore"):
        ref = G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, dev, Γ=float("nan"), route="host")
    got = G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, dev, Γ=float("nan"), route="device")
    _, count = M.host_solid_angle(G, dev, r_bins, ϕ_bins)
    np.testing.assert_array_equal(np.isnan(got), count > 0)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    assert not got[count == 0].any()
    g = dev.values["g"][dev.grid.leaves()]
    assert 400 * (np.log2(np.nanmax(g)) - np.log2(np.nanmin(g))) > 200      # (the premise: no fixed-point grid of 124 bits holds both)
    with pytest.raises(G.GradusMI355XError, match="resolution"):
        G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, dev, Γ=400, route="device")
    again = G.bin_redshift_grid(r_bins, ϕ_bins, dev, route="device")
    M.assert_map(again, G.bin_redshift_grid(r_bins, ϕ_bins, dev, route="host"), M.map_rtol(count.max()), "redshift after the refusal")


@pytest.mark.parametrize("n_theta,n_phi", M.FILLS + [(5, 3)])
def test_fill_equals_the_host_route(G, dev, n_theta, n_phi):
    ϕ_grid, θ_grid = M.single_cell_column(dev) if (n_theta, n_phi) == (5, 3) else M.fill_grids(n_theta, n_phi)
    ref, ref_cells = G.fill_sky_values(dev, (ϕ_grid, θ_grid), route="host", cells=True)
    got, got_cells = G.fill_sky_values(dev, (ϕ_grid, θ_grid), route="device", cells=True)
    assert got.shape == ref.shape == (θ_grid.size, ϕ_grid.size)
    k = int(np.argmin(np.abs(ϕ_grid + math.pi)))
    assert np.isnan(got["r"][:, k]).all() and not got_cells[0][:, k].any()
    if (n_theta, n_phi) == (5, 3):
        assert np.isnan(got["t"][:, 0]).all() and not got_cells[0][:, 0].any() and ref_cells[0][:, 1].all()
    M.assert_fill(dev, θ_grid, got, got_cells, ref, ref_cells, f"fill {n_theta} x {n_phi}")
    assert G.fill_sky_values(dev, (ϕ_grid, θ_grid), route="device").tobytes() == got.tobytes()
    if (n_theta, n_phi) == (67, 7):
        # the θ grid in any order, as the host route takes it: descending, and shuffled with one θ twice
        shuffled = np.random.default_rng(3).permutation(θ_grid)
        shuffled[5] = shuffled[40]
        for θ in (θ_grid[::-1].copy(), shuffled):
            ref, ref_cells = G.fill_sky_values(dev, (ϕ_grid, θ), route="host", cells=True)
            got, got_cells = G.fill_sky_values(dev, (ϕ_grid, θ), route="device", cells=True)
            assert got_cells[0].any()
            M.assert_fill(dev, θ, got, got_cells, ref, ref_cells, "fill, θ in another order")


def test_disc_area_factor_on_the_device(G, ens):
    """gr_disc_area_factor for Kerr and for the same hole as a tabulated metric, against numpy's lorentz_factor x _proper_area with
    the table the device read; bound: 4 δ_F (skymaps_scene.DELTA_F; the tabulated metric adds its fit's own error)"""
    from gradus_jl_amd.corona import _plunging_table, _proper_area, disc_area_factor, keplerian_velocity_projector, lorentz_factor

    kerr = G.KerrMetric(1.0, 0.9)
    for m, bound in ((kerr, 4 * M.DELTA_F), (G.TabulatedMetric(kerr), None)):
        table = _plunging_table(m, ens)
        isco = m.isco()
        r = np.concatenate([np.linspace(1.02 * float(table[0][0]), isco * (1 - 1e-6), 300), np.geomspace(isco * (1 + 1e-6), 900.0, 333)])
        x = np.zeros((r.size, 4))
        x[:, 1], x[:, 2] = r, math.pi / 2
        ref = lorentz_factor(kerr, x, keplerian_velocity_projector(kerr, plunging=table)(x)) * _proper_area(kerr, r, np.full(r.size, math.pi / 2))
        got = disc_area_factor(m, r, ensemble=ens, plunging=table, r_isco=isco)
        rel = np.abs(got / ref - 1.0)
        if bound is None:
            # a table's components and their ∂/∂r carry the error of its fit: the fit's own estimates (m.errors), amplified by at
            # most 4 on the way to γ (δ_F's reasoning), with a margin of 4
            bound = 4 * M.DELTA_F + 16 * float(m.errors[0] + m.errors[1])
        print(f"{type(m).__name__}: worst relative difference {rel.max():.3e}, bound {bound:.3e}")
        assert rel.max() <= bound


def test_refusals_leave_the_sky_usable(G, ens):
    ens.set("tangent_pairs", 1)
    sky, host = new_sky(G, ens, True, steps=0), new_sky(G, ens, False, steps=0)
    L, r, p, out = sky._L, np.geomspace(1.3, 900.0, 20), np.linspace(0.0, 2 * math.pi, 20), np.zeros((20, 20))
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    bad_r, bad_p = r.copy(), p.copy()
    bad_r[[3, 4]] = bad_r[[4, 3]]
    bad_p[7] = np.nan
    refused = [
        L.gr_sky_bin_grid(sky._dev, 0, None, 20, ptr(p), 20, None, ptr(out), None),
        L.gr_sky_bin_grid(sky._dev, 0, ptr(r), 20, None, 20, None, ptr(out), None),
        L.gr_sky_bin_grid(sky._dev, 0, ptr(r), 20, ptr(p), 20, None, None, None),
        L.gr_sky_bin_grid(sky._dev, 0, ptr(r), 0, ptr(p), 20, None, ptr(out), None),
        L.gr_sky_bin_grid(sky._dev, 0, ptr(r), 20, ptr(p), 46341, None, ptr(out), None),
        L.gr_sky_bin_grid(sky._dev, 0, ptr(bad_r), 20, ptr(p), 20, None, ptr(out), None),
        L.gr_sky_bin_grid(sky._dev, 0, ptr(r), 20, ptr(bad_p), 20, None, ptr(out), None),
        L.gr_sky_bin_grid(sky._dev, 3, ptr(r), 20, ptr(p), 20, None, ptr(out), None),
        L.gr_sky_bin_grid(sky._dev, -1, ptr(r), 20, ptr(p), 20, None, ptr(out), None),
        L.gr_sky_fill(sky._dev, None, 20, ptr(p), 20, ptr(out), None),
        L.gr_sky_fill(sky._dev, ptr(p), 0, ptr(p), 20, ptr(out), None),
    ]
    assert refused == [-1] * len(refused)          # GR_ERR_INVALID_ARGUMENT
    untraced = new_sky(G, ens, True, steps=None)
    with pytest.raises(G.GradusMI355XError, match="not been traced"):
        G.bin_redshift_grid(r, p, untraced, route="device")
    with pytest.raises(G.GradusMI355XError, match="not been traced"):
        G.fill_sky_values(untraced, (p, p), route="device")
    with pytest.raises(ValueError, match="route"):
        G.bin_time_grid(r, p, sky, route="gpu")
    # the sky works as before: the maps are there, and a step refines what the host route refines
    assert np.count_nonzero(G.bin_redshift_grid(r, p, sky, route="device")) > 0
    G.trace_step(sky)
    G.trace_step(host)
    assert_same(host, sky)


def test_route_device_needs_a_resident_sky(G, ens):
    ens.set("tangent_pairs", 1)
    m, _, d = scene(G)
    host = new_sky(G, ens, False, steps=None)
    r, p = np.geomspace(1.3, 900.0, 20), np.linspace(0.0, 2 * math.pi, 20)
    for call in (lambda: G.bin_emissivity_grid(m, d, r, p, host, route="device"), lambda: G.bin_redshift_grid(r, p, host, route="device"),
                 lambda: G.bin_time_grid(r, p, host, route="device"), lambda: G.fill_sky_values(host, 16, route="device")):
        with pytest.raises(ValueError, match="resident"):
            call()
