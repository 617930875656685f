"""The (r, ϕ) maps, the filled image and γ(r) A(r) of a resident sky (gr_sky_bin_grid, gr_sky_fill, gr_disc_area_factor) on the
host: the text the kernels run (gr_skygrid.hpp, gr_lagbin.hpp, disc_area_factor of gr_device.hpp; tests/harness_skymaps.py)
against the numpy route of gradus.jl_amd/adaptive.py and corona.py, without a GPU.  Scene: the analytic sky of
tests/test_adaptive_sky_host.py after trace_initial and two steps.  Tolerances and their reasons: tests/skymaps_scene.py; the
device's turn: tests/test_gpu_sky_maps.py."""
import copy
import math

import numpy as np
import pytest

import harness_skygrid as SG
import harness_skymaps as H
import redshift_scene as R
import skymaps_scene as M
from test_adaptive_sky_host import analytic_rows

R_LO, R_HI = 1.0, 60.0


@pytest.fixture(scope="module")
def sky(G):
    s = G.AdaptiveSky(analytic_rows, G.check_refine)
    G.trace_initial(s, level=3)
    for _ in range(2):
        G.trace_step(s)
    assert len(s.grid) == 36045
    s._values.setflags(write=False)
    return s


@pytest.fixture(scope="module")
def hsky(sky):
    return H.Sky(sky)


@pytest.mark.parametrize("what", ["redshift", "time"])
def test_redshift_and_time_maps_equal_numpy(G, sky, hsky, what):
    r_bins, ϕ_bins = M.bins(R_LO, R_HI, 37, 53)
    ref = (G.bin_redshift_grid if what == "redshift" else G.bin_time_grid)(r_bins, ϕ_bins, sky)
    solid_ref, count = M.host_solid_angle(G, sky, r_bins, ϕ_bins)
    rc, got, solid = H.bin_grid(hsky, what, r_bins, ϕ_bins)
    assert rc == 0 and got.shape == (37, 53)
    assert 50 < np.count_nonzero(ref) < ref.size and count.max() > 20
    M.assert_map(got, ref, M.map_rtol(count.max()), what)
    M.assert_map(solid, solid_ref, M.map_rtol(count.max()), "Σ ΔΩ")


def test_emissivity_map_with_a_given_area_equals_numpy(G, sky, hsky):
    """J g^Γ γA with γA handed over per cell (a smooth stand-in: the analytic sky has no metric): Γ = 2 and Γ = None"""
    r_bins, ϕ_bins = M.bins(R_LO, R_HI, 37, 53)
    area = 1.0 + np.nan_to_num(sky.values["r"]) ** 1.5
    v, ΔΩ, r_i, ϕ_i = G.adaptive._binned_cells(sky, r_bins, ϕ_bins)
    solid, count = M.host_solid_angle(G, sky, r_bins, ϕ_bins)
    for Γ in (2, None):
        w = v["J"] * ((np.ones(v.size) if Γ is None else v["g"] ** Γ) * (1.0 + v["r"] ** 1.5))
        ref = np.zeros_like(solid)
        np.add.at(ref, (r_i, ϕ_i), ΔΩ * w)
        ref[solid > 0] /= solid[solid > 0]
        rc, got, _ = H.bin_grid(hsky, "emissivity", r_bins, ϕ_bins, Γ=Γ, area=area)
        assert rc == 0
        M.assert_map(got, ref, M.map_rtol(count.max()), f"emissivity Γ={Γ}")


def test_maps_do_not_depend_on_the_order_of_the_leaves(sky, hsky):
    r_bins, ϕ_bins = M.bins(R_LO, R_HI, 37, 53)
    order = np.random.default_rng(7).permutation(np.arange(1, hsky.n + 1))
    for what in ("redshift", "time"):
        _, a, sa = H.bin_grid(hsky, what, r_bins, ϕ_bins)
        _, b, sb = H.bin_grid(hsky, what, r_bins, ϕ_bins, order=order)
        _, c, sc = H.bin_grid(hsky, what, r_bins, ϕ_bins, order=order[::-1])
        assert a.tobytes() == b.tobytes() == c.tobytes() and sa.tobytes() == sb.tobytes() == sc.tobytes()


def test_a_nan_row_makes_its_bin_nan_on_both_routes(G, sky):
    r_bins, ϕ_bins = M.bins(R_LO, R_HI, 37, 53)
    binned = SG.bins(SG.Grid(sky.grid), sky.values, r_bins, ϕ_bins, Γ=None)[0]
    victim = int(binned[len(binned) // 2])
    twin = copy.copy(sky)
    twin._values = sky._values.copy()
    twin._values["g"][victim] = np.nan
    assert np.isfinite(twin.values["r"][victim])
    ref = G.bin_redshift_grid(r_bins, ϕ_bins, twin)
    rc, got, _ = H.bin_grid(H.Sky(twin), "redshift", r_bins, ϕ_bins)
    assert rc == 0 and np.isnan(ref).sum() == 1
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    # ... and the time map of the same rows is untouched by it
    assert not np.isnan(H.bin_grid(H.Sky(twin), "time", r_bins, ϕ_bins)[1]).any()


def test_a_term_below_the_resolution_of_the_sums_is_refused_not_dropped(G, sky):
    """one leaf alone in its bin with t = 1e-300 beside t ~ 10: its term is below the resolution of the sums (2^-86 of the largest
    here), the map would be 0 in a bin the census counts"""
    r_bins, ϕ_bins = M.bins(R_LO, R_HI, 37, 53)
    _, count = M.host_solid_angle(G, sky, r_bins, ϕ_bins)
    alone = np.argwhere(count == 1)
    assert alone.size
    leaf, ri, pi, _ = SG.bins(SG.Grid(sky.grid), sky.values, r_bins, ϕ_bins, Γ=None)
    victim = int(leaf[(ri == alone[0][0]) & (pi == alone[0][1])][0])
    twin = copy.copy(sky)
    twin._values = sky._values.copy()
    twin._values["t"][victim] = 1e-300
    rc, got, _ = H.bin_grid(H.Sky(twin), "time", r_bins, ϕ_bins)
    assert rc == -2 and got[alone[0][0], alone[0][1]] == 0.0


@pytest.mark.parametrize("n_theta,n_phi", M.FILLS + [(5, 3)])
def test_fill_equals_fill_sky_values(G, sky, hsky, n_theta, n_phi):
    ϕ_grid, θ_grid = M.single_cell_column(sky) if (n_theta, n_phi) == (5, 3) else M.fill_grids(n_theta, n_phi)
    ref, ref_cells = G.fill_sky_values(sky, (ϕ_grid, θ_grid), cells=True)
    assert G.fill_sky_values(sky, (ϕ_grid, θ_grid)).tobytes() == ref.tobytes()
    got, lower, upper, columns, bad = H.fill(hsky, ϕ_grid, θ_grid)
    assert bad == 0
    # the domain's boundary: no cell, a NaN column with cells 0, 0
    k = int(np.argmin(np.abs(ϕ_grid + math.pi)))
    assert columns[k].size == 0 and np.isnan(ref["r"][:, k]).all() and not lower[:, k].any()
    if (n_theta, n_phi) == (5, 3):
        assert columns[0].size == 1 and columns[1].size >= 2
        assert np.isnan(got[:, 0, :]).all() and not lower[:, 0].any() and ref_cells[0][:, 1].all()
    else:
        assert max(c.size for c in columns) > 20
    # the claim the kernel rests on: the cells in the order the column meets them ARE the sorted set of the reference
    for k, ph in enumerate(ϕ_grid):
        held = {sky.grid.get_parent_index(c, ph) for c in np.cos(θ_grid)} - {0}
        held = np.fromiter(held, dtype=np.int64, count=len(held))
        held = held[np.argsort(np.arccos(sky.grid.pos[held, 0]), kind="stable")]
        np.testing.assert_array_equal(columns[k], held)
    M.assert_fill(sky, θ_grid, got, (lower, upper), ref, ref_cells, f"fill {n_theta} x {n_phi}")
    # the carries of the two scans: chunks of 64 and of 7 points give the same bytes as chunks of 256
    for chunk in (64, 7):
        again = H.fill(hsky, ϕ_grid, θ_grid, chunk=chunk)
        assert again[0].tobytes() == got.tobytes() and again[1].tobytes() == lower.tobytes() and again[2].tobytes() == upper.tobytes()


def test_fill_takes_the_theta_grid_in_any_order(G, sky, hsky):
    """the host route sorts nothing and needs nothing sorted; the kernel's column walk needs θ ascending, so the driver walks the
    grid in ascending order and stores at the caller's indices: descending and shuffled grids, one with a repeated θ"""
    ϕ_grid, θ_grid = M.fill_grids(67, 7)
    shuffled = np.random.default_rng(3).permutation(θ_grid)
    shuffled[5] = shuffled[40]
    for θ in (θ_grid[::-1].copy(), shuffled):
        ref, ref_cells = G.fill_sky_values(sky, (ϕ_grid, θ), cells=True)
        got, lower, upper, _, bad = H.fill(hsky, ϕ_grid, θ)
        assert bad == 0 and lower.any()
        M.assert_fill(sky, θ, got, (lower, upper), ref, ref_cells, "fill, θ in another order")


def test_infinite_terms_come_out_as_numpy_sums_them(G, sky):
    """a +∞ t makes its bin +∞, a +∞ and a -∞ in one bin make it NaN, as np.add.at does"""
    r_bins, ϕ_bins = M.bins(R_LO, R_HI, 37, 53)
    leaf, ri, pi, _ = SG.bins(SG.Grid(sky.grid), sky.values, r_bins, ϕ_bins, Γ=None)
    _, count = M.host_solid_angle(G, sky, r_bins, ϕ_bins)
    a, b = np.argwhere(count >= 2)[0]
    pair = leaf[(ri == a) & (pi == b)][:2]
    other = int(leaf[(ri != a) | (pi != b)][0])
    twin = copy.copy(sky)
    twin._values = sky._values.copy()
    twin._values["t"][pair] = [np.inf, -np.inf]
    twin._values["t"][other] = np.inf
    with np.errstate(invalid="ignore"):
        ref = G.bin_time_grid(r_bins, ϕ_bins, twin)
    rc, got, _ = H.bin_grid(H.Sky(twin), "time", r_bins, ϕ_bins)
    assert rc == 0 and np.isnan(ref[a, b]) and np.isposinf(ref).sum() == 1
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(ref))
    finite = np.isfinite(ref)
    np.testing.assert_allclose(got[finite], ref[finite], rtol=M.map_rtol(count.max()), atol=0.0)


@pytest.mark.parametrize("name,params,cls", R.CASES, ids=R.CASE_IDS)
def test_disc_area_factor_equals_lorentz_factor_times_proper_area(G, oracle, name, params, cls):
    """γ(r) A(r) of the kernel text against numpy, radii on both sides of the ISCO, inside it the oracle's plunging table of the
    case (from 1.02 x its first radius: the rows the table's invariants hold on).  Bound: skymaps_scene.AREA_MARGIN; the largest
    figure printed here is δ_F (skymaps_scene.DELTA_F, DESIGN_measurements.md §M33).

    Measured: <= 3.0e-15 (Kerr, inside the ISCO) for every case -- except in the window corona_radius ± 1.25 of Kerr-refractive,
    where the refractive index runs from n to 1: there the two differ by up to 1.6e-2 (19.9: 1.60e-2, 20.1: 1.35e-2, 19.03 and
    20.91: 1.7e-4; equal again within 1e-2 of the step itself), because metrics.KerrRefractive._components takes the index at the
    VALUE of r (`_value(r)`), so numpy's circular_fourvelocity differentiates g without ∂n/∂r, while the kernels' `eval` carries
    it.  Two existing routes of the project that the redshift tests already hold apart (redshift_scene.OUTSIDE_BOUND); neither is
    changed here.  The window's radii are compared, printed and held to WINDOW_BOUND, outside it the case meets AREA_MARGIN."""
    from gradus_jl_amd.corona import _proper_area, keplerian_velocity_projector, lorentz_factor

    WINDOW_BOUND = 5e-2          # (no derived figure: a sanity bound on a documented disagreement of the two existing routes)
    m = R.metric(G, cls, params)
    _, table = R.oracle_table(oracle, name, params)
    isco = m.isco()
    r_from = R.R_FROM * float(table[0][0])
    assert r_from < isco < float(table[0][-1]) * (1 + 1e-6)
    r = np.concatenate([np.linspace(r_from, isco * (1 - 1e-6), 40), np.geomspace(isco * (1 + 1e-6), 1000.0, 60),
                        [19.03, 19.5, 19.9, 20.1, 20.5, 20.91]])
    x = np.zeros((r.size, 4))
    x[:, 1], x[:, 2] = r, math.pi / 2
    ref = lorentz_factor(m, x, keplerian_velocity_projector(m, plunging=table)(x)) * _proper_area(m, r, np.full(r.size, math.pi / 2))
    got = H.area_factor(G, m, r, isco, table)
    rel = np.abs(got / ref - 1.0)
    window = np.abs(r - 20.0) <= 1.25 if name == "kerr-refractive" else np.zeros(r.size, dtype=bool)
    inside = (r < isco) & ~window
    print(f"{name}: γA in [{ref.min():.4g}, {ref.max():.4g}], worst relative difference inside the ISCO {rel[inside].max():.3e}, "
          f"outside {rel[~inside & ~window].max():.3e}" + (f", in the index window {rel[window].max():.3e}" if window.any() else ""))
    assert np.all(np.isfinite(ref)) and np.all(ref > 0)
    assert inside.sum() == 40 and (~inside & ~window).sum() >= 50
    assert rel[~window].max() <= M.AREA_MARGIN
    assert not window.any() or rel[window].max() <= WINDOW_BOUND
