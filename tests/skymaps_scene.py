"""What tests/test_skymaps_host.py (the kernel text on the host) and tests/test_gpu_sky_maps.py (the device) share: the bin and
fill grids, the single-cell column and the tolerances of a resident sky's (r, ϕ) maps and filled image against the numpy route
of gradus.jl_amd/adaptive.py.

Tolerances (derived, none taken from the code under test):
  * a map bin: every summed term is >= 0 (ΔΩ, g, t, J, γA), so a floating sum of n of them in any order is within (n - 1) 2^-53
    relative of exact -- numpy's numerator and denominator together 2 n 2^-53 -- and the integer sums of the kernels are exact to
    below an ulp.  16 ulp more for sin(acos x) and pow between numpy and the other math library, a margin of 4:
    rtol = 4 (2 n_max + 16) 2^-53 with n_max the largest number of leaves in a bin; the emissivity map adds 4 δ_F for γ(r) A(r).
  * δ_F: the largest relative difference between disc_area_factor (the kernel text, compiled for the host) and numpy's
    lorentz_factor x _proper_area over the seven metrics of tests/redshift_scene.py, radii on both sides of the ISCO: two
    implementations of one formula on one CPU.  Measured 3.0e-15 (DESIGN_measurements.md §M33; outside the index window of
    Kerr-refractive, where the two existing routes disagree by 1.6e-2 -- tests/test_skymaps_host.py): DELTA_F, what the device
    tests add 4 x of.  The host test that measures it asserts AREA_MARGIN = 256 x 2^-53 instead, so that another math library's
    last bits do not fail it: γA is some sixty operations whose worst amplifications are γ² V² <= 4 from V to γ = 1 / √(1 - V²)
    and the cancellation in Ω's discriminant (∂g_tϕ)² - ∂g_tt ∂g_ϕϕ, a few ulp each way through two libraries.
  * a filled point, per field: (8 2^-53 π / (θ_k+1 - θ_k) + 8 2^-53) (|v1| + |v2|) from the host's own column: w = (θ - θ_k) /
    (θ_k+1 - θ_k) moves by a few ulp of π over the interval's width when acos differs by an ulp or two.
"""
import math

import numpy as np

ULP = 2.0 ** -53
DELTA_F = 3.0e-15                      # measured on the host, §M33
AREA_MARGIN = 256.0 * ULP              # the host test's own assertion on disc_area_factor against numpy
BINS = [(100, 100), (37, 53)]          # unequal counts: a transposed stride shows
FILLS = [(300, 5), (67, 7)]            # θ x ϕ: more points than a block of 256, not a multiple of a wave, few columns


def bins(r_lo, r_hi, n_r, n_ϕ):
    return np.geomspace(r_lo, r_hi, n_r), np.linspace(0.0, 2.0 * math.pi, n_ϕ)


def fill_grids(n_θ, n_ϕ):
    """(ϕ grid, θ grid): ϕ from -π -- the domain's boundary, where no cell holds a point: a NaN column -- to 3"""
    return np.linspace(-math.pi, 3.0, n_ϕ), np.linspace(0.0, math.pi, n_θ)


def map_rtol(n_max, delta_f=0.0):
    return 4.0 * (2.0 * n_max + 16.0) * ULP + 4.0 * delta_f


def host_solid_angle(G, sky, r_bins, ϕ_bins):
    """(Σ ΔΩ per bin, leaves per bin) as adaptive._bin_grid forms them"""
    _, ΔΩ, r_i, ϕ_i = G.adaptive._binned_cells(sky, r_bins, ϕ_bins)
    solid, count = np.zeros((len(r_bins), len(ϕ_bins))), np.zeros((len(r_bins), len(ϕ_bins)), dtype=np.int64)
    np.add.at(solid, (r_i, ϕ_i), ΔΩ)
    np.add.at(count, (r_i, ϕ_i), 1)
    return solid, count


def assert_map(got, ref, rtol, label=""):
    """the NaN and the zero pattern are the reference's; everything else within rtol.  Prints the worst figure first."""
    got, ref = np.asarray(got), np.asarray(ref)
    both = np.isfinite(got) & np.isfinite(ref) & (ref != 0)
    worst = float(np.max(np.abs(got[both] / ref[both] - 1.0))) if both.any() else 0.0
    print(f"{label}: {int(both.sum())} bins compared, worst relative difference {worst:.3e}, bound {rtol:.3e}")
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(got == 0, ref == 0)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=0.0, equal_nan=True)


def fill_bounds(sky, θ_grid, lower, upper):
    """per field the bound of every filled point, from the host's own column: the cells `lower` / `upper` [θ, ϕ] of the host
    route; NaN where the column is NaN"""
    θ_lo, θ_hi = np.arccos(sky.grid.pos[lower, 0]), np.arccos(sky.grid.pos[upper, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        factor = np.where(lower != 0, 8.0 * ULP * math.pi / (θ_hi - θ_lo) + 8.0 * ULP, np.nan)
    return {f: factor * (np.abs(sky.values[f][lower]) + np.abs(sky.values[f][upper])) for f in sky.values.dtype.names}


def assert_fill(sky, θ_grid, got, got_cells, ref, ref_cells, label=""):
    """`got` (a structured array [θ, ϕ], or [θ, ϕ, 6] doubles) against the host route's `ref`: the cells exactly, the values
    within fill_bounds, NaN where the reference is"""
    for a, b in zip(got_cells, ref_cells):
        np.testing.assert_array_equal(a, b)
    bounds = fill_bounds(sky, θ_grid, *ref_cells)
    worst = 0.0
    for q, f in enumerate(ref.dtype.names):
        a, b = (got[f] if got.dtype.names else got[..., q]), ref[f]
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        ok = ~np.isnan(b)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.abs(a[ok] - b[ok]) / bounds[f][ok]
        ratio = ratio[np.isfinite(ratio)]
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        assert np.all(np.abs(a[ok] - b[ok]) <= bounds[f][ok]), (f, label)
    print(f"{label}: worst |difference| / bound over the six fields {worst:.3e}")


def single_cell_column(sky):
    """(ϕ grid of 3, θ grid of 5): θ inside ONE coarse leaf of the column ϕ[0], while the column ϕ[1] meets at least two cells over
    the same θ -- and ϕ[2] = -π meets none.  Found on the sky's host arrays."""
    g = sky.grid
    leaves = g.leaves()
    for side in (0, 2):                    # the neighbours in ϕ
        beside = g.neighbours[leaves, side]
        refined = (beside != 0) & (g.children[beside, 0] != 0) & (g.level[beside] == g.level[leaves])
        for c, nb in zip(leaves[refined][:50], beside[refined][:50]):
            (x, y), (wx, wy) = g.pos[c], g.get_cell_width(c)
            θ = np.arccos(np.linspace(x + 0.4 * wx, x - 0.4 * wx, 5))
            ϕ_b = float(g.pos[nb, 1])
            held = {g.get_parent_index(v, ϕ_b) for v in np.cos(θ)} - {0}
            if len(held) >= 2 and {g.get_parent_index(v, y) for v in np.cos(θ)} == {int(c)}:
                return np.array([y, ϕ_b, -math.pi]), θ
    raise AssertionError("no leaf beside a refined cell of its level: the scene has changed")
