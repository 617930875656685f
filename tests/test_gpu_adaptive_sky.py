"""`AdaptiveSky(m, corona, d)` on the MI355X: the refinement loop of gradus.jl_amd/adaptive.py with every step's cells traced by
one `gr_sky_cells` launch.  The scene of the reference's adaptive-tracing walk-through: RingCorona r = 10, h = 4 over a Kerr
hole with a = 0.998 and ThinDisc(0, ∞)."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def fresh_rows(G, sky, cells):
    """gr_sky_cells of the centres of `cells` with the sky's own configuration"""
    tr = sky.tracer
    cosθ = np.ascontiguousarray(sky.grid.pos[cells, 0])
    ϕ = np.ascontiguousarray(sky.grid.pos[cells, 1])
    sc = G._lib.gr_skycells()
    for q in range(4):
        sc.x_src[q] = tr["x_src"][q]
    for q, val in enumerate(tr["Mx"].ravel()):
        sc.Mx[q] = val
    sc.cos_theta, sc.phi, sc.n = cosθ.ctypes.data, ϕ.ctypes.data, cosθ.size
    out = np.empty(cosθ.size, dtype=G.adaptive.SKY_DTYPE)
    G._lib.check(G._lib.load().gr_sky_cells(tr["ensemble"].ctx.handle, C.byref(tr["cfg"]), C.byref(sc), C.byref(tr["pf"]), out.ctypes.data, None))
    return out


def check_grid_invariants(sky):
    g = sky.grid
    assert sky.n_values == len(g) and sky.values.shape == (len(g) + 1,)
    parents = np.flatnonzero(g.has_children(np.arange(1, len(g) + 1))) + 1
    mid = g.children[parents, 4]
    assert sky.values[mid].tobytes() == sky.values[parents].tobytes()
    np.testing.assert_array_equal(g.pos[mid], g.pos[parents])
    # the leaves tile the domain: their areas add up to the extent's
    wx, wy = g.get_cell_width(g.leaves())
    Δx, Δy = g.extent()
    assert abs(np.sum(wx * wy) / (Δx * Δy) - 1.0) < 1e-12
    # every bordering cell of a leaf is a leaf
    for c in g.leaves()[::97]:
        assert not any(g.has_children(b) for b in g.get_bordering(int(c)))


@pytest.mark.parametrize("shape", [0, 1], ids=["lane", "pair"])
def test_the_walk_through_scene_refines_and_every_leaf_is_its_own_trace(G, ens, shape):
    # (one shape for every launch: by its size alone the library would give the small steps to the pairs and a launch of all the
    # leaves to single lanes, and the two shapes agree to 1e-11, not bit for bit)
    ens.set("tangent_pairs", shape)
    m, corona, d = G.KerrMetric(1.0, 0.998), G.RingCorona(r=10.0, h=4.0), G.ThinDisc(0.0, math.inf)
    sky = G.AdaptiveSky(m, corona, d, ensemble=ens)
    G.trace_initial(sky)
    assert len(sky.grid) == 819 and [n for n, _ in sky.tracer["launches"]] == [9, 72, 648]
    for step in range(2):
        need = G.find_need_refine(sky)
        launches = len(sky.tracer["launches"])
        before = len(sky.grid)
        G.trace_step(sky)
        assert need.size > 0 and len(sky.grid) == before + 9 * need.size
        assert [n for n, _ in sky.tracer["launches"][launches:]] == [8 * need.size]         # all the new cells in one launch
    check_grid_invariants(sky)
    leaves = sky.grid.leaves()
    assert sky.values[leaves].tobytes() == fresh_rows(G, sky, leaves).tobytes()
    v = sky.values[leaves]
    hit = v["status"] == 1.0
    assert hit.mean() > 0.3 and np.all(np.isnan(v["r"][~hit])) and np.all(np.isfinite(v["J"][hit]))
    assert set(np.unique(v["status"])) <= {1.0, -3.0, 7.0, 0.0}
    # the (r, ϕ) maps
    r_bins, ϕ_bins = np.geomspace(m.isco(), 200.0, 40), np.linspace(0.0, 2 * math.pi, 40)
    em = G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, sky)
    _, ΔΩ, r_i, ϕ_i = G.adaptive._binned_cells(sky, r_bins, ϕ_bins)
    solid = np.zeros_like(em)
    np.add.at(solid, (r_i, ϕ_i), ΔΩ)
    lit = solid > 0
    assert lit.sum() > 0.5 * em.size and np.all(np.isfinite(em)) and np.all(em[lit] > 0) and np.all(em[~lit] == 0)
    g_map, t_map = G.bin_redshift_grid(r_bins, ϕ_bins, sky), G.bin_time_grid(r_bins, ϕ_bins, sky)
    assert np.all(g_map[lit] > 0) and np.all(t_map[lit] > 0)
    ϕ_grid, θ_grid, dense = G.fill_sky_values(sky, 30)
    assert dense.shape == (30, 30)


def test_an_on_axis_source_has_J_equal_to_dr_dtheta_over_sin_theta(G, ens):
    """A lamp post on the axis: ϕ_disc = ϕ_sky + const, so ∂ϕ/∂ϕ_sky = 1, ∂r/∂ϕ_sky = 0 and J sin θ = |∂r/∂θ|, which central
    differences of the device's own r along a column of cells (one ϕ, neighbouring cos θ) give as sin θ |Δr / Δcos θ|.  A swapped
    or mis-signed column of the Jacobian is off by O(1).  Held at 1e-2 on the cells with 5 <= r <= 20: between the strongly lensed
    rays near the hole, where r(θ) bends on the scale of a cell, and the far field, where r grows like tan θ -- there the
    truncation error of the difference itself (measured on the host build at this cell size: 2.7e-3) stays below the bar.
    The source sits 1e-4 rad off the axis (the coordinates are singular on it): its lateral offset, 1e-3, moves J by 1e-3 / r."""
    m, d = G.KerrMetric(1.0, 0.998), G.ThinDisc(0.0, math.inf)
    sky = G.AdaptiveSky(m, G.LampPostModel(h=10.0, θ=1e-4), d, ensemble=ens)
    G.trace_initial(sky, level=4)
    leaves = sky.grid.leaves()
    assert leaves.size == 9 ** 4
    pos, v = sky.grid.pos[leaves], sky.values[leaves]
    order = np.lexsort((pos[:, 0], np.round(pos[:, 1], 9)))       # columns of one ϕ (to rounding), cos θ ascending
    c, r, J = (a[order].reshape(81, 81) for a in (pos[:, 0], v["r"], v["J"]))
    with np.errstate(invalid="ignore"):
        drdc = (r[:, 2:] - r[:, :-2]) / (c[:, 2:] - c[:, :-2])
        sinθ = np.sqrt(1.0 - c[:, 1:-1] ** 2)
        use = np.isfinite(drdc) & (r[:, 1:-1] >= 5.0) & (r[:, 1:-1] <= 20.0) & (r[:, 2:] <= 20.0) & (r[:, :-2] >= 5.0)
    assert use.sum() > 1000
    est, got = np.abs(drdc[use]) * sinθ[use], J[:, 1:-1][use] * sinθ[use]
    print(f"lamp post: {int(use.sum())} cells, max |est / J sin θ - 1| = {np.max(np.abs(est / got - 1.0)):.2e}")
    np.testing.assert_allclose(got, est, rtol=1e-2)
