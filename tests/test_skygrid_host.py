"""gr_skygrid.hpp -- the tree logic the k_sky_* kernels of a resident adaptive sky run per cell -- compiled for the host
(tests/harness_skygrid.py), against grids.py / adaptive.py on the analytic flat-space sky of tests/test_adaptive_sky_host.py
after trace_initial and two trace_steps (36 045 cells).  Index decisions are compared as arrays and bytes: they have to be
the ones numpy makes."""
import math

import numpy as np
import pytest

import harness_skygrid as H
from test_adaptive_sky_host import analytic_rows

FIELDS = ("pos", "level", "children", "neighbours", "parent", "location")


@pytest.fixture(scope="module")
def G():
    import gradus_jl_amd

    return gradus_jl_amd


@pytest.fixture(scope="module")
def scene(G):
    """(sky, its pair list): computed once, left unchanged"""
    sky = G.AdaptiveSky(analytic_rows, G.check_refine)
    G.trace_initial(sky, level=3)
    G.trace_step(sky)
    G.trace_step(sky)
    assert len(sky.grid) == 36045
    return sky, sky.grid.bordering_pairs()


def menu(G):
    """the criteria the drivers use"""
    return {
        "default 2 %": G.check_refine,
        "default 10 %": G.fine_refine_function(G.RadialBox(-math.inf, math.inf, open=False), percentage=10),
        "refine_function box": G.refine_function(G.RadialBox(15.0, 40.0)),
        "fine, open r bound": G.fine_refine_function(G.RadialBox(20.0, math.inf, open=(True, False)), percentage=10),
        "closed box, wrapped ϕ": G.fine_refine_function([G.RadialBox(5.0, 30.0, ϕ=[(0.0, 0.7), (5.6, 2 * math.pi)], open=False),
                                                         G.RadialBox(2.0, 4.0, ϕ=(1.0, 2.5), open=False)], percentage=10),
        "refine_to_level(4)": G.refine_to_level(4),      # (names nothing on this sky: every cell that hits is at level 4 by now)
        "refine_to_level(5)": G.refine_to_level(5),
    }


def assert_same_grid(h, grid):
    assert h.n == grid.n
    got = h.arrays()
    for f in FIELDS:
        want = getattr(grid, f)[:grid.n + 1]
        assert got[f].dtype == want.dtype and got[f].tobytes() == want.tobytes(), f


def test_the_pair_list_equals_bordering_pairs(G, scene):
    sky, (i1, i2) = scene
    a, b = H.pairs(H.Grid(sky.grid))
    assert a.size == i1.size > 100_000
    np.testing.assert_array_equal(a, i1)
    np.testing.assert_array_equal(b, i2)


def test_find_need_refine_under_every_criterion_equals_the_python_route(G, scene):
    sky, _ = scene
    h = H.Grid(sky.grid)
    for name, criterion in menu(G).items():
        want = G.find_need_refine(sky, criterion)
        cr = G.adaptive.gr_criterion_of(criterion)
        assert cr is not None, name
        got = H.find_need_refine(h, sky.values, cr)
        assert want.size > 0 or name == "refine_to_level(4)", name
        np.testing.assert_array_equal(got, want, err_msg=name)
    # the default criterion written as a fine criterion over the whole plane names the rows that hit only: a subset
    assert set(G.find_need_refine(sky, menu(G)["default 10 %"])) <= set(G.find_need_refine(sky, lambda s, a, b: G.check_refine(s, a, b, percentage=10)))


def test_the_default_criterion_at_ten_per_cent(G, scene):
    """check_refine(percentage = 10) itself: the same struct with another rtol"""
    sky, _ = scene
    cr = G.adaptive.gr_criterion_of(G.check_refine)
    cr.rtol = 10 / 100
    want = G.find_need_refine(sky, lambda s, a, b: G.check_refine(s, a, b, percentage=10))
    np.testing.assert_array_equal(H.find_need_refine(H.Grid(sky.grid), sky.values, cr), want)
    assert 0 < want.size < G.find_need_refine(sky).size


def test_a_radial_box_is_a_predicate_over_rows(G):
    v = np.zeros(6, dtype=G.adaptive.SKY_DTYPE)
    v["r"] = [1.0, 2.0, 3.0, np.nan, 2.0, 2.0]
    v["ϕ"] = [0.0, 0.0, 0.0, 0.0, -0.5, 7.0]
    assert list(G.RadialBox(1.0, 3.0)(v)) == [False, True, False, False, True, True]
    assert list(G.RadialBox(1.0, 3.0, open=False)(v)) == [True, True, True, False, True, True]
    assert list(G.RadialBox(1.0, 3.0, open=(False, True))(v)) == [True, True, False, False, True, True]
    # ϕ is folded into [0, 2π): -0.5 -> 5.78, 7 -> 0.72
    assert list(G.RadialBox(0.0, 9.0, ϕ=(0.5, 1.0))(v)) == [False, False, False, False, False, True]
    assert list(G.RadialBox(0.0, 9.0, ϕ=[(0.0, 0.1), (5.5, 6.0)])(v)) == [True, True, True, False, True, False]


def test_refining_the_list_leaves_all_six_arrays_equal_as_bytes(G, scene):
    sky, _ = scene
    need = G.find_need_refine(sky)
    h = H.Grid(sky.grid)
    rows = np.zeros((sky.grid.n + 1 + 9 * need.size, 6))
    rows[:sky.grid.n + 1] = sky.values.view(np.float64).reshape(-1, 6)
    assert H.refine(h, need, rows) == 0
    import copy

    grid = copy.deepcopy(sky.grid)
    kids = grid.refine_many(need)
    assert_same_grid(h, grid)
    # the middle child carries its parent's row
    assert rows[kids[:, 4]].tobytes() == rows[need].tobytes()
    # ... and the walk on the refined tree is still the reference's
    a, b = H.pairs(h)
    i1, i2 = grid.bordering_pairs()
    np.testing.assert_array_equal(a, i1)
    np.testing.assert_array_equal(b, i2)


@pytest.mark.parametrize("periodic", [True, False])
def test_the_nine_cell_grid_and_a_few_refinements(G, periodic):
    grid = G.AdaptiveGrid(-1.0, 2.0, 0.5, -0.25, x_periodic=periodic)
    h = H.Grid(limits=grid.limits, x_periodic=periodic)
    assert_same_grid(h, grid)
    a, b = H.pairs(h)
    i1, i2 = grid.bordering_pairs()
    assert a.size == (30 if periodic else 24)
    np.testing.assert_array_equal(a, i1)
    np.testing.assert_array_equal(b, i2)
    for cells in ([1, 5, 9], [10, 14, 36, 2], [40, 37, 7, 3], [66, 67, 4, 6, 8]):
        grid.refine_many(cells)
        assert H.refine(h, cells) == 0
        assert_same_grid(h, grid)
        a, b = H.pairs(h)
        i1, i2 = grid.bordering_pairs()
        np.testing.assert_array_equal(a, i1)
        np.testing.assert_array_equal(b, i2)


def test_refusals_leave_the_grid_as_it_was(G):
    grid = G.AdaptiveGrid(0.0, 1.0, 0.0, 1.0)
    grid.refine_many([3])
    h = H.Grid(grid, room=40)
    before = {f: a.tobytes() for f, a in h.arrays().items()}
    for cells, code in (([2, 2], 4), ([3], 2), ([0], 1), ([19], 1), ([4, 3], 2), ([-1], 1)):
        assert H.refine(h, cells) == code
        assert h.n == 18 and {f: a.tobytes() for f, a in h.arrays().items()} == before
    with pytest.raises(ValueError):
        grid.refine_many([2, 2])
    # the deepest level: a cell at GR_SKY_MAX_LEVEL is refused, never truncated
    deep = G.AdaptiveGrid(0.0, 1.0, 0.0, 1.0)
    cell = 5
    for _ in range(H.lib().hsg_max_level() - 1):
        cell = int(deep.refine_many([cell])[0, 4])
    d = H.Grid(deep, room=9)
    assert deep.level[cell] == H.lib().hsg_max_level() and H.refine(d, [cell]) == 3 and d.n == deep.n
    a, b = H.pairs(d)
    i1, i2 = deep.bordering_pairs()
    np.testing.assert_array_equal(a, i1)
    np.testing.assert_array_equal(b, i2)


def test_get_parent_index_on_boundaries_and_outside(G, scene):
    sky, _ = scene
    g = sky.grid
    rng = np.random.default_rng(5)
    (x1, x2), (y1, y2) = g.limits
    x = rng.uniform(x1 - 0.05, x2 + 0.05, 300)
    y = rng.uniform(y1 - 0.1, y2 + 0.1, 300)
    # points ON cell boundaries: corners and edge mid-points of cells of every level, and the domain's own edge
    cells = rng.choice(np.arange(1, g.n + 1), 60, replace=False)
    wx, wy = g.get_cell_width(cells)
    bx = np.concatenate([g.pos[cells, 0] + wx / 2, g.pos[cells, 0] - wx / 2, g.pos[cells, 0], g.pos[cells, 0] + wx / 6, [x1, x2, 0.0]])
    by = np.concatenate([g.pos[cells, 1] + wy / 2, g.pos[cells, 1], g.pos[cells, 1] - wy / 2, g.pos[cells, 1] - wy / 6, [0.0, 0.0, y2]])
    x, y = np.concatenate([x, bx, [np.nan]]), np.concatenate([y, by, [0.0]])
    want = np.array([g.get_parent_index(a, b) for a, b in zip(x, y)])
    got = H.parent_index(H.Grid(g), x, y)
    np.testing.assert_array_equal(got, want)
    assert np.count_nonzero(want == 0) > 10 and np.count_nonzero(want) > 300


def test_the_bins_equal_binned_cells(G, scene):
    sky, _ = scene
    r_bins, ϕ_bins = np.geomspace(1.3, 60.0, 50), np.linspace(0.0, 2 * math.pi, 50)
    v, _, r_i, ϕ_i = G.adaptive._binned_cells(sky, r_bins, ϕ_bins)
    for Γ in (2, None):
        leaf, ri, pi, counts = H.bins(H.Grid(sky.grid), sky.values, r_bins, ϕ_bins, Γ=Γ)
        assert leaf.size == r_i.size > 5000
        assert sky.values[leaf].tobytes() == v.tobytes()
        np.testing.assert_array_equal(ri, r_i)
        np.testing.assert_array_equal(pi, ϕ_i)
        # the census is where the emissivity map is non-zero
        m, d = G.KerrMetric(1.0, 0.998), G.ThinDisc(0.0, math.inf)
        lit = G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, sky, Γ=Γ) != 0
        np.testing.assert_array_equal(counts != 0, lit)
        assert counts.sum() == leaf.size and 0 < lit.sum() < lit.size
