"""The adaptive image plane on the host: the pair criterion and the filled image of gr_planegrid.hpp (what the k_plane_* kernels
run, compiled with g++: tests/host_harness_planegrid.cpp) against adaptive.py (check_refine_plane, fill_sky_values) on trees traced
by the CPU oracle through the generic form of AdaptiveSky, and the growth of a sky whose rows are GeodesicPoints."""
import math

import numpy as np
import pytest

import harness_planegrid as H
import plane_scene as S


@pytest.fixture(scope="module")
def plane_b(G, oracle):
    """scene B after trace_initial and two trace_steps; only ever read"""
    return S.oracle_plane(G, oracle, "B", steps=2)


@pytest.fixture(scope="module")
def plane_a(G, oracle):
    return S.oracle_plane(G, oracle, "A", steps=1)


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- 1. the criterion ----

def test_the_prototype_counts(G, oracle):
    for scene in ("A", "B"):
        sky = S.oracle_plane(G, oracle, scene)
        assert len(sky.grid) == 819 and sky.values.dtype == G.POINT_DTYPE
        for expected in S.REFINED[scene][:2]:
            assert G.find_need_refine(sky).size == expected
            G.trace_step(sky)
        if scene == "B":
            assert sky.grid.leaves().size == 4753


@pytest.mark.parametrize("percentage", [20, 5])
def test_the_header_decides_every_pair_as_check_refine_plane(G, plane_b, percentage):
    i1, i2 = plane_b.grid.bordering_pairs()
    assert i1.size > 10_000
    # a condition of the comparison: an ulp between numpy's and glibc's log10 cannot flip a decision
    margin = S.threshold_margin(plane_b, i1, i2, percentage)
    assert margin.size > 1000 and margin.min() > 1e-9, margin.min()
    ours = G.check_refine_plane(plane_b, i1, i2, percentage=percentage)
    theirs = H.need_refine(H.Plane(plane_b), i1, i2, percentage=percentage)
    np.testing.assert_array_equal(theirs, ours)
    np.testing.assert_array_equal(G.refine_plane(percentage)(plane_b, i1, i2), ours)
    assert 0 < ours.sum() < ours.size
    if percentage == 20:
        assert np.unique(i2[ours]).size == S.REFINED["B"][2]


def test_the_level_criterion_on_a_plane(G, plane_b):
    i1, i2 = plane_b.grid.bordering_pairs()
    ours = G.refine_to_level(5)(plane_b, i1, i2)
    np.testing.assert_array_equal(H.need_refine(H.Plane(plane_b), i1, i2, kind=H.CRIT_LEVEL, level=5), ours)
    status = plane_b.values["status"]
    assert not ours[(status[i1] != 2) & (status[i2] != 2)].any() and 0 < ours.sum() < ours.size


def test_the_criterion_on_synthetic_rows(G, plane_b):
    rows = G.adaptive.make_null(8, G.POINT_DTYPE)
    assert (rows["status"] == 3).all() and np.isnan(rows["x"]).all() and (rows["flags"] == 0).all()
    hit = lambda r, θ: (2, [0.0, r, θ, 0.3])
    spec = [(0, [0.0, 5.0, 1.0, 0.0]), (1, [0.0, 1.2, 0.5, 0.0]),            # 0, 1: misses (out of domain, inner boundary)
            hit(10.0, 1.5), hit(10.0, 1.5),                                   # 2, 3: equal rows
            hit(math.nan, 1.5),                                               # 4: NaN radius
            hit(10.0, 1.5 - 2 * math.pi), hit(10.0, 1.5 + 2 * math.pi),       # 5, 6: θ negative, θ above 2π
            hit(40.0, 1.5)]                                                   # 7: another radius
    for k, (status, x) in enumerate(spec):
        rows["status"][k], rows["x"][k] = status, x

    class Rows:
        values = rows

    i1, i2 = (a.ravel() for a in np.meshgrid(np.arange(8), np.arange(8), indexing="ij"))
    ours = G.check_refine_plane(Rows, i1, i2)
    p = H.Plane(plane_b)
    np.testing.assert_array_equal(H.need_refine(p, i1, i2, points=rows), ours)
    table = ours.reshape(8, 8)
    assert not table[:2, :2].any()                       # both miss
    assert table[:2, 2:].all() and table[2:, :2].all()   # exactly one hits
    assert not table[2, 3] and not table[2, 2]           # equal rows
    assert table[4, 2] and table[2, 4] and table[4, 4]   # NaN is never approximately anything
    assert not table[2, 5] and not table[2, 6] and not table[5, 6]       # θ is folded into [0, 2π) ...
    assert abs(np.mod(1.5 - 2 * math.pi, 2 * math.pi) - 1.5) < 1e-15
    assert table[2, 7]                                   # log10 40 against log10 10


# ---- 2. the filled image ----

def grids_for(sky, n_x, n_y):
    (x1, x2), (y1, y2) = sky.grid.limits
    leaves = sky.grid.leaves()
    centres = np.unique(sky.grid.pos[leaves, 0])
    pick = centres[np.linspace(0, centres.size - 1, max(n_x - 4, 1)).astype(int)]
    wx = sky.grid.get_cell_width(leaves)[0].min()
    # left and right of cell centres, the centres themselves, and the outermost cells from both sides (neighbour 0)
    x = np.concatenate([pick - wx / 4, pick + wx / 4, pick, [x1 + wx / 8, x2 - wx / 8, x1, x2]])
    return np.sort(x), np.linspace(y1, y2, n_y)


def assert_fill_agrees(G, sky, x_grid, y_grid, pf=None, val=None):
    out, (lower, upper) = G.fill_sky_values(sky, (x_grid, y_grid), pf=pf, cells=True)
    val = G.adaptive._plane_cell_values(sky, pf, None) if val is None else val
    h_out, h_lower, h_upper, counts = H.fill(H.Plane(sky), val, x_grid, y_grid)
    assert out.shape == (len(y_grid), len(x_grid))
    assert same_bytes(out, h_out)
    np.testing.assert_array_equal(lower, h_lower)
    np.testing.assert_array_equal(upper, h_upper)
    assert same_bytes(out, G.fill_sky_values(sky, (x_grid, y_grid), pf=pf))
    return out, lower, upper, counts


def test_fill_header_and_numpy_give_the_same_bytes(G, plane_b):
    x_grid, y_grid = grids_for(plane_b, 16, 33)
    out, lower, upper, counts = assert_fill_agrees(G, plane_b, x_grid, y_grid)
    assert (counts[1:-1] >= 2).all() and counts[0] == counts[-1] == 0        # x on the domain's edge lies in no cell
    assert np.isnan(out[:, 0]).all() and np.isfinite(out[:, 1:-1]).all()
    assert (lower[:, 1:-1] > 0).all() and (lower[:, 0] == 0).all()
    # the two cells of a point are consecutive cells of its column, ascending in β
    pos_y = plane_b.grid.pos[:, 1]
    assert (pos_y[lower[:, 1:-1]] < pos_y[upper[:, 1:-1]]).all()
    # a value array of the caller's, with NaN on the cells that miss
    val = np.where(plane_b.values["status"] == 2, plane_b.values["x"][:, 1], np.nan)
    out, lower, upper, _ = assert_fill_agrees(G, plane_b, x_grid, y_grid, pf=val, val=val)
    hit = plane_b.values["status"] == 2
    np.testing.assert_array_equal(np.isnan(out[:, 1:-1]), ~(hit[lower] & hit[upper])[:, 1:-1])


def test_fill_descending_and_non_square(G, plane_b):
    x_grid, y_grid = grids_for(plane_b, 7, 9)
    up = G.fill_sky_values(plane_b, (x_grid, y_grid))
    down, _, _, _ = assert_fill_agrees(G, plane_b, x_grid, y_grid[::-1].copy())
    assert same_bytes(down, up[::-1])
    shuffled = np.random.default_rng(5).permutation(y_grid.size)
    assert same_bytes(G.fill_sky_values(plane_b, (x_grid, y_grid[shuffled])), up[shuffled])
    x5, y7 = np.linspace(-50.0, 55.0, 5), np.linspace(-30.0, 33.0, 7)
    out, _, _, _ = assert_fill_agrees(G, plane_b, x5, y7)
    assert out.shape == (7, 5) and np.isfinite(out).all()
    # out[β index, α index]: one column and one row of it are what the 1-wide grids give
    assert same_bytes(G.fill_sky_values(plane_b, (x5[3:4], y7))[:, 0], out[:, 3])
    # the call shape with N
    α, β, image = G.fill_sky_values(plane_b, 6, metric=S.metric(G))
    np.testing.assert_array_equal(α, np.linspace(-60.0, 60.0, 6))
    np.testing.assert_array_equal(β, np.linspace(-35.0, 35.0, 6))
    assert same_bytes(image, G.fill_sky_values(plane_b, (α, β)))


def test_fill_of_nine_cells(G, oracle):
    sky = S.oracle_plane(G, oracle, "A", level=1)
    assert len(sky.grid) == 9
    x_grid = np.array([-11.0, -8.0, -5.0, 0.5, 7.9, 8.0, 11.5])
    # three cells per column: the points beyond the outer centres extrapolate from the clamped interval
    out, lower, upper, counts = assert_fill_agrees(G, sky, x_grid, np.linspace(-11.9, 11.9, 11))
    assert (counts == 3).all() and np.isfinite(out).all()
    assert set(np.unique(upper - lower)) == {1}
    # a β grid over two of the three rows: a column of two cells, every point clamped to their interval
    out, lower, upper, counts = assert_fill_agrees(G, sky, x_grid, np.linspace(-11.0, 3.0, 6))
    assert (counts == 2).all() and np.isfinite(out).all()
    assert (lower == lower[0]).all() and (upper == upper[0]).all()
    # a β grid inside one row: one cell per column, NaN (the reference indexes out of bounds)
    out, lower, upper, counts = assert_fill_agrees(G, sky, x_grid, np.linspace(-3.0, 3.0, 5))
    assert (counts == 1).all() and np.isnan(out).all() and not lower.any() and not upper.any()


# ---- 3. the grid and the growth of a sky of points ----

REFERENCE_TOP_NEIGHBOURS = [(0, 4, 2, 7), (1, 5, 3, 8), (2, 6, 0, 9), (0, 7, 5, 1), (4, 8, 6, 2), (5, 9, 0, 3), (0, 1, 8, 4), (7, 2, 9, 5), (8, 3, 0, 6)]


def test_x_periodic_reproduces_the_reference_grid(G, oracle):
    wrapped = S.oracle_plane(G, oracle, "A", x_periodic=True, level=1)
    np.testing.assert_array_equal(wrapped.grid.neighbours[1:10], REFERENCE_TOP_NEIGHBOURS)
    np.testing.assert_array_equal(H.top_neighbours(S.LIMITS["A"], True)[1:], REFERENCE_TOP_NEIGHBOURS)
    plain = S.oracle_plane(G, oracle, "A", level=1)
    np.testing.assert_array_equal(plain.grid.neighbours[1:10], H.top_neighbours(S.LIMITS["A"], False)[1:])
    assert (plain.grid.neighbours[[1, 2, 3], 3] == 0).all() and (plain.grid.neighbours[[7, 8, 9], 1] == 0).all()
    # across the wrap there is nothing to interpolate with: the outermost columns take their cells' own values
    x_grid = np.array([-11.0, 11.0])
    out, _, _, _ = assert_fill_agrees(G, wrapped, x_grid, np.linspace(-11.0, 11.0, 7))
    assert same_bytes(out, G.fill_sky_values(plain, (x_grid, np.linspace(-11.0, 11.0, 7))))


def test_a_sky_of_points_grows(G, plane_b):
    assert plane_b.is_plane and plane_b.n_values == len(plane_b.grid) > 1024
    assert plane_b.values.dtype == G.POINT_DTYPE and plane_b.values.shape == (plane_b.n_values + 1,)
    null = plane_b.values[0]
    assert null["status"] == 3 and null["flags"] == 0 and np.isnan(null["x"]).all() and np.isnan(null["lambda_max"])
    assert same_bytes(plane_b.make_null(3), G.adaptive.make_null(3, G.POINT_DTYPE))
    # the corona's rows are what they were
    sky_null = G.adaptive.make_null(2)
    assert sky_null.dtype == G.adaptive.SKY_DTYPE and all(np.isnan(sky_null[f]).all() for f in G.adaptive.SKY_FIELDS)
    # the middle child's row is its parent's, whole
    refined = np.flatnonzero(plane_b.grid.children[:plane_b.grid.n + 1, 0])
    assert refined.size > 500
    middle = plane_b.grid.children[refined, 4]
    assert same_bytes(plane_b.values[middle], plane_b.values[refined])
    np.testing.assert_array_equal(plane_b.grid.pos[middle], plane_b.grid.pos[refined])


def test_corona_only_functions_refuse_a_plane(G, plane_b):
    m, bins = S.metric(G), np.linspace(1.0, 10.0, 5)
    for call in (lambda: G.bin_emissivity_grid(m, None, bins, bins, plane_b), lambda: G.bin_redshift_grid(bins, bins, plane_b),
                 lambda: G.bin_time_grid(bins, bins, plane_b), lambda: G.step_block(m, None, plane_b),
                 lambda: G.adaptive_solve(m, None, plane_b, verbose=False)):
        with pytest.raises(TypeError, match="AdaptivePlane"):
            call()


# ---- 4. point functions ----

def test_fill_with_point_functions(G, oracle, plane_a):
    cfg = S.oracle_config(G, oracle)
    x_grid, y_grid = np.linspace(-11.5, 11.5, 24), np.linspace(-11.5, 11.5, 20)
    hit = plane_a.values["status"] == 2
    # the default: the coordinate time of the end point, finite for every traced cell
    out, lower, upper, _ = assert_fill_agrees(G, plane_a, x_grid, y_grid)
    assert np.isfinite(out).all() and (lower > 0).all()
    np.testing.assert_array_equal(G.adaptive._plane_cell_values(plane_a, None, None)[1:], plane_a.values["x"][1:, 0])

    def redshift(points):
        return oracle.apply_pf(cfg, np.ascontiguousarray(points), S.T_MAX, pf_id=oracle.PF_REDSHIFT, filter_id=oracle.FILTER_INTERSECTED,
                               r_isco=S.metric(G).isco())

    val = redshift(plane_a.values)
    np.testing.assert_array_equal(np.isnan(val), ~hit)
    out, lower, upper, _ = assert_fill_agrees(G, plane_a, x_grid, y_grid, pf=redshift, val=val)
    # finite inside the disc's image; NaN spreads from a miss cell to every point interpolated with it, and no further (a
    # neighbour that misses is not interpolated with)
    np.testing.assert_array_equal(np.isnan(out), ~(hit[lower] & hit[upper]))
    inside = np.isfinite(out)
    assert inside.any() and not inside.all()             # the window holds the disc's image and the hole's shadow
    assert 0.05 < out[inside].min() and out[inside].max() < 2.0
