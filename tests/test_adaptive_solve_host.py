"""The drivers of adaptive tracing (gradus.jl_amd/adaptive.py: empty_fraction, evaluate_refinement_metric, step_block,
adaptive_solve) on the analytic flat-space sky of tests/test_adaptive_sky_host.py, without a GPU, against a scalar,
loop-by-loop restatement of src/corona/adaptive-sample.jl:486-842 written here -- 1-based inclusive ranges, one pair at a
time, as `brute_force_need_refine` restates find_need_refine there."""
import copy
import math

import numpy as np
import pytest

from test_adaptive_sky_host import analytic_rows, brute_force_need_refine, scalar_isapprox

TWO_PI = 2 * math.pi


@pytest.fixture(scope="module")
def G():
    import gradus_jl_amd

    return gradus_jl_amd


@pytest.fixture(scope="module")
def scene(G):
    """(m, d, the sky after trace_initial, two plain steps, the far pass and the inner pass): computed once, only ever copied"""
    m, d = G.KerrMetric(1.0, 0.998), G.ThinDisc(0.0, math.inf)
    sky = G.AdaptiveSky(analytic_rows, G.check_refine)
    G.trace_initial(sky)
    G.trace_step(sky)
    G.trace_step(sky)
    assert len(sky.grid) == 36045
    G.trace_step(sky, G.fine_refine_function(G.RadialBox(800.0, math.inf, open=(True, False)), percentage=10))
    G.trace_step(sky, G.fine_refine_function(G.RadialBox(m.isco(), 2.0), percentage=20))
    return m, d, sky


# ---- the restatement ----

def pairs_that(sky, pred):
    """find_need_refine (adaptive-sky.jl:130-152): the sorted bordering cells of the pairs `pred(cell, other)` names"""
    found = set()
    for cell in range(1, len(sky.grid) + 1):
        if sky.grid.has_children(cell):
            continue
        for other in sky.grid.get_bordering(cell):
            if pred(cell, other):
                found.add(other)
    return sorted(found)


def default_criterion(v, a, b, percentage):
    """check_refine (adaptive-sample.jl:123-140)"""
    if math.isnan(v["r"][a]) and math.isnan(v["r"][b]):
        return False
    return (not scalar_isapprox(v["g"][a], v["g"][b], percentage / 100)) or (not scalar_isapprox(v["J"][a], v["J"][b], percentage / 100))


def is_in(limits, domain, x):
    """_is_in(al::AxisLimits, domain, x), limits = ((first, last), (first, last) or None) with 1-based inclusive ranges"""
    (a, b), second = limits
    inside = domain[a - 1] <= x <= domain[b - 1]
    if second is not None and second[1] >= second[0]:
        inside = (domain[second[0] - 1] <= x <= domain[second[1] - 1]) or inside
    return inside


def scalar_metric(output, N, split):
    """evaluate_refinement_metric with empty_fraction: [(r limits, ϕ limits, score)] in the reference's order"""
    stencil = N // split
    half = stencil // 2
    axis = list(range(1, N - stencil + 1, stencil // 4))          # 1:(stencil ÷ 4):(N - stencil)

    def evaluate(i, j):
        r = ((i, i + stencil), None)
        ϕ = ((1, half), (N - half, N)) if j == 0 else ((j, j + stencil), None)
        rows = list(range(r[0][0], r[0][1] + 1))
        cols = list(range(ϕ[0][0], ϕ[0][1] + 1)) + ([] if ϕ[1] is None else list(range(ϕ[1][0], ϕ[1][1] + 1)))
        filled = total = 0
        for a in rows:
            for b in cols:
                total += 1
                filled += 1 if output[a - 1, b - 1] != 0 else 0
        return r, ϕ, filled / total

    wrapped = [evaluate(i, 0) for i in axis]
    matrix = {(i, j): evaluate(i, j) for i in axis for j in axis}
    return wrapped + [matrix[i, j] for j in axis for i in axis]          # vec() of a matrix: the first index runs fastest


def scalar_step_block(G, m, d, sky, N=500, top=3, split=6, threshold=0.2, percentage=10, limit=200_000):
    """step_block! (adaptive-sample.jl:603-665); returns (code name, the cells it names)"""
    r_bins, ϕ_bins = np.geomspace(m.isco(), 1000.0, N), np.linspace(0.0, TWO_PI, N)
    counts = scalar_metric(G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, sky), N, split)
    counts = [c for c in counts if c[2] != 0]
    ordered = []                                                         # a stable insertion sort by score
    for c in counts:
        k = len(ordered)
        while k > 0 and ordered[k - 1][2] > c[2]:
            k -= 1
        ordered.insert(k, c)
    ordered = [c for c in ordered if c[2] < threshold]
    if not ordered:
        return "converged", []
    lims = ordered[:top]
    v = sky.values

    def in_a_block(cell):
        if math.isnan(v["r"][cell]):
            return False
        for r, ϕ, _ in lims:
            if is_in(r, r_bins, v["r"][cell]) and is_in(ϕ, ϕ_bins, v["ϕ"][cell] % TWO_PI):
                return True
        return False

    cells = pairs_that(sky, lambda a, b: default_criterion(v, a, b, percentage) and (in_a_block(a) or in_a_block(b)))
    if len(cells) > limit:
        return "limit_exceeded", cells
    G.refine_and_trace(sky, cells)
    return "not_converged", cells


def same_sky(a, b):
    ga, gb = a.grid, b.grid
    assert ga.n == gb.n and a.n_values == b.n_values
    for f in ("pos", "level", "children", "neighbours", "parent", "location"):
        assert getattr(ga, f)[:ga.n + 1].tobytes() == getattr(gb, f)[:gb.n + 1].tobytes(), f
    assert a.values.tobytes() == b.values.tobytes()


# ---- the tests ----

def test_empty_fraction_is_the_filled_fraction(G):
    block = np.array([[0.0, 1.0, -0.0], [2.0, np.nan, 0.0]])
    assert G.empty_fraction(None, None, block) == 3 / 6
    assert G.empty_fraction(None, None, np.zeros((3, 3))) == 0.0 and G.empty_fraction(None, None, np.ones((2, 5), dtype=np.int64)) == 1.0


def test_axis_limits_are_the_references_ranges(G):
    al = G.AxisLimits((3, 5))
    assert list(al.as_index()) == [2, 3, 4] and al.intervals(np.arange(10.0)) == [(2.0, 4.0)]
    wrapped = G.AxisLimits((1, 2), (8, 10))
    assert list(wrapped.as_index()) == [0, 1, 7, 8, 9] and wrapped.intervals(np.arange(10.0)) == [(0.0, 1.0), (7.0, 9.0)]
    assert [c.name for c in G.StepBlockCodes] == ["converged", "not_converged", "limit_exceeded"]


@pytest.mark.parametrize("N, split", [(100, 5), (60, 6), (47, 5)])
def test_evaluate_refinement_metric_equals_the_loops(G, scene, N, split):
    m, d, sky = scene
    r_bins, ϕ_bins = np.geomspace(m.isco(), 1000.0, N), np.linspace(0.0, TWO_PI, N)
    got = G.evaluate_refinement_metric(m, d, sky, r_bins, ϕ_bins, split=split)
    want = scalar_metric(G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, sky), N, split)
    assert len(got) == len(want) > 0
    for (r, ϕ, score), (wr, wϕ, wscore) in zip(got, want):
        assert (r.l1, r.l2) == wr and (ϕ.l1, ϕ.l2) == wϕ and score == wscore
    assert len({c[2] for c in want}) > 3 and all(0.0 <= c[2] <= 1.0 for c in want)
    # a metric of the caller's own is given the ranges and the block
    seen = G.evaluate_refinement_metric(m, d, sky, r_bins, ϕ_bins, split=split, metric=lambda r, ϕ, block: block.shape)
    stencil = N // split
    assert seen[0][2] == (stencil + 1, 2 * (stencil // 2) + 1) and seen[-1][2] == (stencil + 1, stencil + 1)


def test_step_block_equals_the_loops_until_it_converges(G, scene):
    m, d, base = scene
    ours, theirs = copy.deepcopy(base), copy.deepcopy(base)
    kw = dict(N=100, split=5, top=4)
    # a limit below the first step's list: the code says so and the sky stays as it was
    code, cells = scalar_step_block(G, m, d, theirs, limit=1000, **kw)
    assert G.step_block(m, d, ours, limit=1000, **kw).name == code
    same_sky(ours, base)
    outcomes = [(code, len(cells))]
    for _ in range(8):
        code, cells = scalar_step_block(G, m, d, theirs, **kw)
        assert G.step_block(m, d, ours, **kw).name == code
        same_sky(ours, theirs)
        outcomes.append((code, len(cells)))
        if code != "not_converged":
            break
    print("step_block, N = 100:", outcomes)
    names = [c for c, _ in outcomes]
    assert names[-1] == "converged" and "not_converged" in names and names[0] == "limit_exceeded"
    # fewer, larger bins are covered at once
    assert G.step_block(m, d, ours, N=60, split=5, top=4).name == scalar_step_block(G, m, d, theirs, N=60, split=5, top=4)[0]
    same_sky(ours, theirs)
    # check_threshold = False: the lowest-scoring blocks whatever their score
    code = G.step_block(m, d, ours, check_threshold=False, N=60, split=5, top=2)
    assert code is G.StepBlockCodes.not_converged and len(ours.grid) >= len(theirs.grid)


def scalar_adaptive_solve(G, m, d, sky, limit, trace_calls, **kw):
    """adaptive_solve! (adaptive-sample.jl:745-842)"""
    i = 0
    G.trace_initial(sky)
    G.refine_and_trace(sky, brute_force_need_refine(sky))
    i += 1
    for _ in range(trace_calls):
        G.refine_and_trace(sky, brute_force_need_refine(sky))
        i += 1
    v = lambda: sky.values
    far = lambda c: v()["r"][c] > 800
    G.refine_and_trace(sky, pairs_that(sky, lambda a, b: default_criterion(v(), a, b, 10) and (far(a) or far(b))))
    i += 1
    r_isco = m.isco()
    inner = lambda c: v()["r"][c] > r_isco and v()["r"][c] < 2.0
    G.refine_and_trace(sky, pairs_that(sky, lambda a, b: default_criterion(v(), a, b, 20) and (inner(a) or inner(b))))
    i += 1
    status = "not_converged"
    while status == "not_converged":
        status, _ = scalar_step_block(G, m, d, sky, split=5, top=4, **kw)
        i += 1
        if i >= limit:
            break
    for n in (4, 5):
        both_miss = lambda a, b: math.isnan(v()["r"][a]) and math.isnan(v()["r"][b])
        G.refine_and_trace(sky, pairs_that(sky, lambda a, b: not both_miss(a, b) and sky.grid.level[b] < n))
        i += 1
    return i


def test_adaptive_solve_equals_the_loops(G, scene):
    m, d, _ = scene
    ours, theirs = G.AdaptiveSky(analytic_rows, G.check_refine), G.AdaptiveSky(analytic_rows, G.check_refine)
    n_theirs = scalar_adaptive_solve(G, m, d, theirs, limit=6, trace_calls=1, N=100)
    n_ours = G.adaptive_solve(m, d, ours, limit=6, trace_calls=1, N=100, verbose=False)
    assert n_ours == n_theirs and 7 <= n_ours <= 8
    same_sky(ours, theirs)
    assert int(ours.grid.level[1:ours.grid.n + 1].max()) >= 5
    print(f"adaptive_solve: {n_ours} iterations, {len(ours.grid)} cells")
