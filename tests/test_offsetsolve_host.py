"""csrc/gr_offsetsolve.hpp -- the offset solve and the extremum search as per-problem state machines -- in its host build (no GPU),
against the lock-step route it restates: `find_offsets_for_radius_newton_ad` and `_golden_section_batch` of transfer_functions.py
on `harness.tangent_tracer`, the same host-compiled ray code.  That tracer does not speculate, so it traces on-path rays only and
the two routes must trace the SAME rays: offsets, redshifts, rows and ray counts are compared byte for byte."""
import math

import numpy as np
import pytest

import harness as Hh
import harness_offsetsolve as Ho


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def counted(trace):
    """`trace` with its `.tangent` wrapped: launches and rays of the lock-step route"""
    count = {"launches": 0, "rays": 0}
    inner = trace.tangent

    def tangent(α, β, heights=None):
        count["launches"] += 1
        count["rays"] += np.asarray(α).size
        return inner(α, β, heights)

    trace.tangent = tangent
    return count


def pair(G, a, angle, r_obs=1000.0, max_time=2000.0):
    """(metric, lock-step tracer, its counts, state-machine tracer) for Kerr `a` seen from `angle` degrees"""
    x = np.array([0.0, r_obs, math.radians(angle), 0.0])
    m, lock = Hh.tangent_tracer(G, a, x, max_time)
    return m, x, lock, counted(lock), Ho.tracer(G, m, x, max_time)


def both_routes(G, a, angle, rₑ, θ, heights=None):
    TF = G.transfer_functions
    m, x, lock, count, mine = pair(G, a, angle)
    ref = TF.find_offsets_for_radius_newton_ad(lock, rₑ, θ, r_min=m.inner_radius(), heights=heights)
    before = Ho.rays_traced()
    got = mine.solve(rₑ, θ, heights, r_min=m.inner_radius())
    return ref, got, count, Ho.rays_traced() - before


def assert_same_solve(ref, got, count, traced):
    r, pts, g, rows = ref
    r2, pts2, g2, rows2, n_rays = got
    assert same_bytes(r, r2)
    assert same_bytes(g, g2)
    assert same_bytes(rows, rows2)
    assert np.array_equal(pts["status"], pts2["status"]) and same_bytes(pts["x"], pts2["x"])
    # the rays the lock-step route traced, and never one after `done`
    assert int(n_rays.sum()) == count["rays"]
    assert traced == count["rays"]


def scene1():
    return np.repeat([1.3, 2.0, 4.0, 11.0, 40.0], 12), np.tile(np.linspace(-math.pi / 2, 3 * math.pi / 2, 12), 5)


def test_scene1_roots_rows_and_ray_counts_are_the_lockstep_ones(G):
    rₑ, θ = scene1()
    ref, got, count, traced = both_routes(G, 0.998, 60, rₑ, θ)
    assert (count["launches"], count["rays"]) == (79, 663)
    assert not np.isnan(ref[0]).any() and float(np.max(np.abs(ref[3][:, 1] - rₑ))) < 1e-7
    assert_same_solve(ref, got, count, traced)


def test_scene2_bracket_finish(G):
    rₑ, θ = np.repeat([1.25, 1.6, 3.0], 16), np.tile(np.linspace(-math.pi / 2, 3 * math.pi / 2, 16), 3)
    ref, got, count, traced = both_routes(G, 0.998, 85, rₑ, θ)
    assert (count["launches"], count["rays"]) == (86, 852)
    assert not np.isnan(ref[0]).any() and float(np.max(np.abs(ref[3][:, 1] - rₑ))) < 1e-7
    assert_same_solve(ref, got, count, traced)


def test_scene3_problems_without_an_offset(G):
    rₑ, θ = np.array([1.5, 1.5, 1.9, 5000.0, 6.0]), np.array([0.3, 2.0, 1.0, 0.5, 0.5])
    ref, got, count, traced = both_routes(G, 0.5, 60, rₑ, θ)
    assert count["rays"] == 137
    assert np.array_equal(np.isnan(ref[0]), [True, True, False, True, False])
    assert np.allclose(ref[0][[2, 4]], [4.14941526, 7.54065605], rtol=0, atol=1e-8)
    assert list(ref[1]["status"]) == [1, 1, 2, 3, 2]
    assert_same_solve(ref, got, count, traced)


def test_scene4_one_datum_plane_per_problem(G):
    rₑ, θ = scene1()
    ref, got, count, traced = both_routes(G, 0.998, 60, rₑ, θ, heights=0.05 * rₑ)
    assert not np.isnan(ref[0]).any()
    assert_same_solve(ref, got, count, traced)


@pytest.fixture(scope="module")
def transfer_pair(G):
    """cunningham_transfer_functions for rₑ = 2 and 11, N = 20, N_extrema = 5, by both routes, with their raw tables"""
    TF = G.transfer_functions
    m, x, lock, count, mine = pair(G, 0.998, 60)
    d = G.ThinDisc(0.0, float("inf"))
    raw_ref, raw_dev = [], []
    ref = TF.cunningham_transfer_functions(m, x, d, [2.0, 11.0], N=20, N_extrema=5, tracer=lock, root_finder="reference", _raw=raw_ref)
    before = Ho.rays_traced()
    dev = TF.cunningham_transfer_functions(m, x, d, [2.0, 11.0], N=20, N_extrema=5, tracer=mine, root_finder="device", _raw=raw_dev)
    return ref, raw_ref[0], dev, raw_dev[0], count, Ho.rays_traced() - before


def test_transfer_functions_match_the_lockstep_route(transfer_pair):
    ref, (data_r, gmin_r, gmax_r), dev, (data_d, gmin_d, gmax_d), count, traced = transfer_pair
    assert (count["launches"], count["rays"]) == (184, 675)
    assert traced == count["rays"]
    assert same_bytes(data_r[:, 0], data_d[:, 0])            # θ: exactly
    for row in (1, 2, 3):                                    # g, J, t
        np.testing.assert_allclose(data_d[:, row], data_r[:, row], rtol=1e-12, atol=0)
    np.testing.assert_allclose(gmin_d, gmin_r, rtol=1e-12, atol=0)
    np.testing.assert_allclose(gmax_d, gmax_r, rtol=1e-12, atol=0)
    for a, b in zip(ref, dev):
        assert a.g_star.size == b.g_star.size == 30 and a.rₑ == b.rₑ
        np.testing.assert_allclose([b.gmin, b.gmax], [a.gmin, a.gmax], rtol=1e-12, atol=0)


def test_failure_raises_the_lockstep_message(G):
    TF = G.transfer_functions
    m, x, lock, _, mine = pair(G, 0.998, 60)
    d = G.ThinDisc(0.0, float("inf"))
    kw = dict(N=20, N_extrema=5)
    with pytest.raises(RuntimeError) as ref:
        TF.cunningham_transfer_functions(m, x, d, [6.0, 5000.0], tracer=lock, root_finder="reference", **kw)
    with pytest.raises(RuntimeError) as dev:
        TF.cunningham_transfer_functions(m, x, d, [6.0, 5000.0], tracer=mine, root_finder="device", **kw)
    assert str(ref.value).startswith("Transfer function integration failed (rₑ=5000.0")
    assert str(dev.value) == str(ref.value)


def test_failure_inside_a_search_raises_the_lockstep_message(G):
    """a search whose first root solve has no acceptable offset (rₑ = 5000 seen from 1000) ends there with the failure flag on that
    record; its neighbours in the launch run to the end"""
    TF = G.transfer_functions
    m, x, lock, _, mine = pair(G, 0.998, 60)
    θ_offset, n_iter = 0.3, 4
    rr2 = np.array([6.0, 5000.0, 6.0, 5000.0])
    lower = np.array([-θ_offset, -θ_offset, math.pi - θ_offset, math.pi - θ_offset])
    upper = lower + 2 * θ_offset
    sign = np.array([1.0, 1.0, -1.0, -1.0])
    θ, r, rows, n_rays, bad, best = mine.search(rr2, lower, upper, sign, n_iter, r_min=m.inner_radius())
    assert np.array_equal(bad[:, 0], [False, True, False, True]) and not bad[:, 1:].any()
    assert np.isnan(best[[1, 3]]).all() and not np.isnan(best[[0, 2]]).any()
    # a failed search stops there: nothing recorded, nothing traced behind the failure
    assert np.isnan(θ[[1, 3], 1:]).all() and (n_rays[[1, 3], 1:] == 0).all()
    assert same_bytes(θ[:, 0], lower + TF.GOLDEN * (upper - lower))


def test_search_records_and_minimum(G):
    TF = G.transfer_functions
    m, x, lock, count, mine = pair(G, 0.998, 60)
    rr2, sign = np.array([2.0, 11.0, 2.0, 11.0]), np.array([1.0, 1.0, -1.0, -1.0])
    lower = np.array([-0.3, -0.3, math.pi - 0.3, math.pi - 0.3])
    upper = lower + 0.6
    n_iter = 4
    before = Ho.rays_traced()
    θ, r, rows, n_rays, bad, best = mine.search(rr2, lower, upper, sign, n_iter, r_min=m.inner_radius())
    assert Ho.rays_traced() - before == int(n_rays.sum())
    assert not bad.any() and θ.shape == (4, n_iter + 1)
    assert same_bytes(θ[:, 0], lower + TF.GOLDEN * (upper - lower))
    assert same_bytes(best, np.min(sign[:, None] * rows[:, :, 0], axis=1))

    # the lock-step search at depth 1 visits the same angles and finds the same minima
    seen = []

    def evaluate(idx, θ2):
        θ2 = np.array(θ2, dtype=np.float64)
        pole = (np.abs(θ2) < 1e-4) | (np.abs(np.abs(θ2) - math.pi) < 1e-4)
        θ2 = np.where(pole, θ2 + 1e-4, θ2)
        out = TF.find_offsets_for_radius_newton_ad(lock, rr2[idx], θ2, r_min=m.inner_radius())
        return θ2, out[2]

    def record(_, vals):
        seen.append(vals[0].copy())
        return sign * vals[1]

    ref_best = TF._golden_section_batch(evaluate, record, lower, upper, n_iter, depth=1)
    assert same_bytes(np.stack(seen, axis=1), θ)
    np.testing.assert_allclose(best, ref_best, rtol=1e-12, atol=0)
    assert int(n_rays.sum()) == count["rays"]


def test_pole_nudge(G):
    m, x, lock, _, mine = pair(G, 0.998, 60)
    # a bracket whose first golden-section point is θ = 0 to within 1e-4, and one about π
    g = G.transfer_functions.GOLDEN
    lower = np.array([-g, math.pi - g])
    upper = np.array([1.0 - g, math.pi + 1.0 - g])
    θ, r, rows, n_rays, bad, best = mine.search([6.0, 6.0], lower, upper, [1.0, -1.0], 0, r_min=m.inner_radius())
    first = lower + g * (upper - lower)
    assert np.all(np.abs(first - [0.0, math.pi]) < 1e-4)
    assert same_bytes(θ[:, 0], first + 1e-4) and not bad.any()


def test_tracer_without_solve_is_refused(G):
    TF = G.transfer_functions
    m, x, lock, _, mine = pair(G, 0.998, 60)
    with pytest.raises(ValueError, match="solve"):
        TF.cunningham_transfer_functions(m, x, G.ThinDisc(0.0, float("inf")), [6.0], N=20, N_extrema=5, tracer=lock, root_finder="device")
