"""The defer cull (Ray::start_decided, Ray::step) on the kernel logic compiled for the host
(tests/host_harness_culls.cpp): whole 8 x 8 tiles traced as shipped, with the defer cull off, with the step loop's culls off
and in full.  Pixel bytes (NaN pattern included) and statuses must be identical in all arms and no ray flagged; every ray the
defer cull ended started outside R_cull going in, took exactly one accepted step, has NoStatus and a NaN pixel and misses in the
full trace; the decisions at the start are those of the same ζ without the defer cull; every ray the start marks is ended; the
GRADUS_MI355X_ESCAPE_CULL switch ratio stays inside the bracket of the older tests; each of the four switches turns it off.  The
closed forms themselves are those of the pass cull with a deeper depth limit: tests/test_pass_cull_bounds_host.py and
tests/test_entry_cull_host.py check them against root finding and quadrature down to ζ_dip.  CPU only."""
import json

import numpy as np
import pytest

import cull_scenes
import harness_culls as H
from cull_scenes import SCENES, bench_variant as scene


def _check_exact(G, cfg, res, runs):
    hit = int(G.StatusCodes.IntersectedWithGeometry)
    for arm, a in res["arms"].items():
        assert a["same_image"], arm
        assert a["same_status"], arm
        assert a["flagged"] == 0, arm
        assert a["wrongly_ended_early"] == 0, arm
    on, off, start, full = runs["all"], runs["no-defer"], runs["start"], runs["full"]
    assert np.all(full["at_start"] == 0) and not np.any(full["marked"]) and not np.any(full["entry_step"] > 0)
    # the defer cull marks only as shipped: off alone and with the step loop's culls off no ray carries the bit
    for arm in ("no-defer", "start", "full"):
        assert not np.any(runs[arm]["marked"]) and not np.any(runs[arm]["defer_end"]), arm
    # ... and every ray it marks it ends
    ended = on["defer_end"] == 1
    assert np.array_equal(on["marked"] == 1, ended)
    # the decisions at the start: those of the same ζ without the defer cull, and of the arm with the step loop's culls off
    assert np.array_equal(on["at_start"], off["at_start"]) and np.array_equal(on["at_start"], start["at_start"])
    assert not np.any(ended & (on["at_start"] == 1))
    rc = H.gate_radius(cfg)
    assert np.all(on["r_start"][ended] > rc) and np.all(on["vr_start"][ended] < 0.0)
    assert np.all(on["nacc"][ended] == 1)
    assert np.all(on["status"][ended] == int(G.StatusCodes.NoStatus))
    assert np.all(np.isnan(on["image"][ended]))
    assert not np.any(ended & (full["status"] == hit))
    assert not np.any(ended & (on["entry_step"] > 0))
    # every other ray takes the steps of the arm without the defer cull, and ends on entry there iff it does here
    att_on, att_off = on["nacc"] + on["nrej"], off["nacc"] + off["nrej"]
    assert np.array_equal(att_on[~ended], att_off[~ended])
    assert np.array_equal(on["entry_step"][~ended], off["entry_step"][~ended])
    assert np.all(att_on[ended] < att_off[ended])
    return ended


def test_constants_and_defaults():
    """memset + derive_params leave the entry cull and the defer cull on: render_tiles' defaults trace with both.  ζ_dip < ζ_defer < ζ."""
    assert H.default_culls() == (1, 1)
    assert H.zeta_dip() < H.zeta_defer() < H.zeta()
    assert H.zeta_dip() == 0.2


@pytest.fixture(scope="module")
def bench(G):
    """The 400 tiles of tests/test_cull_host.py (25 600 rays of the 2048² bench plane), every arm once."""
    cfg, pf = cull_scenes.bench_scene(G)
    nt = cull_scenes.SIZE // 8
    picks = np.random.default_rng(11).choice(nt * nt, size=400, replace=False)
    res, runs = H.census(G, cfg, pf, picks, *H.DEFER)
    return cfg, pf, picks, res, runs


def test_bench_tiles_defer_cull_exact_and_fires(G, bench):
    cfg, pf, picks, res, runs = bench
    print(json.dumps(res, indent=1))
    ended = _check_exact(G, cfg, res, runs)
    a = res["arms"]
    assert ended.sum() > 0
    assert a["all"]["accepted_steps"] < a["no-defer"]["accepted_steps"] < a["start"]["accepted_steps"] < a["full"]["accepted_steps"]
    assert a["all"]["wave_steps"] < a["no-defer"]["wave_steps"]
    # the entry cull keeps rays of its own (what chose kDeferCullZeta: at least 10 here)
    assert a["all"]["ended_on_entry"] >= 10
    # render_tiles' own defaults (memset + derive_params and the library's ζ) trace the same rays as the explicit "all" arm
    old = H.render_tiles(G, cfg, pf, picks[:50])
    assert np.array_equal(old["nacc"], runs["all"]["nacc"][:50]) and np.array_equal(old["nrej"], runs["all"]["nrej"][:50])
    # The ratio tests/test_gpu_escape_cull.py brackets at 2048²: accepted steps with GRADUS_MI355X_ESCAPE_CULL unset over =0
    print(f"GRADUS_MI355X_ESCAPE_CULL switch ratio on these tiles: {res['escape_switch_bracket_ratio']:.4f}")
    assert 0.62 < res["escape_switch_bracket_ratio"] < 0.73, res["escape_switch_bracket_ratio"]


def test_bench_tiles_each_switch_turns_the_defer_cull_off(G, bench):
    """GRADUS_MI355X_DEFER_CULL=0 alone, and GRADUS_MI355X_START_CULL=0, _PASS_CULL=0, _ESCAPE_CULL=0 each: no ray is marked or
    ended, and the defer cull's own switch then changes no step count.  (50 tiles; the arms of the fixture cover two of the four.)"""
    cfg, pf, picks, res, runs = bench
    t = picks[:50]
    assert runs["all"]["defer_end"][:50].sum() > 0
    #                    step start entry defer zeta
    for name, args in {"defer": (1, 1, 1, 0, -1.0), "start": (1, 0, 1, 1, -1.0), "pass": (1, 1, 1, 1, 0.0), "escape": (0, 1, 1, 1, -1.0)}.items():
        r = H.render_tiles(G, cfg, pf, t, *args)
        assert not np.any(r["marked"]) and not np.any(r["defer_end"]), name
        o = H.render_tiles(G, cfg, pf, t, *args[:3], 0, args[4])
        for k in ("nacc", "nrej", "at_start", "entry_step", "status"):
            assert np.array_equal(r[k], o[k]), (name, k)
        assert r["image"].tobytes() == o["image"].tobytes(), name


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_defer_cull_exact(G, name):
    """The scenes where the signs and closed forms can go wrong, at 64² (every tile).  `theta30` has no ray in the defer cull's band
    (its misses that enter R_cull turn deeper than R_defer or fail the closed forms): there it must end nothing."""
    cfg, pf, _ = scene(G, **SCENES[name])
    tiles = np.arange(64)
    res, runs = H.census(G, cfg, pf, tiles, *H.DEFER)
    ended = _check_exact(G, cfg, res, runs)
    a = res["arms"]
    print(name, json.dumps({k: a["all"][k] for k in ("decided_at_start_any", "ended_by_defer", "ended_on_entry", "accepted_steps")}),
          "no-defer", a["no-defer"]["ended_on_entry"], a["no-defer"]["accepted_steps"])
    if name == "theta30":
        assert ended.sum() == 0 and a["all"]["accepted_steps"] == a["no-defer"]["accepted_steps"]
        assert a["all"]["ended_on_entry"] == a["no-defer"]["ended_on_entry"] > 0
    else:
        assert ended.sum() > 0, name
        assert a["all"]["accepted_steps"] < a["no-defer"]["accepted_steps"], name
        assert a["all"]["ended_on_entry"] >= 10, name


@pytest.mark.parametrize("case", ["disc500", "observer30"])
def test_defer_cull_ends_nothing_where_it_cannot(G, case):
    """`disc500`: the disc fills the field of view, no ray misses.  `observer30`: r0 = 30 < R_cull, the start asks nothing."""
    if case == "disc500":
        cfg, pf, _ = scene(G, r_out=500.0)
    else:
        cfg, pf, _ = scene(G, r_obs=30.0)
    tiles = np.arange(64)
    res, runs = H.census(G, cfg, pf, tiles, *H.DEFER)
    ended = _check_exact(G, cfg, res, runs)
    assert ended.sum() == 0 and not np.any(runs["all"]["marked"])
    assert np.array_equal(runs["all"]["nacc"], runs["no-defer"]["nacc"]) and np.array_equal(runs["all"]["nrej"], runs["no-defer"]["nrej"])
