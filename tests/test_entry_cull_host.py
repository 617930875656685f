"""The entry cull (Ray::step) on the kernel logic compiled for the host (tests/host_harness_culls.cpp): whole
8 x 8 tiles traced with the entry cull on and off under every other cull.  Pixel bytes (NaN pattern included) and statuses must be
identical, no ray flagged, no ray ended on entry a hit of the full trace; every such ray started outside R_cull and stands at or
inside it after its last step; the cull must fire where it can and end nothing where it cannot.  The closed forms it decides by
(KerrFamily::pass_cull_bounds with u0 >= uc) are checked against the quadrature of tests/test_pass_cull_bounds_host.py at the
states in which the step asks.  CPU only.

Tolerances of the quadrature check: those of tests/test_pass_cull_bounds_host.py (the bracket as it stands, 1e-9 of slack on the
time back at R_cull and the rates).  T_a^lo is asked to be <= 0 and nothing more: the ray is inside R_cull, the first visit of
the wedge ahead is the one the decision tests, and the formula is no bound of a negative time."""
import json
import math

import numpy as np
import pytest

import cull_scenes
import harness_culls as H
import test_pass_cull_bounds_host as B
from cull_scenes import SCENES, bench_variant as scene


def _check_exact(G, cfg, pf, tiles, res, runs):
    for arm, a in res["arms"].items():
        assert a["same_image"], arm
        assert a["same_status"], arm
        assert a["flagged"] == 0, arm
        assert a["wrongly_ended_on_entry"] == 0, arm
    on = runs["all"]
    ended = on["entry_step"] > 0
    assert not np.any(runs["no-entry"]["entry_step"] > 0) and not np.any(runs["start"]["entry_step"] > 0)
    # against the full trace: every cull off
    full = H.render_tiles(G, cfg, pf, tiles, step=0, start=0, entry=0, zeta=0.0)
    assert np.all(full["at_start"] == 0) and not np.any(full["entry_step"] > 0)
    assert on["image"].tobytes() == full["image"].tobytes()
    assert np.array_equal(on["status"], full["status"])
    assert not np.any(ended & (full["status"] == int(G.StatusCodes.IntersectedWithGeometry)))
    rc = H.gate_radius(cfg)
    assert np.all(on["r_last"][ended] <= rc)
    assert np.all(on["r_start"][ended] > rc)
    assert np.all(on["vr_last"][ended] < 0.0)
    assert np.all(on["status"][ended] == int(G.StatusCodes.NoStatus))
    assert np.all(np.isnan(on["image"][ended]))
    # a ray ended on entry took the steps of the arm without the cull up to that one
    att_on = on["nacc"] + on["nrej"]
    att_off = runs["no-entry"]["nacc"] + runs["no-entry"]["nrej"]
    assert np.all(att_on[ended] == on["entry_step"][ended]) and np.all(att_on[ended] < att_off[ended])
    assert np.array_equal(att_on[~ended], att_off[~ended])
    return ended


def test_derive_params_leaves_the_entry_cull_on():
    """memset + derive_params leave the entry cull on: render_tiles' default traces with it wherever r_cull and r_pass are finite."""
    assert H.default_culls()[0] == 1
    assert H.zeta_dip() == 0.2


def test_bench_tiles_entry_cull_exact_and_fires(G):
    """The 400 tiles of tests/test_cull_host.py (25 600 rays of the 2048² bench plane)."""
    cfg, pf = cull_scenes.bench_scene(G)
    nt = cull_scenes.SIZE // 8
    picks = np.random.default_rng(11).choice(nt * nt, size=400, replace=False)
    res, runs = H.census(G, cfg, pf, picks, *H.ENTRY)
    print(json.dumps(res, indent=1))
    ended = _check_exact(G, cfg, pf, picks, res, runs)
    a = res["arms"]
    assert ended.sum() > 0
    assert a["all"]["decided_at_start_any"] == a["no-entry"]["decided_at_start_any"] == a["start"]["decided_at_start_any"] > 0
    assert a["all"]["accepted_steps"] < a["no-entry"]["accepted_steps"] < a["start"]["accepted_steps"]
    assert a["all"]["wave_steps"] < a["no-entry"]["wave_steps"]
    # render_tiles' own defaults (memset + derive_params and the library's ζ) trace the same rays as the explicit "all" arm
    old = H.render_tiles(G, cfg, pf, picks[:50])
    assert np.array_equal(old["nacc"], runs["all"]["nacc"][:50]) and np.array_equal(old["nrej"], runs["all"]["nrej"][:50])
    print(f"GRADUS_MI355X_ESCAPE_CULL switch ratio on these tiles: {res['escape_switch_bracket_ratio']:.4f}")


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_entry_cull_exact_and_fires(G, name):
    """The scenes where the signs and closed forms can go wrong, at 64² (every tile)."""
    cfg, pf, _ = scene(G, **SCENES[name])
    tiles = np.arange(64)
    res, runs = H.census(G, cfg, pf, tiles, *H.ENTRY)
    print(json.dumps(res, indent=1))
    ended = _check_exact(G, cfg, pf, tiles, res, runs)
    assert ended.sum() > 0, name
    assert res["arms"]["all"]["accepted_steps"] < res["arms"]["no-entry"]["accepted_steps"], name


@pytest.mark.parametrize("case", ["disc500", "observer30"])
def test_entry_cull_ends_nothing_where_it_cannot(G, case):
    """`disc500`: the disc fills the field of view, no ray misses.  `observer30`: r0 = 30 < R_cull, no ray is armed."""
    if case == "disc500":
        cfg, pf, _ = scene(G, r_out=500.0)
    else:
        cfg, pf, _ = scene(G, r_obs=30.0)
    tiles = np.arange(64)
    res, runs = H.census(G, cfg, pf, tiles, *H.ENTRY)
    ended = _check_exact(G, cfg, pf, tiles, res, runs)
    assert ended.sum() == 0
    a = res["arms"]
    assert a["all"]["accepted_steps"] == a["no-entry"]["accepted_steps"]
    assert a["all"]["wave_steps"] == a["no-entry"]["wave_steps"]
    assert np.array_equal(runs["all"]["nacc"], runs["no-entry"]["nacc"]) and np.array_equal(runs["all"]["nrej"], runs["no-entry"]["nrej"])


def _check_entry_bounds(cfg, a, rays):
    """The bounds at the asking state of each ray against root finding and quadrature; returns (bounds, asked, decided)."""
    b = H.entry_bounds(cfg, rays.ravel())
    asked = b["asked"] == 1.0
    assert np.all(b["u0"][asked] >= b["uc"][asked])          # at or inside R_cull
    assert np.all(b["vr"][asked] < 0.0)
    formed = np.flatnonzero(asked & (b["Tb_hi"] > 0.0))     # rays whose radial side went through
    loose_b = []
    for i in formed[:: max(1, formed.size // 400)]:
        E, Q, w2, c1, q4 = B._coeffs(b, i, a)
        ut = B._turning_point(E, w2, c1, q4, b["uc"][i])
        assert b["u_lo"][i] <= ut <= b["u_hi"][i], (i, b["u_lo"][i], ut, b["u_hi"][i])
        assert b["u0"][i] < b["u_lo"][i]
        quot, _ = np.polydiv(np.array([-q4, c1, -w2, 0.0, E * E]), np.array([1.0, -ut]))
        P = -quot
        t0, tc = B._mino_time(P, ut, b["u0"][i]), B._mino_time(P, ut, b["uc"][i])
        Ta, Tb = t0 - tc, t0 + tc       # Ta <= 0: minus the time since R_cull was passed; Tb: back at R_cull, from now
        # inside R_cull the formula of T_a^lo bounds nothing (the upper harmonic bound makes it >= Ta there); the decision needs
        # its sign alone: <= 0, so that the first visit ahead is the one tested
        assert Ta <= 0.0 and b["Ta_lo"][i] <= 0.0, (i, b["Ta_lo"][i], Ta)
        assert b["Tb_hi"][i] >= Tb * (1.0 - 1e-9), (i, b["Tb_hi"][i], Tb)
        loose_b.append(b["Tb_hi"][i] / Tb - 1.0)
    polar = np.flatnonzero(asked & (b["Om_hi"] > 0.0))
    gtol = cfg.abi_config().gtol
    for i in polar[:: max(1, polar.size // 400)]:
        E, Q, w2, c1, q4 = B._coeffs(b, i, a)
        A = a * a * E * E
        mp2 = Q / w2 if A == 0.0 else float(np.max(np.roots([A, w2, -Q]).real))
        mu = math.sqrt(mp2) * np.linspace(-0.999, 0.999, 201)
        rate = np.sqrt((Q - w2 * mu ** 2 - A * mu ** 4) / (mp2 - mu ** 2))
        assert b["Om_lo"][i] * (1.0 - 1e-9) <= rate.min() and rate.max() <= b["Om_hi"][i] * (1.0 + 1e-9), (i, rate.min(), rate.max())
        assert math.isclose(math.sqrt(mp2) * math.sin(b["psi0"][i]), b["mu0"][i], rel_tol=1e-9, abs_tol=1e-12)
        assert (math.cos(b["psi0"][i]) >= 0.0) == (b["mu_rising"][i] == 1.0)
        assert abs(b["mu0"][i]) > gtol
        if b["decided"][i] == 1.0:
            # the decision itself, from the reported bounds: the first visit of the wedge ahead starts after T_b^hi
            delta = math.asin(gtol / math.sqrt(mp2))
            n1 = next(n for n in range(4) if n * math.pi - delta > b["psi0"][i])
            assert (n1 * math.pi - delta - b["psi0"][i]) / b["Om_hi"][i] > b["Tb_hi"][i]
    decided = asked & (b["decided"] == 1.0)
    if loose_b:
        print(f"rays {rays.size}, asked {int(asked.sum())}, radial side formed {formed.size}, decided {int(decided.sum())}; "
              f"looseness of T_b^hi {np.min(loose_b):.4f}..{np.max(loose_b):.4f}")
    return b, asked, decided


def test_bench_plane_entry_bounds_enclose_and_decided_rays_miss(G):
    """8 tiles of the 2048² bench plane on the image's diagonal from the rim of the disc's image outwards (512 rays)."""
    cfg, pf, a = scene(G, size=2048)
    nt = 2048 // 8
    tiles = np.array([k * nt + k for k in (40, 56, 64, 72, 80, 88, 96, 104)])
    rays = B.tile_rays(tiles, 2048)
    b, asked, decided = _check_entry_bounds(cfg, a, rays)
    assert asked.sum() >= 100 and decided.sum() > 0
    hit = B._full_trace_hits(G, cfg, pf, tiles)
    assert not np.any(decided & hit)


@pytest.mark.parametrize("name", ["bench64", "a0", "a-0.998", "theta105"])
def test_scene_entry_bounds_enclose_and_decided_rays_miss(G, name):
    """Every ray of the scene at 64² for the decision, up to 400 asking states for the numerics."""
    cfg, pf, a = scene(G, **SCENES[name])
    tiles = np.arange(64)
    rays = B.tile_rays(tiles, 64)
    b, asked, decided = _check_entry_bounds(cfg, a, rays)
    assert decided.sum() > 0, name
    hit = B._full_trace_hits(G, cfg, pf, tiles)
    assert not np.any(decided & hit), name
