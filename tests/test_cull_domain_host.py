"""The miss culls (Ray::start_decided, Ray::step) against the uncut trace over the whole domain their gate lets them
act in, on the kernel logic compiled for the host (tests/host_harness_culls.cpp): the scene table of tests/cull_scenes.py --
M != 1, |a| = M, observers face-on, edge-on, below the plane, on and just outside R_cull, rings and discs whose R_cull is R_esc,
gtol near the gate's limit, windows off the centre and off the disc, and both outcomes of "λ1 comes first" -- and 40 scenes
drawn inside the gate.  The library as shipped (every cull on) against every cull off: pixel bytes (NaN pattern included) and
statuses identical, no ray flagged, no ray ended early that the full trace sees hit, and each mechanism fires exactly where
cull_scenes.FIRES says it does, so that a cull that has gone silent does not pass as exact.  CPU only."""
import json

import numpy as np
import pytest

import cull_scenes as CS
import harness_culls as H

SIZE = 64
ALL_TILES = np.arange((SIZE // 8) ** 2)
_named = {}


def _arms(G, name):
    """The named scene at 64², every tile, both arms: traced once per session."""
    if name not in _named:
        cfg, rc, on, off = CS.host_arms(G, CS.scene(G, name, SIZE), ALL_TILES)
        for r in (on, off):
            for v in r.values():
                v.setflags(write=False)
        _named[name] = (cfg, rc, on, off, CS.counts(G, on, off))
    return _named[name]


def _check_exact(G, on, off, c):
    assert on["image"].tobytes() == off["image"].tobytes()          # NaN pattern included
    assert np.array_equal(on["status"], off["status"])
    assert not np.any(on["status"] < 0) and not np.any(off["status"] < 0)
    assert c["wrongly_ended"] == 0
    # the uncut arm decides, marks and ends nothing
    assert not np.any(off["at_start"]) and not np.any(off["marked"]) and not np.any(off["defer_end"]) and not np.any(off["entry_step"] > 0)
    # the culls only ever take steps away
    assert np.all(on["nacc"].astype(np.int64) + on["nrej"] <= off["nacc"].astype(np.int64) + off["nrej"])


def test_scene_table_is_the_one_the_culls_are_gated_for(G):
    """The table is complete, FIRES names every scene, and R_cull is what the scene says: R_esc = 4 M for a disc inside it, else
    r_out / sqrt(1 - gtol²), in the scene's M."""
    assert set(CS.FIRES) == set(CS.NAMED) and len(CS.NAMED) == 30
    for name in CS.NAMED:
        p = CS.parameters(name)
        _, _, rc = CS.configuration(G, CS.scene(G, name, SIZE))
        gtol = 1e-2 if p["gtol"] is None else p["gtol"]
        assert rc == pytest.approx(p["M"] * CS.gate_radius_closed_form(1.0, p["r_out"], gtol), rel=1e-14), name
    # `rout3`: R_cull is R_esc itself; `rout4`: the disc's reach, 5e-5 beyond it
    assert CS.gate_radius_closed_form(1.0, 3.0, 1e-2) == 4.0 * (1.0 + 1e-6) < CS.gate_radius_closed_form(1.0, 4.0, 1e-2) < 4.001


@pytest.mark.parametrize("name", list(CS.NAMED))
def test_named_scene_exact_and_fires(G, name):
    cfg, rc, on, off, c = _arms(G, name)
    print(name, f"R_cull {rc:.6g}", json.dumps(c))
    _check_exact(G, on, off, c)
    for k in CS.MECHANISMS:
        assert (c[k] > 0) == (k in CS.FIRES[name]), (name, k, c[k])
    if not CS.FIRES[name]:
        assert np.array_equal(on["nacc"], off["nacc"]) and np.array_equal(on["nrej"], off["nrej"])
        assert c["attempted_on"] == c["attempted_off"]
    else:
        assert c["attempted_on"] < c["attempted_off"]


def test_named_table_every_mechanism_fires_in_five_scenes(G):
    for k in CS.MECHANISMS:
        by_table = [n for n in CS.NAMED if k in CS.FIRES[n]]
        measured = [n for n in CS.NAMED if _arms(G, n)[4][k] > 0]
        print(k, len(measured), measured)
        assert by_table == measured
        assert len(measured) >= 5, k


@pytest.mark.parametrize("name", CS.LAMBDA1_BOUNDARY)
def test_lambda1_first_boundary_both_outcomes(G, name):
    """The start's reach bound r0 + B (λ1 - λ0) fails for every ray (max_time 11500 M under the 12000 M chart; 2000 M under a
    1100 M chart): it decides and marks nothing.  The entry cull forms the same bound at R_cull with the affine time that is left
    and ends more than 1000 rays.  The statuses are the full trace's either way."""
    cfg, rc, on, off, c = _arms(G, name)
    print(name, json.dumps(c))
    assert c["start"] == 0 and c["defer"] == 0 and not np.any(on["marked"])
    assert c["entry"] > 1000
    # the same scene under a bound that holds decides at the start: it is the bound that kept the start silent
    assert _arms(G, "bench")[4]["start"] > 1000
    _check_exact(G, on, off, c)
    assert np.all(on["status"][on["entry_step"] > 0] == int(G.StatusCodes.NoStatus))


def test_offdisc_every_tile_decided_and_census_ratios(G):
    """A window off the disc: every ray is decided at the start, no tile is traced, and the census of each mechanism -- which forms
    its ratios from a denominator of 0 here -- reports 1.0: nothing was traced in either arm."""
    cfg, rc, on, off, c = _arms(G, "offdisc")
    assert c["start"] == 64 * 64 and c["whole_tiles_decided"] == 64 and c["attempted_on"] == 0 and c["hit_share"] == 0.0
    assert np.all(np.isnan(on["image"])) and np.all(on["status"] == int(G.StatusCodes.NoStatus))
    _, pf, _ = CS.configuration(G, CS.scene(G, "offdisc", SIZE))
    res, _ = H.census(G, cfg, pf, ALL_TILES, *H.DEFER)
    assert res["arms"]["all"]["wave_steps"] == 0 and res["arms"]["no-defer"]["wave_steps"] == 0
    assert res["defer_wave_steps_ratio"] == 1.0 and res["defer_accepted_steps_ratio"] == 1.0
    assert res["escape_switch_bracket_ratio"] == 1.0
    assert all(a["same_image"] and a["same_status"] and a["wrongly_ended_early"] == 0 for a in res["arms"].values())
    res, _ = H.census(G, cfg, pf, ALL_TILES, *H.PASS)
    assert res["arms"]["both+pass"]["whole_tiles_decided"] == 64
    assert res["pass_wave_steps_ratio"] == 1.0 and res["pass_accepted_steps_ratio"] == 1.0 and res["escape_switch_bracket_ratio"] == 1.0
    res, _ = H.census(G, cfg, pf, ALL_TILES[:16], *H.ENTRY)
    assert res["entry_wave_steps_ratio"] == 1.0 and res["entry_accepted_steps_ratio"] == 1.0 and res["escape_switch_bracket_ratio"] == 1.0
    # a traced window still gets the quotient itself
    cfg_b, _, on_b, _, c_b = _arms(G, "bench")
    _, pf_b, _ = CS.configuration(G, CS.scene(G, "bench", SIZE))
    res, _ = H.census(G, cfg_b, pf_b, ALL_TILES[:16], *H.PASS)
    a = res["arms"]
    assert res["pass_wave_steps_ratio"] == a["both+pass"]["wave_steps"] / a["both"]["wave_steps"] < 1.0


def test_random_scenes_exact(G):
    """40 scenes drawn inside the gate's domain (cull_scenes.random_parameters), 16 tiles each.  Every draw's gate radius is finite
    (cull_scenes.configuration asserts it), at most a quarter of the scenes end no ray early, and the scenes in which nothing at
    all fires are those the device test expects equal steps of."""
    silent, quiet, r_esc_scenes = 0, [], 0
    for i, (p, built) in enumerate(CS.random_scenes(G, CS.SEED, CS.N_RANDOM, SIZE)):
        cfg, rc, on, off = CS.host_arms(G, built, CS.random_tiles(p, SIZE))
        c = CS.counts(G, on, off)
        print(i, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in p.items() if k != "tile_seed"}, f"R_cull {rc:.5g}",
              {k: c[k] for k in CS.MECHANISMS}, f"{c['step_ratio']:.3f}")
        assert on["status"].shape == (16, 64)
        # R_cull carries M: the closed form in units of M, times the scene's M (R_esc = 4 M where the disc ends inside it)
        assert rc == pytest.approx(p["M"] * CS.gate_radius_closed_form(1.0, p["r_out"], p["gtol"]), rel=1e-14)
        r_esc_scenes += p["r_out"] < CS.ESCAPE_RADIUS_M and abs(p["M"] - 1.0) > 0.2
        _check_exact(G, on, off, c)
        silent += not (c["start"] or c["defer"] or c["entry"])
        if not CS.fired(c):
            quiet.append(i)
            assert np.array_equal(on["nacc"], off["nacc"]) and np.array_equal(on["nrej"], off["nrej"])
    print(f"seed {CS.SEED}: {silent} of {CS.N_RANDOM} scenes end no ray early; nothing fires in {quiet}")
    assert 4 * silent <= CS.N_RANDOM
    assert quiet == list(CS.RANDOM_QUIET)
    assert r_esc_scenes >= 1          # some draw has R_cull = R_esc with M well away from 1
