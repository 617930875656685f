"""The pass cull (Ray::start_decided) on the kernel logic compiled for the host (tests/host_harness_culls.cpp):
whole 8 x 8 tiles traced with the pass cull on and off, under the start cull alone and under all culls.  Pixel bytes (NaN pattern
included) and statuses must be identical, no ray flagged, no decided ray a hit of the arm without the cull; the cull must decide
something where it can and nothing where it cannot.  CPU only."""
import json

import numpy as np
import pytest

import cull_scenes
import harness_culls as H
from cull_scenes import SCENES, bench_variant as scene


def _check_exact(res):
    for arm, a in res["arms"].items():
        assert a["same_image"], arm
        assert a["same_status"], arm
        assert a["flagged"] == 0, arm
        assert a["wrongly_decided_by_pass"] == 0, arm


def test_bench_tiles_pass_cull_exact_and_switch_ratio_in_bracket(G):
    """The 400 tiles of tests/test_cull_host.py::test_bench_tiles_all_arms_exact_and_fewer_steps (25 600 rays of the 2048² bench
    plane) with the pass cull as the library has it."""
    cfg, pf = cull_scenes.bench_scene(G)
    nt = cull_scenes.SIZE // 8
    picks = np.random.default_rng(11).choice(nt * nt, size=400, replace=False)
    res, runs = H.census(G, cfg, pf, picks, *H.PASS)
    print(json.dumps(res, indent=1))
    _check_exact(res)
    a = res["arms"]
    for with_pass, without in (("start+pass", "start"), ("both+pass", "both")):
        assert a[with_pass]["decided_by_pass_cull"] > 0 and a[without]["decided_by_pass_cull"] == 0
        assert a[with_pass]["decided_by_start_test"] == a[without]["decided_by_start_test"] > 0      # the older test decides what it did
        assert a[with_pass]["accepted_steps"] < a[without]["accepted_steps"]
        assert a[with_pass]["wave_steps"] < a[without]["wave_steps"]
    # a ray the pass cull decides takes no step at all, keeps NoStatus and the fill value
    r = runs["both+pass"]
    dec = r["by_pass"] == 1
    assert np.all(r["nacc"][dec] + r["nrej"][dec] == 0)
    assert np.all(r["status"][dec] == int(G.StatusCodes.NoStatus))
    assert np.all(np.isnan(r["image"][dec]))
    # whole tiles are decided: the weak-field annulus is contiguous in the image
    assert a["both+pass"]["whole_tiles_decided"] > a["both"]["whole_tiles_decided"]
    # The ratio tests/test_cull_host.py and tests/test_gpu_escape_cull.py bracket -- accepted steps with GRADUS_MI355X_ESCAPE_CULL
    # unset over =0, the decisions at the start on in both arms -- recomputed with the pass cull on
    assert 0.62 < res["escape_switch_bracket_ratio"] < 0.73, res["escape_switch_bracket_ratio"]
    assert 0.62 < res["escape_switch_bracket_ratio_pass_off"] < 0.73, res["escape_switch_bracket_ratio_pass_off"]


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_pass_cull_exact_and_fires(G, name):
    """The scenes where the signs and closed forms can go wrong, at 64² (every tile)."""
    cfg, pf, _ = scene(G, **SCENES[name])
    res, _ = H.census(G, cfg, pf, np.arange(64), *H.PASS)
    print(json.dumps(res, indent=1))
    _check_exact(res)
    a = res["arms"]
    for with_pass, without in (("start+pass", "start"), ("both+pass", "both")):
        assert a[with_pass]["decided_by_pass_cull"] > 0, with_pass
        assert a[with_pass]["accepted_steps"] < a[without]["accepted_steps"], with_pass


@pytest.mark.parametrize("case", ["disc500", "observer30"])
def test_pass_cull_decides_nothing_where_it_cannot(G, case):
    """`disc500`: the disc fills the field of view, no ray misses.  `observer30`: r0 = 30 < R_cull."""
    if case == "disc500":
        cfg, pf, _ = scene(G, r_out=500.0)
    else:
        cfg, pf, _ = scene(G, r_obs=30.0)
    res, _ = H.census(G, cfg, pf, np.arange(64), *H.PASS)
    _check_exact(res)
    a = res["arms"]
    for with_pass, without in (("start+pass", "start"), ("both+pass", "both")):
        assert a[with_pass]["decided_by_pass_cull"] == 0
        assert a[with_pass]["accepted_steps"] == a[without]["accepted_steps"]
        assert a[with_pass]["wave_steps"] == a[without]["wave_steps"]
