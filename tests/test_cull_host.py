"""The start cull (Ray::init) and the step loop's culls (Ray::step: escape and polar-rate) on the kernel logic
compiled for the host (tests/host_harness_culls.cpp): whole 8 x 8 tiles traced with both mechanisms off, the start cull alone, the
step loop's culls alone and both.  The pixel bytes (NaN pattern included) and the status of every ray must be the same in all
four, each mechanism must take steps away, and no ray that an arm ended early may be one that hits the disc.  CPU only."""
import json
import math

import numpy as np
import pytest

import cull_scenes
import harness_culls as H

ARMS_ON = ("start", "step", "both")


def _check_exact(res):
    for arm, a in res["arms"].items():
        assert a["same_image"], arm
        assert a["same_status"], arm
        assert a["flagged"] == 0, arm
        assert a["wrongly_fired"] == 0, arm


def test_bench_tiles_all_arms_exact_and_fewer_steps(G):
    """400 random whole tiles of the 2048² bench plane (25 600 rays)."""
    cfg, pf = cull_scenes.bench_scene(G)
    nt = cull_scenes.SIZE // 8
    picks = np.random.default_rng(11).choice(nt * nt, size=400, replace=False)
    res, runs = H.census(G, cfg, pf, picks, *H.STEP)
    print(json.dumps(res, indent=1))
    _check_exact(res)
    a = res["arms"]
    assert 0.15 < res["hit_fraction"] < 0.5
    for arm in ARMS_ON:
        assert a[arm]["accepted_steps"] < a["off"]["accepted_steps"], arm
        assert a[arm]["wave_steps"] < a["off"]["wave_steps"], arm
        assert a[arm]["fired"] > 0, arm
    assert a["both"]["accepted_steps"] < min(a["start"]["accepted_steps"], a["step"]["accepted_steps"])
    # a ray decided at its start takes no step at all and keeps NoStatus
    s = runs["start"]
    dec = s["at_start"] == 1
    assert dec.sum() == a["start"]["decided_at_start_any"] > 0
    assert np.all(s["nacc"][dec] + s["nrej"][dec] == 0)
    assert np.all(s["status"][dec] == int(G.StatusCodes.NoStatus))
    assert np.all(np.isnan(s["image"][dec]))
    # The ratio tests/test_gpu_escape_cull.py brackets at 2048²: accepted steps with GRADUS_MI355X_ESCAPE_CULL unset over =0, the
    # start cull on in both arms.  The same bracket here, on a sample of the image's 65 536 tiles (scripts/cull_scenes.py: 0.645
    # on 1500 tiles, 0.637 on 1000, 0.640 on 200 with other seeds)
    assert 0.62 < res["escape_switch_bracket_ratio"] < 0.73, res["escape_switch_bracket_ratio"]


@pytest.mark.parametrize("case", ["disc500", "observer30", "gtol0.1"])
def test_other_scenes_all_arms_exact(G, case):
    """The scenes of tests/test_gpu_escape_cull.py::test_cull_exact_1024 at 64²: a disc that fills the field of view, an observer
    inside R_cull (the start cull asks r0 > R_cull: it cannot fire there, the step loop's culls do), a wider wedge."""
    x, r_out, kw = cull_scenes.X_OBS, 50.0, {}
    if case == "disc500":
        r_out = 500.0
    elif case == "observer30":
        x = np.array([0.0, 30.0, math.radians(75.0), 0.0])
    else:
        kw = {"gtol": 0.1}
    cfg, pf = cull_scenes.bench_scene(G, size=64, x=x, r_out=r_out, **kw)
    res, _ = H.census(G, cfg, pf, np.arange(64), *H.STEP)
    print(json.dumps(res, indent=1))
    _check_exact(res)
    a = res["arms"]
    if case == "disc500":
        # every ray hits the disc or falls into the hole: nothing to cull
        assert all(a[arm]["accepted_steps"] == a["off"]["accepted_steps"] for arm in ARMS_ON)
    elif case == "observer30":
        assert a["start"]["decided_at_start_any"] == 0 and a["start"]["accepted_steps"] == a["off"]["accepted_steps"]
        assert a["both"]["accepted_steps"] == a["step"]["accepted_steps"] < a["off"]["accepted_steps"]
    else:
        for arm in ARMS_ON:
            assert a[arm]["accepted_steps"] < a["off"]["accepted_steps"], arm
        assert a["both"]["accepted_steps"] < min(a["start"]["accepted_steps"], a["step"]["accepted_steps"])
