"""The start cull (Ray::init, GRADUS_MI355X_START_CULL) and the step loop's culls (Ray::step: escape and polar-rate,
GRADUS_MI355X_ESCAPE_CULL) of the fp64 trace kernels, DESIGN.md §5a.  Every comparison here runs one build in one process under
the four combinations of the two switches: outputs byte for byte, the same status counts and rays, no flagged ray; fewer accepted
steps with each mechanism on where it can fire, and the same steps where the host gates both off.  Needs an MI355X.

Where a mechanism cannot fire by its own precondition the steps are asserted EQUAL instead of fewer: no ray misses `disc500`
(neither mechanism fires), and the observer of `observer30` sits inside R_cull, where the start cull's r0 > R_cull never holds
(the step loop's culls do fire there)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_FAR = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
ALIMS, BLIMS = (-60.0, 60.0), (-35.0, 35.0)
STEP_SWITCH, START_SWITCH = "GRADUS_MI355X_ESCAPE_CULL", "GRADUS_MI355X_START_CULL"
ARMS = {"off": (False, False), "start": (False, True), "step": (True, False), "both": (True, True)}      # (step loop, start)


def _arms(monkeypatch, run):
    """{arm: result} under the four switch combinations"""
    out = {}
    for arm, (step, start) in ARMS.items():
        for name, on in ((STEP_SWITCH, step), (START_SWITCH, start)):
            if on:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, "0")
        out[arm] = run()
    monkeypatch.delenv(STEP_SWITCH, raising=False)
    monkeypatch.delenv(START_SWITCH, raising=False)
    return out


def _render(G, ens, m, x, d, size, pf=None, **kw):
    if pf is None:
        pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    _, _, img, st = G.rendergeodesics(m, x, d, 2000.0, image_width=size, image_height=size, alpha_lims=ALIMS,
                                      beta_lims=BLIMS, pf=pf, ensemble=ens, stats=True, **kw)
    return np.asarray(img), st


def _same_outputs(res):
    img_off, st_off = res["off"]
    for arm, (img, st) in res.items():
        assert img.tobytes() == img_off.tobytes(), arm          # NaN pattern included
        assert st["rays"] == st_off["rays"], arm
        assert list(st["status_count"]) == list(st_off["status_count"]), arm
        assert st["flagged_rays"] == 0, arm


def _steps(res):
    s = {arm: int(st["accepted_steps"]) for arm, (_, st) in res.items()}
    print("accepted steps:", s, "relative to off:", {k: round(v / s["off"], 4) for k, v in s.items()})
    return s


def test_bench_scene_2048_all_switch_combinations(G, ens, monkeypatch):
    """The bench workload: 2048² Kerr a = 0.998, ThinDisc(isco, 50), redshift ∘ filter_intersected."""
    ens.set("kernel", 2).set("precision", 64)
    m = G.KerrMetric(1.0, 0.998)
    d = G.ThinDisc(m.isco(), 50.0)
    res = _arms(monkeypatch, lambda: _render(G, ens, m, X_FAR, d, 2048))
    _same_outputs(res)
    s = _steps(res)
    assert s["start"] < s["off"] and s["step"] < s["off"]
    assert s["both"] < s["start"] and s["both"] < s["step"]


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("case", ["disc500", "observer30", "gtol0.1"])
def test_all_switch_combinations_1024(G, ens, monkeypatch, case, kernel):
    """Other radii, an observer inside R_cull, a wider wedge; the one-ray-per-lane and the persistent kernel."""
    ens.set("kernel", kernel).set("precision", 64)
    m = G.KerrMetric(1.0, 0.998)
    x, d, kw = X_FAR, G.ThinDisc(m.isco(), 50.0), {}
    if case == "disc500":
        d = G.ThinDisc(m.isco(), 500.0)
    elif case == "observer30":
        x = np.array([0.0, 30.0, math.radians(75.0), 0.0])
    else:
        kw = {"gtol": 0.1}
    res = _arms(monkeypatch, lambda: _render(G, ens, m, x, d, 1024, **kw))
    _same_outputs(res)
    s = _steps(res)
    if case == "disc500":
        # the disc fills the whole field of view: every ray hits it or falls into the hole, none is culled
        assert s["start"] == s["step"] == s["both"] == s["off"]
    elif case == "observer30":
        # r0 = 30 < R_cull: the start cull's first condition never holds
        assert s["start"] == s["off"]
        assert s["both"] == s["step"] < s["off"]
    else:
        assert s["start"] < s["off"] and s["step"] < s["off"]
        assert s["both"] < s["start"] and s["both"] < s["step"]


@pytest.mark.parametrize("case", ["endpoints", "hemisphere", "johannsen", "early_term", "tabulated_kerr"])
def test_gated_off_cases_unchanged_by_either_switch(G, ens, monkeypatch, case):
    """Where the host passes +inf for both radii neither switch changes anything: same steps, same bytes."""
    ens.set("kernel", 2).set("precision", 64)
    m = G.KerrMetric(1.0, 0.998)
    d = G.ThinDisc(m.isco(), 50.0)
    S = 256
    kw = dict(image_width=S, image_height=S, alpha_lims=ALIMS, beta_lims=BLIMS, ensemble=ens)
    if case == "endpoints":
        def run():
            _, _, cache = G.prerendergeodesics(m, X_FAR, d, 2000.0, **kw)
            pts = np.ascontiguousarray(cache.points)
            return pts.tobytes(), int(np.sum(pts["status"] == G.StatusCodes.IntersectedWithGeometry))
        res = _arms(monkeypatch, run)
        assert all(r == res["off"] for r in res.values())
        return
    if case == "hemisphere":
        run = lambda: _render(G, ens, m, X_FAR, d, S, callback=G.domain_upper_hemisphere())      # noqa: E731
    elif case == "johannsen":
        mj = G.JohannsenMetric(1.0, 0.7, 2.0, 0.0, 0.0, 1.0)
        dj = G.ThinDisc(mj.isco(), 50.0)
        run = lambda: _render(G, ens, mj, X_FAR, dj, S)      # noqa: E731
    elif case == "early_term":
        pf = G.ConstPointFunctions.affine_time() @ G.ConstPointFunctions.filter_early_term()
        run = lambda: _render(G, ens, m, X_FAR, d, S, pf=pf)      # noqa: E731
    else:
        mt = G.TabulatedMetric(m)
        run = lambda: _render(G, ens, mt, X_FAR, G.ThinDisc(m.isco(), 50.0), S)      # noqa: E731
    res = _arms(monkeypatch, run)
    img_off, st_off = res["off"]
    for arm, (img, st) in res.items():
        assert img.tobytes() == img_off.tobytes(), arm
        assert st["accepted_steps"] == st_off["accepted_steps"], arm
        assert list(st["status_count"]) == list(st_off["status_count"]), arm
