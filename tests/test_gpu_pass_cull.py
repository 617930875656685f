"""The pass cull (Ray::start_decided, GRADUS_MI355X_PASS_CULL) of the fp64 trace kernels: one build in one
process with the switch unset against =0.  Outputs byte for byte (NaN pattern included), the same status counts and rays, no
flagged ray; fewer accepted steps where the cull can fire and the same steps where it cannot -- no ray misses `disc500`, the
observer of `observer30` sits inside R_cull, and the gated-off cases get +inf for every radius.  Needs an MI355X."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALIMS, BLIMS = (-60.0, 60.0), (-35.0, 35.0)
PASS_SWITCH, STEP_SWITCH = "GRADUS_MI355X_PASS_CULL", "GRADUS_MI355X_ESCAPE_CULL"
# name -> (a, observer r, observer θ in degrees, disc r_out, render keywords); the first six can fire, the last two cannot
SCENES = {
    "bench": (0.998, 1000.0, 75.0, 50.0, {}),
    "gtol0.1": (0.998, 1000.0, 75.0, 50.0, {"gtol": 0.1}),
    "a0": (0.0, 1000.0, 75.0, 50.0, {}),
    "a-0.998": (-0.998, 1000.0, 75.0, 50.0, {}),
    "theta30": (0.998, 1000.0, 30.0, 50.0, {}),
    "theta105": (0.998, 1000.0, 105.0, 50.0, {}),
    "disc500": (0.998, 1000.0, 75.0, 500.0, {}),
    "observer30": (0.998, 30.0, 75.0, 50.0, {}),
}
CANNOT_FIRE = ("disc500", "observer30")


def _on_off(monkeypatch, run, switch=PASS_SWITCH):
    monkeypatch.delenv(switch, raising=False)
    on = run()
    monkeypatch.setenv(switch, "0")
    off = run()
    monkeypatch.delenv(switch, raising=False)
    return on, off


def _render(G, ens, m, x, d, size, pf=None, **kw):
    if pf is None:
        pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    _, _, img, st = G.rendergeodesics(m, x, d, 2000.0, image_width=size, image_height=size, alpha_lims=ALIMS,
                                      beta_lims=BLIMS, pf=pf, ensemble=ens, stats=True, **kw)
    return np.asarray(img), st


def _same_outputs(on, off):
    (img_on, st_on), (img_off, st_off) = on, off
    assert img_on.tobytes() == img_off.tobytes()          # NaN pattern included
    assert st_on["rays"] == st_off["rays"]
    assert list(st_on["status_count"]) == list(st_off["status_count"])
    assert st_on["flagged_rays"] == 0 and st_off["flagged_rays"] == 0


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("name", list(SCENES))
def test_pass_cull_exact_256(G, ens, monkeypatch, name, kernel):
    """The bench scene and the scenes where the signs and closed forms can go wrong; the one-ray-per-lane and the persistent kernel."""
    ens.set("kernel", kernel).set("precision", 64)
    a, r_obs, theta, r_out, kw = SCENES[name]
    m = G.KerrMetric(1.0, a)
    x = np.array([0.0, r_obs, math.radians(theta), 0.0])
    on, off = _on_off(monkeypatch, lambda: _render(G, ens, m, x, G.ThinDisc(m.isco(), r_out), 256, **kw))
    _same_outputs(on, off)
    s_on, s_off = int(on[1]["accepted_steps"]), int(off[1]["accepted_steps"])
    print(f"{name} kernel {kernel}: accepted steps {s_on} / {s_off} = {s_on / s_off:.4f}")
    if name in CANNOT_FIRE:
        assert s_on == s_off
    else:
        assert s_on < s_off


@pytest.mark.parametrize("case", ["endpoints", "hemisphere", "johannsen", "early_term", "tabulated_kerr"])
def test_gated_off_cases_unchanged_by_the_switch(G, ens, monkeypatch, case):
    """The gated-off cases of tests/test_gpu_start_polar_cull.py: the host passes +inf for every radius, the switch changes nothing."""
    ens.set("kernel", 2).set("precision", 64)
    m = G.KerrMetric(1.0, 0.998)
    x = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
    d = G.ThinDisc(m.isco(), 50.0)
    S = 256
    if case == "endpoints":
        def run():
            _, _, cache = G.prerendergeodesics(m, x, d, 2000.0, image_width=S, image_height=S, alpha_lims=ALIMS, beta_lims=BLIMS,
                                               ensemble=ens)
            pts = np.ascontiguousarray(cache.points)
            return pts.tobytes(), int(np.sum(pts["status"] == G.StatusCodes.IntersectedWithGeometry))
        on, off = _on_off(monkeypatch, run)
        assert on == off
        return
    if case == "hemisphere":
        run = lambda: _render(G, ens, m, x, d, S, callback=G.domain_upper_hemisphere())      # noqa: E731
    elif case == "johannsen":
        mj = G.JohannsenMetric(1.0, 0.7, 2.0, 0.0, 0.0, 1.0)
        dj = G.ThinDisc(mj.isco(), 50.0)
        run = lambda: _render(G, ens, mj, x, dj, S)      # noqa: E731
    elif case == "early_term":
        pf = G.ConstPointFunctions.affine_time() @ G.ConstPointFunctions.filter_early_term()
        run = lambda: _render(G, ens, m, x, d, S, pf=pf)      # noqa: E731
    else:
        mt = G.TabulatedMetric(m)
        run = lambda: _render(G, ens, mt, x, G.ThinDisc(m.isco(), 50.0), S)      # noqa: E731
    (img_on, st_on), (img_off, st_off) = _on_off(monkeypatch, run)
    assert img_on.tobytes() == img_off.tobytes()
    assert st_on["accepted_steps"] == st_off["accepted_steps"]
    assert list(st_on["status_count"]) == list(st_off["status_count"])


def test_bench_scene_2048_exact_and_escape_switch_ratio(G, ens, monkeypatch):
    """The bench workload once at full size: the pass cull changes no byte and no status, and the accepted-step ratio of
    GRADUS_MI355X_ESCAPE_CULL unset over =0 (tests/test_gpu_escape_cull.py) stays inside its bracket with the pass cull on."""
    ens.set("kernel", 2).set("precision", 64)
    m = G.KerrMetric(1.0, 0.998)
    x = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
    d = G.ThinDisc(m.isco(), 50.0)
    on, off = _on_off(monkeypatch, lambda: _render(G, ens, m, x, d, 2048))
    _same_outputs(on, off)
    s_on, s_off = int(on[1]["accepted_steps"]), int(off[1]["accepted_steps"])
    assert s_on < s_off
    monkeypatch.setenv(STEP_SWITCH, "0")
    no_step = _render(G, ens, m, x, d, 2048)
    monkeypatch.delenv(STEP_SWITCH, raising=False)
    _same_outputs(on, no_step)
    ratio = s_on / int(no_step[1]["accepted_steps"])
    print(f"accepted steps: pass cull on {s_on}, off {s_off} ({s_on / s_off:.4f}); ESCAPE_CULL switch ratio {ratio:.4f}")
    assert 0.62 < ratio < 0.73, ratio
