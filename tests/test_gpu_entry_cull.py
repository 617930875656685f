"""The entry cull (Ray::step, GRADUS_MI355X_ENTRY_CULL) of the fp64 trace kernels: one build in one process with
the switch unset against =0.  Outputs byte for byte (NaN pattern included), the same status counts and rays, no flagged ray;
fewer accepted steps where the cull can fire and the same steps where it cannot -- no ray misses `disc500`, the observer of
`observer30` sits inside R_cull and no ray is armed, and a gated-off launch gets +inf for every radius.  Needs an MI355X."""
import math

import numpy as np
import pytest

from test_gpu_pass_cull import ALIMS, BLIMS, CANNOT_FIRE, SCENES, _on_off, _render, _same_outputs

pytestmark = pytest.mark.gpu

ENTRY_SWITCH = "GRADUS_MI355X_ENTRY_CULL"


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("name", list(SCENES))
def test_entry_cull_exact_256(G, ens, monkeypatch, name, kernel):
    """The eight scenes of tests/test_gpu_pass_cull.py; the one-ray-per-lane and the persistent kernel."""
    ens.set("kernel", kernel).set("precision", 64)
    a, r_obs, theta, r_out, kw = SCENES[name]
    m = G.KerrMetric(1.0, a)
    x = np.array([0.0, r_obs, math.radians(theta), 0.0])
    on, off = _on_off(monkeypatch, lambda: _render(G, ens, m, x, G.ThinDisc(m.isco(), r_out), 256, **kw), ENTRY_SWITCH)
    _same_outputs(on, off)
    s_on, s_off = int(on[1]["accepted_steps"]), int(off[1]["accepted_steps"])
    print(f"{name} kernel {kernel}: accepted steps {s_on} / {s_off} = {s_on / s_off:.4f}")
    if name in CANNOT_FIRE:
        assert s_on == s_off
    else:
        assert s_on < s_off


def test_gated_off_endpoints_unchanged_by_the_switch(G, ens, monkeypatch):
    """End points are never gated on: the host passes +inf for every radius, no ray is armed, the switch changes nothing."""
    ens.set("kernel", 2).set("precision", 64)
    m = G.KerrMetric(1.0, 0.998)
    x = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
    d = G.ThinDisc(m.isco(), 50.0)

    def run():
        _, _, cache = G.prerendergeodesics(m, x, d, 2000.0, image_width=256, image_height=256, alpha_lims=ALIMS, beta_lims=BLIMS,
                                           ensemble=ens)
        pts = np.ascontiguousarray(cache.points)
        return pts.tobytes(), int(np.sum(pts["status"] == G.StatusCodes.IntersectedWithGeometry))
    on, off = _on_off(monkeypatch, run, ENTRY_SWITCH)
    assert on == off


def test_bench_scene_2048_exact(G, ens, monkeypatch):
    """The bench workload once at full size: the entry cull changes no byte and no status; the accepted-step ratio is printed."""
    ens.set("kernel", 2).set("precision", 64)
    m = G.KerrMetric(1.0, 0.998)
    x = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
    d = G.ThinDisc(m.isco(), 50.0)
    on, off = _on_off(monkeypatch, lambda: _render(G, ens, m, x, d, 2048), ENTRY_SWITCH)
    _same_outputs(on, off)
    s_on, s_off = int(on[1]["accepted_steps"]), int(off[1]["accepted_steps"])
    print(f"accepted steps: entry cull on {s_on}, off {s_off} ({s_on / s_off:.4f})")
    assert s_on < s_off
