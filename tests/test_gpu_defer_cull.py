"""The defer cull (Ray::start_decided, Ray::step, GRADUS_MI355X_DEFER_CULL) of the fp64 trace kernels: one build in
one process with the switch unset against =0, on the bench window at 256².  Outputs byte for byte (NaN pattern included), the same
status counts and rays, no flagged ray, fewer accepted steps with it on; under each of the three switches that turn it off as
well its own switch changes nothing.  Needs an MI355X."""
import math

import numpy as np
import pytest

from test_gpu_pass_cull import _on_off, _render, _same_outputs

pytestmark = pytest.mark.gpu

DEFER_SWITCH = "GRADUS_MI355X_DEFER_CULL"


def _bench(G):
    m = G.KerrMetric(1.0, 0.998)
    return m, np.array([0.0, 1000.0, math.radians(75.0), 0.0]), G.ThinDisc(m.isco(), 50.0)


@pytest.mark.parametrize("kernel", [0, 1])
def test_defer_cull_exact_256(G, ens, monkeypatch, kernel):
    """The one-ray-per-lane and the persistent kernel."""
    ens.set("kernel", kernel).set("precision", 64)
    m, x, d = _bench(G)
    on, off = _on_off(monkeypatch, lambda: _render(G, ens, m, x, d, 256), DEFER_SWITCH)
    _same_outputs(on, off)
    s_on, s_off = int(on[1]["accepted_steps"]), int(off[1]["accepted_steps"])
    print(f"kernel {kernel}: accepted steps {s_on} / {s_off} = {s_on / s_off:.4f}")
    assert s_on < s_off


@pytest.mark.parametrize("other", ["GRADUS_MI355X_START_CULL", "GRADUS_MI355X_PASS_CULL", "GRADUS_MI355X_ESCAPE_CULL"])
def test_other_switches_turn_the_defer_cull_off(G, ens, monkeypatch, other):
    ens.set("kernel", 0).set("precision", 64)
    m, x, d = _bench(G)
    monkeypatch.setenv(other, "0")
    on, off = _on_off(monkeypatch, lambda: _render(G, ens, m, x, d, 256), DEFER_SWITCH)
    monkeypatch.delenv(other, raising=False)
    _same_outputs(on, off)
    assert int(on[1]["accepted_steps"]) == int(off[1]["accepted_steps"])
    assert int(on[1]["rejected_steps"]) == int(off[1]["rejected_steps"])
