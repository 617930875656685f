"""The escape cull of the fp64 trace kernels (Ray::step): an outgoing ray beyond R_cull whose pixel is already
decided stops early.  Every comparison here is cull on (the default) against GRADUS_MI355X_ESCAPE_CULL=0 on the same build, in
one process: outputs byte for byte, the same status counts and rays, fewer accepted steps where the cull is on and the same
steps where the host gates it off.  Needs an MI355X."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_FAR = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
ALIMS, BLIMS = (-60.0, 60.0), (-35.0, 35.0)
SWITCH = "GRADUS_MI355X_ESCAPE_CULL"


def _ab(monkeypatch, run):
    """(result with the cull on, result with it off)"""
    monkeypatch.delenv(SWITCH, raising=False)
    on = run()
    monkeypatch.setenv(SWITCH, "0")
    off = run()
    monkeypatch.delenv(SWITCH, raising=False)
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
    assert st_on["flagged_rays"] == st_off["flagged_rays"] == 0


def test_bench_scene_2048_cull_is_exact_and_cuts_steps(G, ens, monkeypatch):
    """The bench workload: 2048² Kerr a = 0.998, ThinDisc(isco, 50), redshift ∘ filter_intersected."""
    ens.set("kernel", 2).set("precision", 64)
    m = G.KerrMetric(1.0, 0.998)
    d = G.ThinDisc(m.isco(), 50.0)
    on, off = _ab(monkeypatch, lambda: _render(G, ens, m, X_FAR, d, 2048))
    _same_outputs(on, off)
    ratio = on[1]["accepted_steps"] / off[1]["accepted_steps"]
    # the CPU census of scripts/escape_census.py: 0.674 of the accepted steps
    assert 0.62 < ratio < 0.73, ratio


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("case", ["disc500", "observer30", "gtol0.1"])
def test_cull_exact_1024(G, ens, monkeypatch, case, kernel):
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
    on, off = _ab(monkeypatch, lambda: _render(G, ens, m, x, d, 1024, **kw))
    _same_outputs(on, off)
    if case == "disc500":
        # the disc fills the whole field of view: every ray hits it or falls into the hole, none is culled
        assert on[1]["accepted_steps"] == off[1]["accepted_steps"]
    else:
        assert on[1]["accepted_steps"] < off[1]["accepted_steps"]


def test_cull_exact_lineprofile_binning(G, ens, monkeypatch):
    """out_mode 2 (BinningMethod fused into finalize) without the hemisphere callback: the histograms agree.  The bins are
    sums of fp64 atomics, whose order is not fixed between two launches: equal to rounding."""
    ens.set("precision", 64)
    m = G.KerrMetric(1.0, 0.998)
    u = np.array([0.0, 1000.0, math.radians(40.0), 0.0])
    d = G.ThinDisc(0.0, 50.0)
    bins = np.linspace(0.1, 1.5, 120)
    plane = G.PolarPlane(G.GeometricGrid(), Nr=200, Nθ=400, r_max=250.0)

    def run():
        x, y, st = G.lineprofile(bins, G.PowerLawEmissivity(3), m, u, d, G.BinningMethod(), plane=plane, callback=None,
                                 ensemble=ens, stats=True)
        return np.asarray(y), st

    (y_on, st_on), (y_off, st_off) = _ab(monkeypatch, run)
    np.testing.assert_allclose(y_on, y_off, rtol=1e-12, atol=1e-15 * float(np.max(np.abs(y_off))))
    assert list(st_on["status_count"]) == list(st_off["status_count"])
    assert st_on["accepted_steps"] < st_off["accepted_steps"]


@pytest.mark.parametrize("case", ["endpoints", "hemisphere", "johannsen", "early_term", "tabulated_kerr"])
def test_gated_off_cases_unchanged(G, ens, monkeypatch, case):
    """Where the host passes R_cull = +inf the switch changes nothing: same steps, same bytes."""
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
        on, off = _ab(monkeypatch, run)
        assert on == off
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
    (img_on, st_on), (img_off, st_off) = _ab(monkeypatch, run)
    assert img_on.tobytes() == img_off.tobytes()
    assert st_on["accepted_steps"] == st_off["accepted_steps"]
    assert list(st_on["status_count"]) == list(st_off["status_count"])
