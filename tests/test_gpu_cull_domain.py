"""The miss culls of the fused fp64 Kerr kernels (Ray::start_decided, Ray::step) against the uncut trace over the
whole domain their gate lets them act in: the scene table of tests/cull_scenes.py (what tests/test_cull_domain_host.py asks of
the host build) on the device.  One build in one process, every cull on (no switch set) against every cull off (all five
GRADUS_MI355X_{ESCAPE,START,PASS,ENTRY,DEFER}_CULL=0): image bytes (NaN pattern included), rays and status counts equal, no ray
flagged, fewer accepted steps where cull_scenes.FIRES says a mechanism fires and the same steps where it says none does.  Also
image sizes that are no multiple of the 8 x 8 tile, the line-profile outputs (bins and (g, ρ) pairs) on both ray layouts and over
several contexts, and -- the leg that shares no code with the culls -- the uncut image against the oracle at the new corners.
Needs an MI355X.

`_render` of tests/test_gpu_pass_cull.py fixes the window and max_time of the bench scene, which the table varies; `_render` here
takes the scene's own.  `_same_outputs` is that file's."""
import math

import numpy as np
import pytest

import cull_scenes as CS
from test_gpu_pass_cull import _same_outputs

pytestmark = pytest.mark.gpu

SWITCHES = tuple(f"GRADUS_MI355X_{k}_CULL" for k in ("ESCAPE", "START", "PASS", "ENTRY", "DEFER"))
# the scenes that also run on the persistent kernel (1) and on the library's choice (2)
OTHER_KERNELS = ("bench", "M2.5", "th90", "obs51", "offdisc", "t11500", "outer1100")
RAGGED = ((100, 52), (8, 200))
RTOL = 1e-6          # the redshift map against the oracle (tests/test_gpu_parity.py)


def _on_off(monkeypatch, run):
    """(run() with every cull on, run() with every cull off): all five switches deleted, then all five set to 0."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    on = run()
    for s in SWITCHES:
        monkeypatch.setenv(s, "0")
    off = run()
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    return on, off


def _render(G, ens, built):
    m, x, d, max_time, kw = built
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    _, _, img, st = G.rendergeodesics(m, x, d, max_time, pf=pf, ensemble=ens, stats=True, **kw)
    assert img.shape == (kw["image_height"], kw["image_width"])
    return np.asarray(img), st


def _exact(G, ens, monkeypatch, built, label):
    """Both arms of one scene: the same outputs; (accepted steps on, off), printed."""
    on, off = _on_off(monkeypatch, lambda: _render(G, ens, built))
    s_on, s_off = int(on[1]["accepted_steps"]), int(off[1]["accepted_steps"])
    print(f"{label}: accepted steps {s_on} / {s_off} = {s_on / s_off:.4f}")
    _same_outputs(on, off)
    assert on[1]["rays"] == built[4]["image_width"] * built[4]["image_height"]
    return s_on, s_off


def _steps_as_fires(name, s_on, s_off):
    if CS.FIRES[name]:
        assert s_on < s_off, name
    else:
        assert s_on == s_off, name


@pytest.mark.parametrize("name,kernel", [(n, 0) for n in CS.NAMED] + [(n, k) for n in OTHER_KERNELS for k in (1, 2)])
def test_named_scene_exact_128(G, ens, monkeypatch, name, kernel):
    ens.set("kernel", kernel).set("precision", 64)
    s_on, s_off = _exact(G, ens, monkeypatch, CS.scene(G, name, 128), f"{name} kernel {kernel}")
    _steps_as_fires(name, s_on, s_off)
    if name == "offdisc":
        assert s_on == 0          # every tile is decided at the start


@pytest.mark.parametrize("kernel", [0, 2])
@pytest.mark.parametrize("size", RAGGED, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["bench", "offcentre", "offdisc"])
def test_ragged_tiles_exact(G, ens, monkeypatch, name, size, kernel):
    """Widths and heights that are no multiple of 8: tiles with lanes that have no ray, next to lanes the start decides and (in
    `offdisc`) whole waves that leave for their fill-value stores without a step."""
    ens.set("kernel", kernel).set("precision", 64)
    s_on, s_off = _exact(G, ens, monkeypatch, CS.scene(G, name, size), f"{name} {size[0]} x {size[1]} kernel {kernel}")
    _steps_as_fires(name, s_on, s_off)
    if name == "offdisc":
        assert s_on == 0


def test_random_scenes_exact_64(G, ens, monkeypatch):
    """The first 12 scenes of the host file's seed, whole 64² images.  The host traced 16 of each image's 64 tiles: where a cull
    fired on those the device takes fewer steps; in the scenes of cull_scenes.RANDOM_QUIET it may take as many."""
    ens.set("kernel", 0).set("precision", 64)
    for i, (p, built) in enumerate(CS.random_scenes(G, CS.SEED, 12, 64)):
        CS.configuration(G, built)          # the gate radius is finite
        s_on, s_off = _exact(G, ens, monkeypatch, built, f"random {i} (M {p['M']:.2f}, a {p['a']:+.2f} M, θ {p['theta']:.0f}°)")
        assert s_on <= s_off
        if i not in CS.RANDOM_QUIET:
            assert s_on < s_off, i


def _profile_scene(G, M):
    """Kerr 0.998, observer (1000, 40°), ThinDisc(0, 50), no hemisphere callback, PolarPlane 64 x 96 out to 250; lengths in M."""
    m = G.KerrMetric(M, 0.998 * M)
    u = np.array([0.0, 1000.0 * M, math.radians(40.0), 0.0])
    d = G.ThinDisc(0.0, 50.0 * M)
    plane = G.PolarPlane(G.GeometricGrid(), Nr=64, Nθ=96, r_min=1.0 * M, r_max=250.0 * M)
    kw = dict(plane=plane, callback=None, maxrₑ=50.0 * M, chart=G.chart_for_metric(m, 12000.0 * M))
    return m, u, d, kw


@pytest.mark.parametrize("layout", ["separable", "explicit"])
@pytest.mark.parametrize("M", [1.0, 2.5])
@pytest.mark.parametrize("route", ["bins", "pairs"])
def test_lineprofile_outputs_exact(G, ens, monkeypatch, route, M, layout):
    """out_mode 2 (line-profile bins fused into finalize, PowerLawEmissivity) and out_mode 3 ((g, ρ) pairs, a callable
    emissivity) against every cull off, on the tiled separable plane and on explicit α / β arrays.  The bins are sums of fp64
    atomics whose order is not fixed between two launches: the bound of test_cull_exact_lineprofile_binning.  The pairs are per
    ray and bucketed on the host in one order: bit-equal."""
    ens.set("precision", 64)
    monkeypatch.setenv("GRADUS_MI355X_SEPARABLE_RAYS", "1" if layout == "separable" else "0")
    m, u, d, kw = _profile_scene(G, M)
    bins = np.linspace(0.1, 1.5, 120)
    emissivity = G.PowerLawEmissivity(3) if route == "bins" else (lambda r: r ** -3.0)

    def run():
        _, y, st = G.lineprofile(bins, emissivity, m, u, d, G.BinningMethod(), ensemble=ens, stats=True, **kw)
        return np.asarray(y), st

    (y_on, st_on), (y_off, st_off) = _on_off(monkeypatch, run)
    s_on, s_off = int(st_on["accepted_steps"]), int(st_off["accepted_steps"])
    print(f"{route} M {M} {layout}: accepted steps {s_on} / {s_off} = {s_on / s_off:.4f}")
    assert st_on["rays"] == st_off["rays"] == 64 * 96
    assert np.count_nonzero(y_off) > 20 and np.all(np.isfinite(y_off))
    if route == "bins":
        np.testing.assert_allclose(y_on, y_off, rtol=1e-12, atol=1e-15 * float(np.max(np.abs(y_off))))
    else:
        assert y_on.tobytes() == y_off.tobytes()
    assert list(st_on["status_count"]) == list(st_off["status_count"])
    assert st_on["flagged_rays"] == st_off["flagged_rays"] == 0
    assert s_on < s_off


@pytest.fixture(scope="module")
def three(G):
    return G.EnsembleMI355X(devices=[0, 0, 0])


@pytest.mark.parametrize("M", [1.0, 2.5])
def test_lineprofile_bins_over_three_contexts_exact(G, ens, three, monkeypatch, M):
    """The fused bins with the plane's rays dealt over three contexts, every cull on, against one context with every cull off."""
    ens.set("precision", 64)
    m, u, d, kw = _profile_scene(G, M)
    bins = np.linspace(0.1, 1.5, 120)
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    _, y_on, st_on = G.lineprofile(bins, G.PowerLawEmissivity(3), m, u, d, G.BinningMethod(), ensemble=three, stats=True, **kw)
    for s in SWITCHES:
        monkeypatch.setenv(s, "0")
    _, y_off, st_off = G.lineprofile(bins, G.PowerLawEmissivity(3), m, u, d, G.BinningMethod(), ensemble=ens, stats=True, **kw)
    _, y_off3, st_off3 = G.lineprofile(bins, G.PowerLawEmissivity(3), m, u, d, G.BinningMethod(), ensemble=three, stats=True, **kw)
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    s_on, s_off = int(st_on["accepted_steps"]), int(st_off["accepted_steps"])
    print(f"three contexts M {M}: accepted steps {s_on} / {s_off} = {s_on / s_off:.4f}")
    assert np.count_nonzero(y_off) > 20
    np.testing.assert_allclose(y_on, y_off, rtol=1e-12, atol=1e-15 * float(np.max(np.abs(y_off))))
    assert list(st_on["status_count"]) == list(st_off["status_count"]) == list(st_off3["status_count"])
    assert st_on["rays"] == st_off["rays"] == 64 * 96
    # the switches reach every context: off over three contexts takes the steps of off on one
    assert int(st_off3["accepted_steps"]) == s_off
    assert s_on < s_off


@pytest.mark.parametrize("name", ["M2.5", "th90", "a-0.7_th150"])
def test_uncut_image_matches_oracle_64(G, oracle, ens, monkeypatch, name):
    """The on / off comparison shares the integrator between its arms; this one does not.  The all-off redshift image of the new
    corners (M != 1, an edge-on observer, one below the plane of a retrograde hole) against the oracle, at the bar of
    test_redshift_image_matches_oracle_128: rtol 1e-6 on the common hits the oracle itself determines to 1e-7 (it is run at
    1e-9 and at 0.9e-9, as tests/test_gpu_baseline_configs.py does), rim flips at most 0.002 of the pixels.  The oracle's two
    tolerances flip 2, 0 and 0 pixels between themselves here (host, 64²): inside that allowance of 8."""
    ens.set("kernel", 0).set("precision", 64)
    W = H = 64
    built = CS.scene(G, name, W)
    m, x, d, max_time, kw = built
    for s in SWITCHES:
        monkeypatch.setenv(s, "0")
    img, st = _render(G, ens, built)
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    refs = []
    for tol in (1e-9, 0.9e-9):
        cfg = oracle.make_config("kerr", (m.M, m.a), disc=(d.inner_radius, d.outer_radius), lambda_max=max_time, abstol=tol,
                                 reltol=tol, outer_radius=kw["chart"].outer_radius)
        refs.append(oracle.rendergeodesics(cfg, x, kw["alpha_lims"], kw["beta_lims"], W, H, pf_id=oracle.PF_REDSHIFT,
                                           filter_id=oracle.FILTER_INTERSECTED, r_isco=m.isco()))
    ref, ref2 = refs
    assert st["rays"] == W * H and st["flagged_rays"] == 0
    nan_i, nan_r, nan_2 = np.isnan(img), np.isnan(ref), np.isnan(ref2)
    both = ~nan_i & ~nan_r
    safe = np.where(both, ref, 1.0)
    rel = np.where(both, np.abs(img / safe - 1.0), 0.0)
    spread = np.where(both & ~nan_2, np.abs(np.where(nan_2, 1.0, ref2) / safe - 1.0), np.inf)
    well = both & (spread < 1e-7)
    print(f"{name}: rim flips {int((nan_i != nan_r).sum())} (the oracle against itself {int((nan_r != nan_2).sum())}), common hits "
          f"{int(both.sum())}, of them determined to 1e-7 {int(well.sum())}, max rel err there {rel[well].max():.3e}, anywhere "
          f"{rel[both].max():.3e}")
    assert (nan_r != nan_2).sum() <= 0.002 * W * H
    assert (nan_i != nan_r).sum() <= 0.002 * W * H
    assert well.sum() > 250          # that test asks 1000 common hits of 128²: 250 of 64², and of the determined ones
    assert rel[well].max() < RTOL
