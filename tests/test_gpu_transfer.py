"""TraceRadiativeTransfer on the device: gr_transfer_render / gr_transfer_endpoints (kernelsrt_m<id>.o) asked what
tests/test_transfer_host.py asked the host build of the same kernel text -- the independent golden with the bound asserted on the
CPU, the exact statements, the equilibrium -- plus what only a launch can get wrong: partial waves, waves that mix lanes inside the
medium, outside it and already finished, the image plane's tile order against the ray list, and every refusal.

Scenes, rays, media and bounds: tests/transfer_scene.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

import transfer_scene as S

pytestmark = pytest.mark.gpu
SCENES = ("A", "B")
W = H = 32
ALIMS, BLIMS = (-14.0, 14.0), (-5.0, 5.0)
GR_ERR_UNSUPPORTED = -2


def device_scene(G, ens, name, md, cache={}):
    """(records, intensities) of every fixture ray of a scene under a medium, from the device: once per (scene, medium)"""
    import json

    key = (name, json.dumps(md, sort_keys=True))
    if key not in cache:
        al, be, _ = S.rays(name)
        cache[key] = G.ensemble_solve_tracing_problem(ens, S.configuration(G, name, S.medium_trace(G, md), al, be, ensemble=ens))
    return cache[key]


def test_render_through_the_torus_returns_an_image(G, ens):
    """the gate: this raised NotImplementedError("trace TraceRadiativeTransfer has no device implementation")"""
    m, x, d, lam = S.setup(G, "A")
    trace = G.TraceRadiativeTransfer(I0=0.0, medium=G.PowerLawMedium(j0=0.1))
    a, b, img = G.rendergeodesics(m, x, d, lam, image_width=W, image_height=H, alpha_lims=ALIMS, beta_lims=BLIMS, trace=trace,
                                  ensemble=ens, abstol=S.TOL, reltol=S.TOL)
    assert img.shape == (H, W) and np.all(np.isfinite(img))
    lit = img > 0.0
    assert 100 <= lit.sum() <= 600 and np.all(img[~lit] == 0.0)      # the torus's silhouette, dark sky around it
    assert 0.05 < img.max() < 5.0


@pytest.mark.parametrize("medium", ["emission", "absorption", "both", "equilibrium"])
@pytest.mark.parametrize("scene", SCENES)
def test_endpoints_against_the_independent_integration(G, ens, scene, medium):
    md = S.golden()["media"][medium]
    pts, I = device_scene(G, ens, scene, md)
    dev = S.deviation(I, S.golden_intensity(scene, medium))
    print(f"scene {scene} {medium}: max deviation {dev.max():.3e} (bound {S.GOLDEN_BOUND:.1e})")
    assert not np.any(pts["flags"] & 0xFFFF)
    assert dev.max() <= S.GOLDEN_BOUND


@pytest.mark.parametrize("scene", SCENES)
def test_exact_statements(G, ens, scene):
    crossing = np.array([len(r["crossings"]) > 0 for r in S.rays(scene)[2]])
    zero = dict(nu0=1.0, I0=0.7, a0=0.0, j0=0.0, pa=0.0, pj=0.0, sa=0.0, sj=0.0)
    assert np.all(device_scene(G, ens, scene, zero)[1] == 0.7)
    dark = dict(S.golden()["media"]["absorption"], I0=0.0)
    assert np.all(device_scene(G, ens, scene, dark)[1] == 0.0)
    em = dict(S.golden()["media"]["emission"], I0=0.25)
    pts, I = device_scene(G, ens, scene, em)
    assert np.all(I >= 0.25) and np.all(I[crossing] > 0.25) and np.all(I[~crossing] == 0.25)
    # a ray that never crosses ends with the status of the plain trace
    al, be, _ = S.rays(scene)
    plain = G.ensemble_solve_tracing_problem(ens, S.configuration(G, scene, None, al, be, ensemble=ens))
    assert np.array_equal(pts["status"][~crossing], plain["status"][~crossing])


@pytest.mark.parametrize("scene", SCENES)
def test_equilibrium_and_superposition(G, ens, scene):
    eq, ab, Sv = S.superposition_media()
    I_at = device_scene(G, ens, scene, dict(eq, I0=Sv))[1]
    assert np.abs(I_at / Sv - 1).max() <= S.EQUILIBRIUM_BOUND
    I_eq, I_ab = device_scene(G, ens, scene, eq)[1], device_scene(G, ens, scene, ab)[1]
    d = np.abs(I_eq - (Sv + (eq["I0"] - Sv) * I_ab / ab["I0"])) / Sv
    print(f"scene {scene}: superposition holds to {d.max():.2e} (bound {S.SUPERPOSITION_BOUND:.1e})")
    assert d.max() <= S.SUPERPOSITION_BOUND


def test_launch_shapes_give_the_same_bits_per_ray(G, ens):
    """n = 1, 63, 64, 65 and 256 rays of scene A's list: a partial wave, a full one, one ray more, four waves.  The list runs down
    the image's columns, so a wave holds rays inside the medium, rays that never meet it and rays the hole has taken."""
    md = S.golden()["media"]["both"]
    al, be, rs = S.rays("A")
    assert al.size >= 255
    al, be = np.append(al, al[:1]), np.append(be, be[:1])      # the 256th ray: the first once more
    full_pts, full_I = G.ensemble_solve_tracing_problem(ens, S.configuration(G, "A", S.medium_trace(G, md), al[:256], be[:256], ensemble=ens))
    assert (full_I != md["I0"]).sum() >= 40 and (full_I == md["I0"]).sum() >= 40
    assert full_I[255] == full_I[0]
    for n in (1, 63, 64, 65):
        pts, I = G.ensemble_solve_tracing_problem(ens, S.configuration(G, "A", S.medium_trace(G, md), al[:n], be[:n], ensemble=ens))
        assert I.shape == (n,)
        assert np.array_equal(I.view(np.uint64), full_I[:n].view(np.uint64)), n
        assert pts.tobytes() == full_pts[:n].tobytes(), n


def test_render_equals_endpoints_on_the_same_rays(G, ens):
    """the 32² render (8 x 8 tiles per wave, tile order) against gr_transfer_endpoints on the same 1024 rays in ray order.  The
    rays are the plane's own: the initial velocities of its end-point records (ray i = x H + y), not a second derivation."""
    m, x, d, lam = S.setup(G, "A")
    trace = S.medium_trace(G, S.golden()["media"]["both"])
    kw = dict(image_width=W, image_height=H, alpha_lims=ALIMS, beta_lims=BLIMS, ensemble=ens, abstol=S.TOL, reltol=S.TOL)
    a, b, img = G.rendergeodesics(m, x, d, lam, trace=trace, **kw)
    rec = G.ensemble_solve_tracing_problem(ens, G.render_configuration(m, x, d, lam, **kw))
    cfg = G.tracing_configuration(m, x, np.ascontiguousarray(rec["v_init"]), d, lam, trace=trace, ensemble=ens, abstol=S.TOL, reltol=S.TOL)
    pts, I = G.ensemble_solve_tracing_problem(ens, cfg)
    flat = np.ascontiguousarray(img.T).ravel()
    assert (flat != trace.I0).sum() >= 100
    assert np.array_equal(flat.view(np.uint64), I.view(np.uint64))


def _refusal_cases(G):
    m, x, d, lam = S.setup(G, "A")
    kerr = G.KerrMetric(1.0, 0.5)
    yield "thin disc", dict(m=kerr, d=G.ThinDisc(0.0, 20.0))
    yield "datum plane", dict(m=kerr, d=G.DatumPlane(0.0))
    yield "warped table", dict(m=kerr, d=G.WarpedThinDisc(lambda r: 0.1 * math.sin(r), inner_radius=2.0, outer_radius=20.0, samples=64))
    yield "no ISCO: Morris-Thorne", dict(m=G.MorrisThorneWormhole(1.0), d=d)
    yield "no ISCO: flat space", dict(m=G.SphericalMetric(), d=d)
    yield "precision 32", dict(m=kerr, d=d, precision=32)
    yield "q != 0", dict(m=G.KerrNewmanMetric(1.0, 0.5, 0.3), d=d, q=0.5)
    yield "count_windings", dict(m=kerr, d=d, windings=True)
    yield "tabulated metric", dict(m=kerr, d=d, metric_id=11)
    yield "compiled metric", dict(m=kerr, d=d, metric_id=12)


def test_every_refusal(G, ens):
    L = G._lib.load()
    x = np.array([0.0, 100.0, math.radians(85.0), 0.0])
    n = 64
    v = np.tile(np.array([1.0, -1.0, 0.0, 0.0]), (n, 1))
    names = []
    for name, case in _refusal_cases(G):
        cfgo = G.tracing_configuration(case["m"], x, v, case["d"], 200.0, ensemble=ens)
        cfg = cfgo.abi_config()
        if "q" in case:
            cfg.q = case["q"]
        if case.get("windings"):
            cfg.count_windings, cfg.winding_plane = 1, math.pi / 2
        if "metric_id" in case:
            cfg.metric_id = case["metric_id"]
        ens.set("precision", case.get("precision", 64))
        tr = G.TraceRadiativeTransfer(medium=G.PowerLawMedium(a0=0.3)).abi_transfer(6.0)
        pts = np.zeros(n, dtype=G._lib.POINT_DTYPE)
        I = np.full(n, -7.0)
        st = G._lib.gr_stats()
        rc = L.gr_transfer_endpoints(ens.ctx.handle, C.byref(cfg), C.byref(tr), x.ctypes.data, 0, v.ctypes.data, n, pts.ctypes.data,
                                     I.ctypes.data, C.byref(st))
        ens.set("precision", 64)
        assert rc == GR_ERR_UNSUPPORTED, (name, rc, L.gr_last_error())
        assert L.gr_last_error(), name
        assert np.all(I == -7.0) and st.rays == 0, name      # nothing was launched, nothing written
        # ... and the render refuses the same
        pl = G.render_configuration(case["m"], x, case["d"], 200.0, image_width=8, image_height=8, alpha_lims=(-5, 5),
                                    beta_lims=(-5, 5), ensemble=ens).abi_plane()
        pf = G._lib.gr_pointfunction()
        pf.pf_id, pf.fill = 5, float("nan")
        rg = G._lib.gr_range(0, 64, 64, 1)
        img = np.full(64, -7.0)
        ens.set("precision", case.get("precision", 64))
        rc = L.gr_transfer_render(ens.ctx.handle, C.byref(cfg), C.byref(tr), C.byref(pl), C.byref(pf), C.byref(rg), img.ctypes.data, None)
        ens.set("precision", 64)
        assert rc == GR_ERR_UNSUPPORTED and np.all(img == -7.0), (name, rc)
        names.append(name)
    assert len(names) == 10
    # a point function other than the intensity is refused by the render, and the Python layer says so before it calls
    m, xa, d, lam = S.setup(G, "A")
    with pytest.raises(NotImplementedError):
        G.rendergeodesics(m, xa, d, lam, image_width=8, image_height=8, trace=G.TraceRadiativeTransfer(), ensemble=ens,
                          pf=G.ConstPointFunctions.affine_time())
    with pytest.raises(ValueError):
        G.rendergeodesics(m, xa, lam, image_width=8, image_height=8, trace=G.TraceRadiativeTransfer(), ensemble=ens)
