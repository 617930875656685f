"""GR_METRIC_COMPILED on the device: a user's metric_components through kernels compiled for it (metrics.CompiledMetric,
gr_metric_module_load).  The metric of no catalogue against the oracle running the same function through its dual numbers; Kerr
written as a callable against the oracle, the tangent oracle and the fused Kerr kernels; the module registry (two modules at
once, a slot reused, an unloaded id, a full registry), several contexts, and what a compiled metric does not have (fp32).
"""
import ctypes as C
import math

import numpy as np
import pytest

from test_compiled_metric_host import BUMP, MODULES, R_H_BUMP, X_FAR, _compare_endpoints, bump_components, kerr_callable

pytestmark = pytest.mark.gpu

A_KERR = 0.998
R_H_KERR = 1.0 + math.sqrt(1.0 - A_KERR ** 2)


@pytest.fixture(scope="session")
def cm_bump(G, oracle):
    with oracle.user_metric_library():
        isco = oracle.isco(oracle.make_config("test-bump", BUMP))
    return G.CompiledMetric(bump_components, inner_radius=R_H_BUMP, isco=isco, cache_dir=MODULES)


@pytest.fixture(scope="session")
def cm_kerr(G):
    return G.CompiledMetric(kerr_callable, inner_radius=R_H_KERR, isco=G.KerrMetric(1.0, A_KERR).isco(), cache_dir=MODULES)


@pytest.fixture(scope="session")
def cm_third(G):
    """a third metric for the slot another one leaves: Kerr a = 0.5 with its spin as a run-time parameter"""
    return G.CompiledMetric(lambda r, th, p: kerr_callable(r, th, (1.0, p[0])), params=(0.5,), inner_radius=1.0 + math.sqrt(0.75),
                            isco=G.KerrMetric(1.0, 0.5).isco(), cache_dir=MODULES)


@pytest.fixture(scope="module", autouse=True)
def _modules_built(cm_bump, cm_kerr, cm_third):
    """the three kernel modules, compiled once per session (and found in the cache by every later one); the registry is left as
    this file found it -- empty: other tests count on the ids above the catalogue being refused"""
    from gradus_jl_amd import compiled_metric

    for m in (cm_bump, cm_kerr, cm_third):
        m.compile()
    yield
    compiled_metric.unload_all()


@pytest.mark.parametrize("which", ["bump", "kerr"])
def test_compiled_endpoints_vs_oracle_on_device(G, ens, oracle, which, cm_bump, cm_kerr):
    """the 96 x 96 plane of test_tabulated_endpoints_vs_oracle_on_device at that test's bars"""
    cm, name, params = {"bump": (cm_bump, "test-bump", BUMP), "kerr": (cm_kerr, "kerr", (1.0, A_KERR))}[which]
    W = H = 96
    disc = (3.0, 400.0)
    _, _, cache = G.prerendergeodesics(cm, X_FAR, G.ThinDisc(*disc), 2000.0, image_width=W, image_height=H, alpha_lims=(-60, 60),
                                       beta_lims=(-35, 35), ensemble=ens)
    got = np.ascontiguousarray(np.asarray(cache.points).T).reshape(-1)
    ocfg = oracle.make_config(name, params, disc=disc, lambda_max=2000.0)
    if which == "bump":
        with oracle.user_metric_library():
            ref = oracle.trace(ocfg, X_FAR, oracle.render_velocities(ocfg, X_FAR, (-60, 60), (-35, 35), W, H))
    else:
        ref = oracle.trace(ocfg, X_FAR, oracle.render_velocities(ocfg, X_FAR, (-60, 60), (-35, 35), W, H))
    _compare_endpoints(got, ref, x_rtol=1e-6, max_flips=8, max_outliers=5, r_horizon=cm.inner_radius())


def test_compiled_user_metric_redshift_image_vs_oracle(G, ens, oracle, cm_bump):
    """The whole render path of test_user_metric_redshift_image_vs_oracle: generic ISCO machinery, device-traced plunging table
    (the module's path kernel), redshift ∘ filter, at that test's bars"""
    W = H = 64
    isco = cm_bump.isco()
    pf = G.ConstPointFunctions.redshift(cm_bump, X_FAR, ensemble=ens) @ G.ConstPointFunctions.filter_intersected()
    a, b, img = G.rendergeodesics(cm_bump, X_FAR, G.ThinDisc(isco, 40.0), 2000.0, image_width=W, image_height=H, alpha_lims=(-50, 50),
                                  beta_lims=(-30, 30), pf=pf, ensemble=ens)
    ocfg = oracle.make_config("test-bump", BUMP, disc=(isco, 40.0), lambda_max=2000.0)
    with oracle.user_metric_library():
        ref = oracle.rendergeodesics(ocfg, X_FAR, (-50, 50), (-30, 30), W, H, pf_id=oracle.PF_REDSHIFT,
                                     filter_id=oracle.FILTER_INTERSECTED, r_isco=isco)
    assert int(np.sum(np.isnan(img) != np.isnan(ref))) <= 4
    both = ~np.isnan(img) & ~np.isnan(ref)
    assert both.sum() > 500
    assert np.max(np.abs(img[both] / ref[both] - 1.0)) < 1e-6


def _ray_tangent(G, ens, m, x, al, be, pairs):
    """gr_ray_tangent of the rays (al, be) against DatumPlane(0) in the shape `pairs` (0: one lane per ray, 1: a pair of lanes) --
    device_tracer's own `tangent` always takes the pairs"""
    from gradus_jl_amd import _lib
    from gradus_jl_amd.rendering import abi_pointfunction
    from gradus_jl_amd.tracing import lnr_momentum_to_global_velocity_matrix, tracing_configuration

    ens.set("tangent_pairs", pairs)
    chart = G.chart_for_metric(m, 2 * x[1], closest_approach=1.005)
    config = tracing_configuration(m, x, np.zeros((1, 4)), G.DatumPlane(0.0), 2 * x[1], chart=chart, ensemble=ens)
    cfg = config.abi_config()
    pf, keep = abi_pointfunction(G.ConstPointFunctions.redshift(m, x, ensemble=ens))
    Mx = lnr_momentum_to_global_velocity_matrix(m, config.position)
    rs = _lib.gr_rayset()
    for i in range(4):
        rs.x_obs[i] = float(config.position[i])
        for k in range(4):
            rs.Mx[4 * i + k] = float(Mx[i, k])
    al, be = np.ascontiguousarray(al, dtype=np.float64), np.ascontiguousarray(be, dtype=np.float64)
    rs.alpha, rs.beta, rs.area, rs.n = al.ctypes.data, be.ctypes.data, None, al.size
    out, st = np.zeros((al.size, 8)), _lib.gr_stats()
    _lib.check(_lib.load().gr_ray_tangent(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), out.ctypes.data, C.byref(st)))
    assert st.rays == al.size
    return out


@pytest.mark.parametrize("pairs", [0, 1])
def test_compiled_tangents_equal_the_tangent_oracle_ray_by_ray(G, ens, oracle, cm_kerr, pairs):
    """gr_ray_tangent of Kerr-as-a-callable in both shapes: the scene and the bars of
    test_tangents_through_the_table_equal_the_tangent_oracle_ray_by_ray"""
    ens.set("kernel", 2).set("precision", 64)
    kerr = G.KerrMetric(1.0, A_KERR)
    x = np.array([0.0, 100_000.0, math.radians(30), 0.0])
    rng = np.random.default_rng(2026)
    rr, th = rng.uniform(2.5, 14.0, 300), rng.uniform(0.0, 2 * math.pi, 300)
    th[:4] = [math.pi / 2, math.pi / 2 + 1e-3, 3 * math.pi / 2, 0.0]
    al, be = rr * np.cos(th), rr * np.sin(th)
    dev = {name: _ray_tangent(G, ens, m, x, al, be, pairs) for name, m in (("compiled", cm_kerr), ("fused", kerr))}
    cfg = oracle.make_config("kerr", (1.0, A_KERR), disc={"datum": 0.0}, lambda_max=2 * x[1], closest_approach=1.005, outer_radius=2 * x[1])
    orc = oracle.ray_tangent(cfg, x, al, be, r_isco=kerr.isco(), max_time=2 * x[1], norm_with_tangents=True)

    def rel(d_, o_, cols):
        out = np.zeros(d_.shape[0])
        for lo in cols:
            scale = np.maximum(np.abs(o_[:, lo]), np.abs(o_[:, lo + 1]))
            out = np.maximum(out, np.max(np.abs(d_[:, lo:lo + 2] - o_[:, lo:lo + 2]), axis=1) / scale)
        return out

    t = dev["compiled"]
    assert np.array_equal(t[:, 7], orc[:, 7]) and np.array_equal(t[:, 7], dev["fused"][:, 7])
    hit = t[:, 7] == 2
    assert hit.sum() > 250
    outside = hit & (t[:, 1] > 1.02 * kerr.isco())          # (inside the ISCO g rests on the traced plunge, as for the table)
    assert 0 < (hit & ~outside).sum() < 10
    np.testing.assert_allclose(t[hit, 1], orc[hit, 1], rtol=1e-5)
    np.testing.assert_allclose(t[outside, 0], orc[outside, 0], rtol=1e-5)
    np.testing.assert_allclose(t[hit, 0], orc[hit, 0], rtol=1e-3)
    e_orc = rel(t[outside], orc[outside], (2, 4))
    e_fused = rel(t[outside], dev["fused"][outside], (2, 4))
    e_rad = rel(t[hit], orc[hit], (4,))
    print(f"  compiled tangents (pairs={pairs}): vs the tangent oracle max {e_orc.max():.2e} median {np.median(e_orc):.2e} "
          f"(∂ρ of all hits: {e_rad.max():.2e}); vs the fused tangent kernel max {e_fused.max():.2e}")
    assert e_orc.max() < 1e-5 and np.median(e_orc) < 2e-6 and e_rad.max() < 1e-5
    assert e_fused.max() < 1e-6


@pytest.mark.parametrize("root_finder", ["reference", "device"])
def test_transfer_function_of_a_compiled_metric(G, ens, cm_kerr, root_finder):
    """One Cunningham transfer function of Kerr-as-a-callable against the fused Kerr metric by the same route: the scene and the bar
    of test_transfer_functions_of_a_tabulated_metric (its `reference` part: duals through the tracer)"""
    ens.set("kernel", 2).set("precision", 64)
    kerr = G.KerrMetric(1.0, A_KERR)
    x = np.array([0.0, 1000.0, math.radians(40), 0.0])
    d = G.ThinDisc(0.0, float("inf"))
    (ca,) = G.cunningham_transfer_functions(kerr, x, d, [12.0], N=60, ensemble=ens, root_finder=root_finder)
    (cc,) = G.cunningham_transfer_functions(cm_kerr, x, d, [12.0], N=60, ensemble=ens, root_finder=root_finder)
    ok = np.isfinite(ca.f) & np.isfinite(cc.f)
    assert ok.sum() >= ca.f.size - 2
    assert cc.gmin == pytest.approx(ca.gmin, rel=1e-7) and cc.gmax == pytest.approx(ca.gmax, rel=1e-7)
    sa, sc = float(np.sum((ca.f * ca.g_star)[ok]) / ca.f.size), float(np.sum((cc.f * cc.g_star)[ok]) / cc.f.size)
    assert sc == pytest.approx(sa, abs=3e-4)


@pytest.mark.parametrize("n", [1, 63, 65])
def test_compiled_kernels_agree_bitwise_on_small_ray_sets(G, ens, cm_bump, n):
    """test_kernels_agree_bitwise's claim for a module's two trace kernels, on ray sets that end inside a wave"""
    rng = np.random.default_rng(n)
    vs = G.map_impact_parameters(cm_bump, X_FAR, rng.uniform(-20, 20, n), rng.uniform(-12, 12, n))
    out = []
    for kernel in (0, 1):
        ens.set("kernel", kernel)
        out.append(G.tracegeodesics(cm_bump, X_FAR, vs, G.ThinDisc(3.0, 400.0), 2000.0, ensemble=ens).copy())
    assert out[0].shape == (n,) and out[0].tobytes() == out[1].tobytes()


def _image(G, ens, m, size=32, **kw):
    _, _, cache = G.prerendergeodesics(m, X_FAR, G.ThinDisc(3.0, 400.0), 2000.0, image_width=size, image_height=size,
                                       alpha_lims=(-60, 60), beta_lims=(-35, 35), ensemble=ens, **kw)
    return np.asarray(cache.points).copy()


def test_two_modules_at_once_and_a_reused_slot(G, ens, cm_bump, cm_kerr, cm_third):
    from gradus_jl_amd import _lib

    L = _lib.load()
    kerr = G.KerrMetric(1.0, A_KERR)
    fused = _image(G, ens, kerr)
    for m in (cm_bump, cm_kerr, cm_third):          # loaded in this order, each into the lowest free slot: bump < kerr < third
        m.unload()
    ids = (cm_bump.metric_id, cm_kerr.metric_id)
    assert ids[0] < ids[1] and all(12 <= i < 28 for i in ids)
    solo = {"bump": _image(G, ens, cm_bump), "kerr": _image(G, ens, cm_kerr)}
    assert solo["bump"].tobytes() != solo["kerr"].tobytes()
    for _ in range(2):
        assert _image(G, ens, cm_bump).tobytes() == solo["bump"].tobytes()
        assert _image(G, ens, cm_kerr).tobytes() == solo["kerr"].tobytes()
    # the third metric in a slot of its own, then in the slot Kerr leaves -- at a size and with the knobs at which the context
    # learns a tile order per (config, plane): the key holds the module's build id, the slot number says nothing
    ens.set("kernel", 1).set("lpt", 2)
    third_solo = _image(G, ens, cm_third, size=384)
    assert cm_third.metric_id > ids[1]
    kerr_big = [_image(G, ens, cm_kerr, size=384) for _ in range(3)]          # (recorded, sorted, used)
    assert kerr_big[1].tobytes() == kerr_big[0].tobytes() == kerr_big[2].tobytes()
    cm_third.unload()
    freed = cm_kerr.metric_id
    cm_kerr.unload()
    assert cm_third.metric_id == freed
    for _ in range(3):
        assert _image(G, ens, cm_third, size=384).tobytes() == third_solo.tobytes()
    ens.set("kernel", 2).set("lpt", 1)
    assert _image(G, ens, cm_third).tobytes() != solo["kerr"].tobytes()
    # the same kernels with another parameter value: nothing is compiled or loaded again
    other = cm_third.with_params(0.9)
    assert other.metric_id == cm_third.metric_id and _image(G, ens, other).tobytes() != _image(G, ens, cm_third).tobytes()
    # a config that names an id whose module is gone is refused, and the context goes on
    cfg_obj = G.render_configuration(cm_third, X_FAR, G.ThinDisc(3.0, 400.0), 2000.0, image_width=32, image_height=32,
                                     alpha_lims=(-60, 60), beta_lims=(-35, 35), ensemble=ens)
    cfg, pl = cfg_obj.abi_config(), cfg_obj.abi_plane()
    gone = cfg.metric_id
    cm_third.unload()
    pts = np.zeros(32 * 32, dtype=_lib.POINT_DTYPE)
    rg, st = _lib.gr_range(0, 1024, 1024, 1), _lib.gr_stats()
    rc = L.gr_render_endpoints(ens.ctx.handle, C.byref(cfg), C.byref(pl), C.byref(rg), pts.ctypes.data, C.byref(st))
    assert rc == -2 and str(gone).encode() in L.gr_last_error()
    assert _image(G, ens, kerr).tobytes() == fused.tobytes()
    assert _image(G, ens, cm_bump).tobytes() == solo["bump"].tobytes()


def test_compiled_metric_over_two_contexts(G, ens, cm_bump):
    two = G.EnsembleMI355X(devices=[0, 0])
    pf = G.ConstPointFunctions.redshift(cm_bump, X_FAR, ensemble=ens) @ G.ConstPointFunctions.filter_intersected()
    kw = dict(image_width=128, image_height=96, alpha_lims=(-60, 60), beta_lims=(-35, 35), pf=pf)
    d = G.ThinDisc(cm_bump.isco(), 50.0)
    _, _, ref = G.rendergeodesics(cm_bump, X_FAR, d, 2000.0, ensemble=ens, **kw)
    _, _, img = G.rendergeodesics(cm_bump, X_FAR, d, 2000.0, ensemble=two, **kw)
    assert np.isfinite(ref).sum() > 500 and img.tobytes() == ref.tobytes()


def test_what_a_compiled_metric_refuses(G, ens, cm_bump):
    from gradus_jl_amd import _lib

    L = _lib.load()
    ens.set("precision", 32)
    with pytest.raises(_lib.GradusMI355XError) as e:
        _image(G, ens, cm_bump)
    assert e.value.code == -2 and "fp32" in str(e.value)
    ens.set("precision", 64)
    # the registry has 16 slots: fill what is free, the next one is refused, and nothing that was loaded has moved
    path = cm_bump.compile().encode()
    mine, rc = [], 0
    for _ in range(17):
        mid = C.c_int64(-1)
        rc = L.gr_metric_module_load(path, C.byref(mid))
        if rc != 0:
            break
        mine.append(mid.value)
    assert rc == -2 and b"slots" in L.gr_last_error() and 1 <= len(mine) <= 16
    for mid in mine:
        assert L.gr_metric_module_unload(mid) == 0
    res = cm_bump.resources
    assert set(res) == {"trace_lane", "trace_persistent", "tangent", "tangent_pairs"}
    assert all(0 < r["vgprs"] <= 512 and r["scratch_bytes"] >= 0 for r in res.values()), res
    print("  resources of the bump module:", res)
