"""ONE host thread, SEVERAL devices: the *_multi entry points of include/gradus_mi355x.h (ABI 6).

The GPU box has one MI355X, so the contexts of these tests live on the same device -- which exercises everything the
call does on the host (the deal of the rays, per-context staging, the order of enqueues, copies and waits, the
kernels' stores at global indices into one pinned block) and leaves only the physical concurrency of distinct devices
untested (tests/test_gpu_parity.py::test_multi_device_render_on_distinct_devices runs where there are two).

Two properties are asserted for every entry point of the boundary (src/tracing/tracing.jl:151-196 and its callers):
  * the bytes equal those of the one-context entry point, for 1, 2 and 4 contexts, into pageable AND into
    library-pinned results;
  * the enqueue phase does not wait for a device: gr_stats.enqueue_ms of every context is a small fraction of the
    kernels' time ("What's missing" 1b: a D2H copy into pageable memory inside the enqueue loop would run the
    devices one after another).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_FAR = np.array([0.0, 1000.0, math.radians(75), 0.0])
ALIMS, BLIMS = (-60.0, 60.0), (-35.0, 35.0)


@pytest.fixture(scope="module")
def multi4(G):
    return G.EnsembleMI355X(devices=[0, 0, 0, 0])


def _ctxs(ens, n):
    from gradus_jl_amd import _lib

    return _lib.ctx_array(ens.contexts[:n])


def _render_config(G, ens, W, H, metric=None, disc="isco"):
    from gradus_jl_amd.rendering import render_configuration

    m = metric or G.KerrMetric(1.0, 0.998)
    d = G.ThinDisc(m.isco(), 50.0) if disc == "isco" else disc
    return m, render_configuration(m, X_FAR, d, 2000.0, image_width=W, image_height=H, alpha_lims=ALIMS, beta_lims=BLIMS,
                                   ensemble=ens)


def _dest(L, ctx, nbytes, pinned):
    """(array of nbytes uint8, keep-alive): pageable numpy memory or a gr_host_alloc block"""
    from gradus_jl_amd import _lib

    if pinned:
        return _lib.PinnedBlock(ctx, nbytes).array(np.uint8, nbytes)
    return np.zeros(nbytes, dtype=np.uint8)


@pytest.mark.parametrize("pinned", [False, True])
def test_fused_render_multi_equals_one_context(G, ens, multi4, pinned):
    """gr_render_multi for 1 / 2 / 4 contexts == gr_render, into pageable memory (strided copies home in phase 2) and
    into a pinned block (every kernel stores its pixels at their place in the whole image: Cold.out_global)."""
    from gradus_jl_amd import _lib
    from gradus_jl_amd.rendering import abi_pointfunction

    L = _lib.load()
    W, H = 256, 160
    m, config = _render_config(G, ens, W, H)
    pf = G.ConstPointFunctions.redshift(m, X_FAR) @ G.ConstPointFunctions.filter_intersected()
    cfg, pl = config.abi_config(), config.abi_plane()
    s, keep = abi_pointfunction(pf)
    n = W * H
    ref = np.zeros(n)
    st = _lib.gr_stats()
    rg = _lib.gr_range(0, n, n, 1)
    _lib.check(L.gr_render(ens.ctx.handle, C.byref(cfg), C.byref(pl), C.byref(s), C.byref(rg), ref.ctypes.data, C.byref(st)))
    assert np.isfinite(ref).sum() > n // 10
    for k in (1, 2, 4):
        arr, sts = _ctxs(multi4, k)
        raw = _dest(L, multi4.ctx, 8 * n, pinned)
        raw[:] = 0xFF
        _lib.check(L.gr_render_multi(arr, k, C.byref(cfg), C.byref(pl), C.byref(s), 0, raw.ctypes.data, sts))
        assert raw.tobytes() == ref.tobytes(), f"{k} contexts, pinned={pinned}"
        assert sum(x.rays for x in sts) == n and all(x.rays == n // k for x in sts)
        assert all(x.enqueue_ms > 0.0 for x in sts)


@pytest.mark.parametrize("pinned", [False, True])
def test_endpoints_multi_equals_one_context(G, ens, multi4, pinned):
    """gr_render_endpoints_multi (prerendergeodesics / the generic boundary on the render closure) == gr_render_endpoints."""
    from gradus_jl_amd import _lib

    L = _lib.load()
    W, H = 256, 96
    m, config = _render_config(G, ens, W, H)
    cfg, pl = config.abi_config(), config.abi_plane()
    n = W * H
    ref = np.zeros(n, dtype=_lib.POINT_DTYPE)
    st = _lib.gr_stats()
    rg = _lib.gr_range(0, n, n, 1)
    _lib.check(L.gr_render_endpoints(ens.ctx.handle, C.byref(cfg), C.byref(pl), C.byref(rg), ref.ctypes.data, C.byref(st)))
    assert (ref["status"] == 2).sum() > n // 10
    for k in (1, 2, 4):
        arr, sts = _ctxs(multi4, k)
        raw = _dest(L, multi4.ctx, 152 * n, pinned)
        raw[:] = 0xFF
        _lib.check(L.gr_render_endpoints_multi(arr, k, C.byref(cfg), C.byref(pl), 0, raw.ctypes.data, sts))
        got = raw.view(_lib.POINT_DTYPE)
        for f in _lib.POINT_DTYPE.names:          # field by field: the 4 padding bytes' twin (flags) is a field too
            assert np.array_equal(got[f], ref[f]), (k, pinned, f)
        assert sum(x.rays for x in sts) == n
    # the Python boundary takes the same route
    pts = G.rendering.prerendergeodesics(m, X_FAR, G.ThinDisc(m.isco(), 50.0), 2000.0, image_width=W, image_height=H,
                                         alpha_lims=ALIMS, beta_lims=BLIMS, ensemble=multi4)[2].points
    assert np.array_equal(np.ascontiguousarray(pts.T).ravel()["x"], ref["x"])


def test_trace_and_rayset_multi_equal_one_context(G, ens, multi4):
    """tracegeodesics on (x, v) arrays and on impact-parameter ray sets, and the per-ray summaries the precision solvers
    read: contiguous shares over 1 / 2 / 3 / 4 contexts give the bytes of the one-context call (n not a multiple of 64,
    so the last share is short and, with 4 contexts, shares differ)."""
    from gradus_jl_amd import _lib
    from gradus_jl_amd.rendering import abi_pointfunction
    from gradus_jl_amd.tracing import map_impact_parameters, tracing_configuration

    L = _lib.load()
    m = G.KerrMetric(1.0, 0.9)
    d = G.ThinDisc(m.isco(), 40.0)
    x = np.array([0.0, 500.0, math.radians(60), 0.0])
    rng = np.random.default_rng(11)
    n = 1000
    al, be = rng.uniform(-30, 30, n), rng.uniform(-20, 20, n)
    v = np.stack([map_impact_parameters(m, x, a, b) for a, b in zip(al, be)])
    config = tracing_configuration(m, x, v, d, (0.0, 1000.0), ensemble=ens)
    cfg = config.abi_config()
    ref = np.zeros(n, dtype=_lib.POINT_DTYPE)
    st = _lib.gr_stats()
    _lib.check(L.gr_trace_endpoints(ens.ctx.handle, C.byref(cfg), x.ctypes.data, 0, v.ctypes.data, n, ref.ctypes.data, C.byref(st)))
    assert (ref["status"] == 2).sum() > 100
    for k in (1, 2, 3, 4):
        arr, sts = _ctxs(multi4, k)
        got = np.zeros(n, dtype=_lib.POINT_DTYPE)
        _lib.check(L.gr_trace_endpoints_multi(arr, k, C.byref(cfg), x.ctypes.data, 0, v.ctypes.data, n, got.ctypes.data, sts))
        for f in _lib.POINT_DTYPE.names:
            assert np.array_equal(got[f], ref[f]), (k, f)
        assert sum(s.rays for s in sts) == n
    # per-ray positions (x_stride = 4)
    xs = np.repeat(x[None, :], n, axis=0).copy()
    arr, sts = _ctxs(multi4, 3)
    got = np.zeros(n, dtype=_lib.POINT_DTYPE)
    _lib.check(L.gr_trace_endpoints_multi(arr, 3, C.byref(cfg), xs.ctypes.data, 4, v.ctypes.data, n, got.ctypes.data, sts))
    assert np.array_equal(got["x"], ref["x"]) and np.array_equal(got["status"], ref["status"])
    # the Python boundary
    got = G.tracegeodesics(m, x, v, d, (0.0, 1000.0), ensemble=multi4)
    assert np.array_equal(got["v"], ref["v"])

    # ---- impact-parameter ray sets
    from gradus_jl_amd.tracing import lnr_momentum_to_global_velocity_matrix

    rs = _lib.gr_rayset()
    Mx = lnr_momentum_to_global_velocity_matrix(m, x)
    for i in range(4):
        rs.x_obs[i] = float(x[i])
        for q in range(4):
            rs.Mx[4 * i + q] = float(Mx[i, q])
    al, be = np.ascontiguousarray(al), np.ascontiguousarray(be)
    rs.alpha, rs.beta, rs.n = al.ctypes.data, be.ctypes.data, n
    pf, keep = abi_pointfunction(G.ConstPointFunctions.redshift(m, x))
    ref_pts = np.zeros(n, dtype=_lib.POINT_DTYPE)
    _lib.check(L.gr_rayset_endpoints(ens.ctx.handle, C.byref(cfg), C.byref(rs), ref_pts.ctypes.data, C.byref(st)))
    ref_sum = np.zeros((n, 4))
    _lib.check(L.gr_ray_summary(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), ref_sum.ctypes.data, C.byref(st)))
    ref_tan = np.zeros((n, 8))
    _lib.check(L.gr_ray_tangent(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), ref_tan.ctypes.data, C.byref(st)))
    ref_gr = np.zeros((n, 2))
    _lib.check(L.gr_redshift_radius(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), m.isco(), 40.0, ref_gr.ctypes.data,
                                    C.byref(st)))
    for k in (2, 4):
        arr, sts = _ctxs(multi4, k)
        got = np.zeros(n, dtype=_lib.POINT_DTYPE)
        _lib.check(L.gr_rayset_endpoints_multi(arr, k, C.byref(cfg), C.byref(rs), got.ctypes.data, sts))
        assert np.array_equal(got["x"], ref_pts["x"]) and np.array_equal(got["lambda_max"], ref_pts["lambda_max"])
        o = np.zeros((n, 4))
        _lib.check(L.gr_ray_summary_multi(arr, k, C.byref(cfg), C.byref(rs), C.byref(pf), o.ctypes.data, sts))
        assert o.tobytes() == ref_sum.tobytes()
        o = np.zeros((n, 8))
        _lib.check(L.gr_ray_tangent_multi(arr, k, C.byref(cfg), C.byref(rs), C.byref(pf), o.ctypes.data, sts))
        assert o.tobytes() == ref_tan.tobytes()
        o = np.zeros((n, 2))
        _lib.check(L.gr_redshift_radius_multi(arr, k, C.byref(cfg), C.byref(rs), C.byref(pf), m.isco(), 40.0, o.ctypes.data, sts))
        assert o.tobytes() == ref_gr.tobytes()
    # a separable plane in ray order (tracegeodesics(m, x, plane, ...)): shares are ranges of sep_first
    plane = G.PolarPlane(G.GeometricGrid(), Nr=37, Nθ=29, r_min=1.0, r_max=40.0)
    one = G.tracegeodesics(m, x, plane, d, (0.0, 1000.0), ensemble=ens)
    many = G.tracegeodesics(m, x, plane, d, (0.0, 1000.0), ensemble=multi4)
    assert one.size == 37 * 29 and np.array_equal(one["x"], many["x"]) and np.array_equal(one["status"], many["status"])


def test_lineprofile_multi_equals_one_context(G, ens, multi4):
    """gr_lineprofile_multi: the rays of a PolarPlane dealt block-cyclically (strips of 8 x 8 tiles), one histogram per
    context, added on the host.  Every ray is binned exactly once (the counters add up) and the histogram equals the
    one-context one to rounding (the order in which a bin receives its rays differs, as between any two launches)."""
    from gradus_jl_amd import _lib

    m = G.KerrMetric(1.0, 0.998)
    d = G.ThinDisc(m.isco(), 120.0)
    u = np.array([0.0, 1000.0, math.radians(60), 0.0])
    bins = np.linspace(0.1, 1.5, 180)
    for (nr, nt) in ((256, 256), (100, 61)):          # whole tiles / ragged edges
        plane = G.PolarPlane(G.GeometricGrid(), Nr=nr, Nθ=nt, r_min=1.0, r_max=120.0)
        kw = dict(plane=plane, maxrₑ=100.0, stats=True)
        _, f1, s1 = G.lineprofile(bins, G.PowerLawEmissivity(3.0), m, u, d, G.BinningMethod(), ensemble=ens, **kw)
        _, f4, s4 = G.lineprofile(bins, G.PowerLawEmissivity(3.0), m, u, d, G.BinningMethod(), ensemble=multi4, **kw)
        assert s4["rays"] == s1["rays"] == nr * nt
        assert s4["status_count"] == s1["status_count"] and s4["accepted_steps"] == s1["accepted_steps"]
        assert f1.sum() == pytest.approx(1.0, abs=1e-12)
        np.testing.assert_allclose(f4, f1, rtol=1e-11, atol=1e-15)
    # ray arrays instead of a separable plane: contiguous shares
    import os

    os.environ["GRADUS_MI355X_SEPARABLE_RAYS"] = "0"
    try:
        _, g1 = G.lineprofile(bins, G.PowerLawEmissivity(3.0), m, u, d, G.BinningMethod(), ensemble=ens, plane=plane, maxrₑ=100.0)
        _, g4 = G.lineprofile(bins, G.PowerLawEmissivity(3.0), m, u, d, G.BinningMethod(), ensemble=multi4, plane=plane, maxrₑ=100.0)
    finally:
        del os.environ["GRADUS_MI355X_SEPARABLE_RAYS"]
    np.testing.assert_allclose(g4, g1, rtol=1e-11, atol=1e-15)
    np.testing.assert_allclose(g1, f1, rtol=1e-11, atol=1e-15)


def test_transfer_function_through_a_multi_ensemble(G, ens, multi4):
    """The Cunningham transfer function's launches (gr_ray_tangent / gr_ray_summary on a few hundred rays each) through an
    ensemble of four contexts: the same numbers as on one (contiguous shares, same kernels, same bytes per ray)."""
    m = G.KerrMetric(1.0, 0.998)
    x = np.array([0.0, 100_000.0, math.radians(60), 0.0])
    kw = dict(N=40, chart=G.chart_for_metric(m, 2 * x[1], closest_approach=1.005))
    one = G.cunningham_transfer_function(m, x, G.ThinDisc(0.0, float("inf")), 7.0, ensemble=ens, **kw)
    many = G.cunningham_transfer_function(m, x, G.ThinDisc(0.0, float("inf")), 7.0, ensemble=multi4, **kw)
    assert one.f.size == many.f.size and np.all(np.isfinite(one.f))
    assert many.f.tobytes() == one.f.tobytes() and many.g_star.tobytes() == one.g_star.tobytes()


def test_multi_argument_errors(G, ens, multi4):
    from gradus_jl_amd import _lib
    from gradus_jl_amd.tracing import separable_rayset, tracing_configuration

    L = _lib.load()
    m, config = _render_config(G, ens, 64, 64)
    cfg, pl = config.abi_config(), config.abi_plane()
    h = multi4.contexts[0].handle
    twice = (C.c_void_p * 2)(h, h)
    out = np.zeros(64 * 64, dtype=_lib.POINT_DTYPE)
    assert L.gr_render_endpoints_multi(twice, 2, C.byref(cfg), C.byref(pl), 0, out.ctypes.data, None) == -1
    assert b"twice" in L.gr_last_error()
    arr, sts = _ctxs(multi4, 3)
    assert L.gr_render_endpoints_multi(arr, 3, C.byref(cfg), C.byref(pl), 0, out.ctypes.data, sts) == -1      # 64 columns over 3
    # per-ray outputs of a TILED separable set have no ray order to share out
    plane = G.PolarPlane(G.GeometricGrid(), Nr=16, Nθ=16, r_min=1.0, r_max=40.0)
    rs, keep = separable_rayset(m, X_FAR, plane, tiled=True)
    pts = np.zeros(256, dtype=_lib.POINT_DTYPE)
    arr, sts = _ctxs(multi4, 2)
    assert L.gr_rayset_endpoints_multi(arr, 2, C.byref(cfg), C.byref(rs), pts.ctypes.data, sts) == -1
    assert b"ray order" in L.gr_last_error()
    # nothing was left in flight: the contexts still work
    rs, keep = separable_rayset(m, X_FAR, plane, tiled=False)
    assert L.gr_rayset_endpoints_multi(arr, 2, C.byref(cfg), C.byref(rs), pts.ctypes.data, sts) == 0
    assert sum(s.rays for s in sts) == 256


GOLDEN_TILED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rayset_endpoints_tiled_16x16.npy")


def test_one_context_call_is_its_multi_form_on_one_context(G, ens, multi4):
    """The one-context entry points ARE their *_multi forms with n = 1: the same bytes and the same counters from both, for
    gr_ray_summary, gr_rayset_endpoints, gr_sky_cells and gr_plane_cells on 3001 rays / cells (no multiple of 64) and on a TILED
    separable set -- which has no ray order to share out, so two contexts refuse it, and which one context takes as it is given:
    its rows are the ones recorded before the two forms became one (tests/golden).  Only enqueue_ms tells the forms apart."""
    import skycell_scene as S
    from gradus_jl_amd import _lib
    from gradus_jl_amd.rendering import abi_pointfunction
    from gradus_jl_amd.tracing import lnr_momentum_to_global_velocity_matrix, separable_rayset

    L = _lib.load()
    h = ens.ctx.handle
    one_ctx = (C.c_void_p * 1)(h)
    m, config = _render_config(G, ens, 64, 64)
    cfg = config.abi_config()
    pf, keep_pf = abi_pointfunction(G.ConstPointFunctions.redshift(m, X_FAR))

    def both(what, single, multi, out, pinned=False):
        """single(out, stats) and multi(ctxs, 1, out, stats) -> the bytes both wrote (into pageable memory or gr_host_alloc blocks)"""
        st, sts = _lib.gr_stats(), (_lib.gr_stats * 1)()
        st.enqueue_ms = -1.0
        a, b = _dest(L, ens.ctx, out.size, pinned), _dest(L, ens.ctx, out.size, pinned)
        a[:] = 0xFF
        b[:] = 0xFF
        _lib.check(single(a.ctypes.data, C.byref(st)))
        _lib.check(multi(one_ctx, 1, b.ctypes.data, sts))
        assert a.tobytes() == b.tobytes(), what
        for f in ("rays", "accepted_steps", "rejected_steps"):
            assert getattr(st, f) == getattr(sts[0], f), (what, f)
        assert list(st.status_count) == list(sts[0].status_count) and st.accepted_steps > 0, what
        assert st.enqueue_ms == 0.0 and sts[0].enqueue_ms > 0.0, (what, st.enqueue_ms, sts[0].enqueue_ms)
        assert st.kernel_ms > 0.0 and st.call_ms >= st.kernel_ms, what
        return st, a

    n = 3001
    rng = np.random.default_rng(5)
    al, be = np.ascontiguousarray(rng.uniform(-30, 30, n)), np.ascontiguousarray(rng.uniform(-20, 20, n))
    rs = _lib.gr_rayset()
    Mx = lnr_momentum_to_global_velocity_matrix(m, X_FAR)
    for i in range(4):
        rs.x_obs[i] = float(X_FAR[i])
        for q in range(4):
            rs.Mx[4 * i + q] = float(Mx[i, q])
    rs.alpha, rs.beta, rs.n = al.ctypes.data, be.ctypes.data, n
    plane = G.PolarPlane(G.GeometricGrid(), Nr=16, Nθ=16, r_min=1.0, r_max=40.0)
    tiled, keep_tiled = separable_rayset(m, X_FAR, plane, tiled=True)
    for what, q in (("arrays", rs), ("tiled", tiled)):
        st, _ = both(f"gr_ray_summary {what}",
                     lambda o, s: L.gr_ray_summary(h, C.byref(cfg), C.byref(q), C.byref(pf), o, s),
                     lambda a, k, o, s: L.gr_ray_summary_multi(a, k, C.byref(cfg), C.byref(q), C.byref(pf), o, s),
                     np.zeros(32 * q.n, dtype=np.uint8))
        assert st.rays == q.n
        st, pts = both(f"gr_rayset_endpoints {what}",
                       lambda o, s: L.gr_rayset_endpoints(h, C.byref(cfg), C.byref(q), o, s),
                       lambda a, k, o, s: L.gr_rayset_endpoints_multi(a, k, C.byref(cfg), C.byref(q), o, s),
                       np.zeros(152 * q.n, dtype=np.uint8))
        assert st.rays == q.n
    assert (pts.view(_lib.POINT_DTYPE)["status"] == 2).sum() > 20
    assert pts.tobytes() == np.load(GOLDEN_TILED).tobytes()
    # ... and sharing the tiled set out is still refused
    arr, sts = _ctxs(multi4, 2)
    assert L.gr_rayset_endpoints_multi(arr, 2, C.byref(cfg), C.byref(tiled), pts.ctypes.data, sts) == -1
    assert b"ray order" in L.gr_last_error()

    # cells of a source's sky
    su = S.setup(G, S.KERR, None, ensemble=ens)
    cosθ, ϕ = np.ascontiguousarray(rng.uniform(-0.95, 0.95, n)), np.ascontiguousarray(rng.uniform(-math.pi, math.pi, n))
    cells = S.skycells_struct(G, su, cosθ, ϕ)
    st, _ = both("gr_sky_cells",
                 lambda o, s: L.gr_sky_cells(h, C.byref(su["cfg"]), C.byref(cells), C.byref(su["pf"]), o, s),
                 lambda a, k, o, s: L.gr_sky_cells_multi(a, k, C.byref(su["cfg"]), C.byref(cells), C.byref(su["pf"]), o, s),
                 np.zeros(48 * n, dtype=np.uint8))
    assert st.rays == n
    # cells of an observer's plane
    pl = config.abi_plane()
    st, _ = both("gr_plane_cells",
                 lambda o, s: L.gr_plane_cells(h, C.byref(cfg), C.byref(pl), al.ctypes.data, be.ctypes.data, n, o, s),
                 lambda a, k, o, s: L.gr_plane_cells_multi(a, k, C.byref(cfg), C.byref(pl), al.ctypes.data, be.ctypes.data, n, o, s),
                 np.zeros(152 * n, dtype=np.uint8))
    assert st.rays == n

    # the image plane: pixels and end-point records, into pageable memory and into a block the library pinned; the bytes are
    # those of the *_device entry points.  64 columns are dealt in blocks of 8; 68 in blocks of 4 to one context and of 1 to
    # four, and 44 rows leave a ragged last row of tiles.
    for W, H in ((64, 64), (68, 44)):
        ref = _plane_reference(G, ens, W, H)
        pcfg, ppl = ref["config"].abi_config(), ref["config"].abi_plane()
        s, keep_s = abi_pointfunction(ref["pf"])
        n_px = W * H
        rg = _lib.gr_range(0, n_px, n_px, 1)
        for pinned in (False, True):
            st, img = both(f"gr_render {W}x{H} pinned={pinned}",
                           lambda o, q: L.gr_render(h, C.byref(pcfg), C.byref(ppl), C.byref(s), C.byref(rg), o, q),
                           lambda a, k, o, q: L.gr_render_multi(a, k, C.byref(pcfg), C.byref(ppl), C.byref(s), 0, o, q),
                           ref["image"], pinned)
            assert img.tobytes() == ref["image"].tobytes() and st.rays == n_px, (W, H, pinned)
            st, pts = both(f"gr_render_endpoints {W}x{H} pinned={pinned}",
                           lambda o, q: L.gr_render_endpoints(h, C.byref(pcfg), C.byref(ppl), C.byref(rg), o, q),
                           lambda a, k, o, q: L.gr_render_endpoints_multi(a, k, C.byref(pcfg), C.byref(ppl), 0, o, q),
                           ref["points"], pinned)
            assert pts.tobytes() == ref["points"].tobytes() and st.rays == n_px, (W, H, pinned)
            arr, sts = _ctxs(multi4, 4)
            raw = _dest(L, multi4.ctx, 8 * n_px, pinned)
            raw[:] = 0xFF
            _lib.check(L.gr_render_multi(arr, 4, C.byref(pcfg), C.byref(ppl), C.byref(s), 0, raw.ctypes.data, sts))
            assert raw.tobytes() == ref["image"].tobytes() and sum(x.rays for x in sts) == n_px, (W, H, pinned)
            raw = _dest(L, multi4.ctx, 152 * n_px, pinned)
            raw[:] = 0xFF
            _lib.check(L.gr_render_endpoints_multi(arr, 4, C.byref(pcfg), C.byref(ppl), 0, raw.ctypes.data, sts))
            assert raw.tobytes() == ref["points"].tobytes() and sum(x.rays for x in sts) == n_px, (W, H, pinned)


_PLANE_REFERENCE = {}


def _plane_reference(G, ens, W, H):
    """The whole W x H plane from gr_render_device and gr_render_endpoints_device into torch memory, copied to the host: the
    image's and the records' bytes (read-only uint8 arrays) and the counters of the two launches.  The host-buffer calls are
    compared with this, never with one another alone."""
    if (W, H) not in _PLANE_REFERENCE:
        import torch
        from gradus_jl_amd import device as gdev

        m, config = _render_config(G, ens, W, H)
        pf = G.ConstPointFunctions.redshift(m, X_FAR) @ G.ConstPointFunctions.filter_intersected()
        dev = torch.device("cuda", 0)
        img = torch.empty(W * H, dtype=torch.float64, device=dev)
        raw = torch.empty(152 * W * H, dtype=torch.uint8, device=dev)
        st_img, st_pts = gdev.new_stats(dev), gdev.new_stats(dev)
        gdev.render_device(config, pf, img, stats=st_img)
        gdev.render_endpoints_device(config, raw, stats=st_pts)
        torch.cuda.synchronize()
        image, points = img.cpu().numpy().view(np.uint8), raw.cpu().numpy()
        image.setflags(write=False)
        points.setflags(write=False)
        assert np.isfinite(image.view(np.float64)).sum() > W * H // 10
        _PLANE_REFERENCE[(W, H)] = {"config": config, "pf": pf, "image": image, "points": points,
                                    "image_stats": gdev.stats_dict(st_img), "points_stats": gdev.stats_dict(st_pts)}
    return _PLANE_REFERENCE[(W, H)]


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("W,H", [(64, 64), (68, 44)])
def test_one_context_renders_of_a_part_of_the_plane(G, ens, W, H, pinned):
    """gr_render and gr_render_endpoints on one context and a range that is not the whole plane write that range's rows, in
    the range's order, to the start of the caller's buffer: a contiguous range of whole 8-column strips (the shape a banded
    return takes) and the two strided halves of a deal over two (rays k block ... of every second block).  The rows are the
    matching ones of the whole plane from the *_device entry points."""
    from gradus_jl_amd import _lib
    from gradus_jl_amd.rendering import abi_pointfunction

    L = _lib.load()
    h = ens.ctx.handle
    ref = _plane_reference(G, ens, W, H)
    cfg, pl = ref["config"].abi_config(), ref["config"].abi_plane()
    s, keep_s = abi_pointfunction(ref["pf"])
    bc = 8
    while W % (2 * bc):
        bc //= 2
    block = bc * H
    ranges = [("strips", _lib.gr_range(8 * H, 16 * H, 16 * H, 1), np.arange(8 * H, 24 * H))]
    for k in (0, 1):
        rows = np.arange(W * H).reshape(-1, block)[k::2].ravel()
        ranges.append((f"every second block from {k}", _lib.gr_range(k * block, rows.size, block, 2), rows))
    for what, rg, rows in ranges:
        st = _lib.gr_stats()
        raw = _dest(L, ens.ctx, 8 * rows.size, pinned)
        raw[:] = 0xFF
        _lib.check(L.gr_render(h, C.byref(cfg), C.byref(pl), C.byref(s), C.byref(rg), raw.ctypes.data, C.byref(st)))
        assert raw.tobytes() == ref["image"].reshape(-1, 8)[rows].tobytes(), (what, "gr_render")
        assert st.rays == rows.size and st.enqueue_ms == 0.0
        raw = _dest(L, ens.ctx, 152 * rows.size, pinned)
        raw[:] = 0xFF
        _lib.check(L.gr_render_endpoints(h, C.byref(cfg), C.byref(pl), C.byref(rg), raw.ctypes.data, C.byref(st)))
        assert raw.tobytes() == ref["points"].reshape(-1, 152)[rows].tobytes(), (what, "gr_render_endpoints")
        assert st.rays == rows.size and st.enqueue_ms == 0.0


@pytest.mark.parametrize("pinned", [False, True])
def test_a_refused_render_leaves_the_context_as_it_was(G, ens, pinned):
    """gr_render_endpoints refuses a range that reaches past the image only once the call has begun on the context (the plane
    is checked where the launch is prepared).  Nothing of the refused call stays behind: the next call on the same context
    returns the plane's records and the counters of one call -- those of the *_device launch of the same plane."""
    from gradus_jl_amd import _lib

    L = _lib.load()
    h = ens.ctx.handle
    W, H = 68, 44
    n = W * H
    ref = _plane_reference(G, ens, W, H)
    cfg, pl = ref["config"].abi_config(), ref["config"].abi_plane()
    raw = _dest(L, ens.ctx, 152 * (n + 64), pinned)
    raw[:] = 0xFF
    st = _lib.gr_stats()
    too_long = _lib.gr_range(0, n + 64, n + 64, 1)
    assert L.gr_render_endpoints(h, C.byref(cfg), C.byref(pl), C.byref(too_long), raw.ctypes.data, C.byref(st)) == -1      # GR_ERR_INVALID_ARGUMENT
    assert L.gr_last_error()
    assert (raw == 0xFF).all()
    rg = _lib.gr_range(0, n, n, 1)
    _lib.check(L.gr_render_endpoints(h, C.byref(cfg), C.byref(pl), C.byref(rg), raw.ctypes.data, C.byref(st)))
    assert raw[:152 * n].tobytes() == ref["points"].tobytes() and (raw[152 * n:] == 0xFF).all()
    want = ref["points_stats"]
    assert st.rays == n == want["rays"]
    assert (st.accepted_steps, st.rejected_steps) == (want["accepted_steps"], want["rejected_steps"])
    assert list(st.status_count) == want["status_count"]
    assert st.enqueue_ms == 0.0 and st.kernel_ms > 0.0 and st.call_ms >= st.kernel_ms


@pytest.mark.parametrize("pinned", [False, True])
def test_enqueue_phase_does_not_wait_for_a_device(G, ens, multi4, pinned):
    """VERDICT r3 1(b).  Four contexts, a 2048² fused render and a 1024² end-point render: the host time each context's
    enqueue took is a small fraction of the kernels' time, into pageable memory (whose copies are queued only after
    EVERY kernel has been launched) and into pinned memory (no copies at all).  Were a blocking copy part of the
    enqueue loop, enqueue_ms of context 0 would be about its kernel's duration."""
    from gradus_jl_amd import _lib
    from gradus_jl_amd.rendering import abi_pointfunction

    L = _lib.load()
    k = 4
    arr, sts = _ctxs(multi4, k)
    report = {}
    for what, (W, H) in (("image", (2048, 2048)), ("endpoints", (1024, 1024))):
        m, config = _render_config(G, ens, W, H)
        cfg, pl = config.abi_config(), config.abi_plane()
        n = W * H
        pf = G.ConstPointFunctions.redshift(m, X_FAR) @ G.ConstPointFunctions.filter_intersected()
        s, keep = abi_pointfunction(pf)
        raw = _dest(L, multi4.ctx, (8 if what == "image" else 152) * n, pinned)
        for rep in range(2):          # the first call allocates scratch and loads code objects
            if what == "image":
                _lib.check(L.gr_render_multi(arr, k, C.byref(cfg), C.byref(pl), C.byref(s), 0, raw.ctypes.data, sts))
            else:
                _lib.check(L.gr_render_endpoints_multi(arr, k, C.byref(cfg), C.byref(pl), 0, raw.ctypes.data, sts))
        enq = [x.enqueue_ms for x in sts]
        ker = [x.kernel_ms for x in sts]
        call = [x.call_ms for x in sts]
        report[what] = (enq, ker, call)
        print(f"  {what} pinned={pinned}: enqueue_ms {['%.3f' % e for e in enq]} kernel_ms {['%.2f' % q for q in ker]} "
              f"call_ms {['%.2f' % q for q in call]}")
        assert max(enq) < 0.1 * max(ker), (what, enq, ker)
        assert sum(enq) < 0.25 * max(ker), (what, enq, ker)
        assert sum(x.rays for x in sts) == n


def test_image_width_not_divisible_by_the_number_of_devices(G, ens):
    """three contexts and a 64-wide image -- the library deals whole columns and refuses 64 / 3; the host side takes
    the largest leading subset of the ensemble that divides the width (here two) instead of raising, for the fused render
    and for the end points, and the pixels / records are those of one context."""
    m = G.KerrMetric(1.0, 0.998)
    d = G.ThinDisc(m.isco(), 50.0)
    three = G.EnsembleMI355X(devices=[0, 0, 0])
    assert len(three.contexts_for_width(64)) == 2 and len(three.contexts_for_width(63)) == 3 and len(three.contexts_for_width(61)) == 1
    pf = G.ConstPointFunctions.redshift(m, X_FAR) @ G.ConstPointFunctions.filter_intersected()
    kw = dict(image_width=64, image_height=64, alpha_lims=ALIMS, beta_lims=BLIMS)
    _, _, one = G.rendergeodesics(m, X_FAR, d, 2000.0, pf=pf, ensemble=ens, **kw)
    _, _, many = G.rendergeodesics(m, X_FAR, d, 2000.0, pf=pf, ensemble=three, **kw)
    assert one.tobytes() == many.tobytes()
    _, _, c1 = G.prerendergeodesics(m, X_FAR, d, 2000.0, ensemble=ens, **kw)
    _, _, c3 = G.prerendergeodesics(m, X_FAR, d, 2000.0, ensemble=three, **kw)
    assert np.asarray(c1.points).tobytes() == np.asarray(c3.points).tobytes()


def test_tabulated_metric_through_a_multi_ensemble(G, ens, multi4):
    """A user-defined metric (GR_METRIC_TABULATED) over several contexts: every context stages its own copy of the table; the
    fused image, the end points of a ray array and a corona's sky rays equal the one-context results bit for bit."""
    tab = G.TabulatedMetric(G.KerrMetric(1.0, 0.9))
    d = G.ThinDisc(tab.isco(), 50.0)
    pf = G.ConstPointFunctions.redshift(tab, X_FAR, ensemble=ens) @ G.ConstPointFunctions.filter_intersected()
    kw = dict(image_width=128, image_height=96, alpha_lims=ALIMS, beta_lims=BLIMS, pf=pf)
    _, _, ref = G.rendergeodesics(tab, X_FAR, d, 2000.0, ensemble=ens, **kw)
    _, _, img = G.rendergeodesics(tab, X_FAR, d, 2000.0, ensemble=multi4, **kw)
    assert np.isfinite(ref).sum() > 500 and img.tobytes() == ref.tobytes()
    rng = np.random.default_rng(3)
    vs = G.map_impact_parameters(tab, X_FAR, rng.uniform(-20, 20, 3001), rng.uniform(-12, 12, 3001))
    a = G.tracegeodesics(tab, X_FAR, vs, d, 2000.0, ensemble=ens)
    b = G.tracegeodesics(tab, X_FAR, vs, d, 2000.0, ensemble=multi4)
    assert a.tobytes() == b.tobytes()
    # a corona's sky source is one context's work: a multi ensemble uses its first context
    s = G.EvenSampler(G.BothHemispheres(), G.GoldenSpiralGenerator())
    p1 = G.emissivity_profile(tab, G.ThinDisc(0.0, 200.0), G.LampPostModel(h=8.0), sampler=s, n_samples=4000, N=20, ensemble=ens)
    p4 = G.emissivity_profile(tab, G.ThinDisc(0.0, 200.0), G.LampPostModel(h=8.0), sampler=s, n_samples=4000, N=20, ensemble=multi4)
    np.testing.assert_array_equal(p1.ε, p4.ε)
