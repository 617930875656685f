"""A corona's energy ratio on the device against rays the ORACLE traces (tests/corona_scene.py holds the sources, the reference
and the criteria; tests/test_corona_energy_host.py what was established on the CPU): the rows of gr_ray_summary for a moving source
at one position (pf->has_u_src) and for a source without one position (gr_rayset.sky_rows, k_sky_velocities / k_sky_scale_g), in
Kerr and in a metric that is not Kerr, inside the ISCO as well; launch edges; shares; the bins of gr_corona_bin as the reduction of
those rows; single precision; and what the library refuses."""
import ctypes as C

import numpy as np
import pytest

import corona_scene as S

pytestmark = pytest.mark.gpu

DISC_KERR = S.CASE["disc-kerr-corotating"]
N_DEALT = 16_641            # 4 chunks of 4096 samples and a fifth of 257: from 16 384 on gr_corona_trace deals its rays by cost


def summary(G, ens, cfg, rs, pf, n, guard=3):
    """gr_ray_summary into a buffer with `guard` rows behind the n the call may write; asserts those stay as they were."""
    from gradus_jl_amd import _lib

    buf = np.full((n + guard, 4), -7.0)
    _lib.check(_lib.load().gr_ray_summary(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), buf.ctypes.data, None))
    assert np.all(buf[n:] == -7.0)
    return buf[:n].copy()


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("case", S.CASES, ids=S.CASE_IDS)
def test_rows_equal_oracle_traced_rays_and_their_energy_ratio(G, ens, oracle, case, kernel):
    """(g, ρ, t, status) of every case through both kernels against the oracle's rays and numpy's energy_ratio -- the criteria of
    corona_scene.check: statuses, 1e-6 on every common hit outside AND inside the ISCO, the median of g below 1e-9."""
    rows = S.device_rows(G, oracle, case, S.N, ens, kernel=kernel)
    isco, _ = S.oracle_table(G, oracle, case)
    S.check(S.compare(rows, S.reference(G, oracle, case), isco), f"{case[0]}, kernel {kernel}")


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_launch_edges_of_a_source_with_rows(G, ens, oracle, n):
    """a partly filled wave, one wave and a ray, more than one workgroup of k_sky_velocities / k_sky_scale_g; every n is a sample
    set of its own (θ depends on n).  The single ray of n = 1 misses: its status, its NaN and its end point."""
    ens.set("kernel", 2).set("precision", 64)
    cfg, rs, pf, keep, _ = S.launch(G, oracle, DISC_KERR, n, ens)
    rows = summary(G, ens, cfg, rs, pf, n)
    ref = S.reference(G, oracle, DISC_KERR, n)
    st = rows[:, 3].astype(int)
    hit = (st == S.HIT) & (ref["status"] == S.HIT)
    print(f"n = {n}: statuses {np.bincount(st, minlength=4).tolist()}, oracle {np.bincount(ref['status'], minlength=4).tolist()}, common hits {hit.sum()}")
    assert np.sum(st != ref["status"]) <= (0 if n == 1 else S.MAX_STATUS_DIFF)
    assert np.all(np.isnan(rows[st != S.HIT, 0])) and np.all(np.isfinite(rows[st == S.HIT, 0]))
    if n == 1:
        assert st[0] != S.HIT and ref["status"][0] != S.HIT
        np.testing.assert_allclose(rows[0, 1:3], [ref["rho"][0], ref["t"][0]], rtol=S.RTOL)
        return
    assert hit.sum() >= n // 2
    np.testing.assert_allclose(rows[hit, 1], ref["rho"][hit], rtol=S.RTOL)
    np.testing.assert_allclose(rows[hit, 2], ref["t"][hit], rtol=S.RTOL)
    np.testing.assert_allclose(rows[hit, 0], ref["g"][hit], rtol=S.RTOL)


def test_no_samples_is_ok_and_writes_nothing(G, ens, oracle):
    ens.set("kernel", 2).set("precision", 64)
    cfg, rs, pf, keep, _ = S.launch(G, oracle, DISC_KERR, 4, ens)
    rs.n = 0
    assert summary(G, ens, cfg, rs, pf, 0).shape == (0, 4)
    lim, hits = np.full(2, -7.0), C.c_int64(-7)
    from gradus_jl_amd import _lib

    L = _lib.load()
    _lib.check(L.gr_corona_trace(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), lim.ctypes.data, C.byref(hits), None))
    assert hits.value == 0 and np.all(np.isnan(lim))


@pytest.fixture(scope="module")
def three(G, _ens_session):
    """three contexts on device 0: the session's and two of the module's own"""
    a, b = G.EnsembleMI355X(0), G.EnsembleMI355X(0)
    return [_ens_session.ctx, a.ctx, b.ctx], (a, b)


def test_shares_of_a_source_with_rows_give_the_same_bytes(G, ens, oracle, three):
    """1001 DiscCorona samples in one call, as three hand-made shares (sky_first / sky_total, sky_rows advanced by GR_SKY_ROW x
    sky_first; boundaries that are no multiple of a wave) and through gr_ray_summary_multi: the same bytes -- a share that read its
    neighbour's rows or numbered its samples from 1 would not give them; gr_corona_trace_multi + gr_corona_bin_multi: the bits of
    the one-context calls."""
    from gradus_jl_amd import _lib

    L = _lib.load()
    n = 1001
    ens.set("kernel", 2).set("precision", 64)
    cfg, rs, pf, keep, src = S.launch(G, oracle, DISC_KERR, n, ens)
    one = summary(G, ens, cfg, rs, pf, n)
    ref = S.reference(G, oracle, DISC_KERR, n)
    hit = (one[:, 3].astype(int) == S.HIT) & (ref["status"] == S.HIT)
    assert np.sum(one[:, 3].astype(int) != ref["status"]) <= S.MAX_STATUS_DIFF and hit.sum() > 500
    np.testing.assert_allclose(one[hit, 0], ref["g"][hit], rtol=S.RTOL)
    parts = []
    for first, stop in ((0, 333), (333, 700), (700, n)):
        share = type(rs).from_buffer_copy(rs)
        share.n, share.sky_first, share.sky_total = stop - first, first, n
        share.sky_rows = src.ctypes.data + 8 * 28 * first
        parts.append(summary(G, ens, cfg, share, pf, stop - first))
    assert np.concatenate(parts).tobytes() == one.tobytes()
    ctxs, _ = three
    arr, sts = _lib.ctx_array(ctxs)
    multi = np.full((n + 2, 4), -7.0)
    _lib.check(L.gr_ray_summary_multi(arr, 3, C.byref(cfg), C.byref(rs), C.byref(pf), multi.ctypes.data, sts))
    assert multi[:n].tobytes() == one.tobytes() and np.all(multi[n:] == -7.0)
    assert sum(x.rays for x in sts) == n and all(x.rays > 0 for x in sts)
    # the reductions: limits, hit count and integer bins of three contexts are those of one
    lim, hits, lim3, hits3 = np.zeros(2), C.c_int64(0), np.zeros(2), C.c_int64(0)
    _lib.check(L.gr_corona_trace(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), lim.ctypes.data, C.byref(hits), None))
    edges = np.ascontiguousarray(np.linspace(lim[0], lim[1], 32))
    bins1, bins3 = np.zeros((3, 32)), np.zeros((3, 32))
    _lib.check(L.gr_corona_bin(ens.ctx.handle, edges.ctypes.data, edges.size, bins1.ctypes.data))
    _lib.check(L.gr_corona_trace_multi(arr, 3, C.byref(cfg), C.byref(rs), C.byref(pf), lim3.ctypes.data, C.byref(hits3), sts))
    _lib.check(L.gr_corona_bin_multi(arr, 3, edges.ctypes.data, edges.size, bins3.ctypes.data))
    finite = np.isfinite(one[:, 0])
    assert hits.value == hits3.value == finite.sum()
    assert lim.tobytes() == lim3.tobytes() and lim[0] == one[finite, 1].min() and lim[1] == one[finite, 1].max()
    assert bins3.tobytes() == bins1.tobytes() and bins1[0].sum() == hits.value


@pytest.mark.parametrize("n", [S.N, N_DEALT])
@pytest.mark.parametrize("case", S.DISC_CASES[:2], ids=S.DISC_CASE_IDS[:2])
def test_bins_are_the_reduction_of_the_pinned_rows(G, ens, oracle, case, n):
    """gr_corona_trace + gr_corona_bin over 32 linear edges against numpy's reductions of the gr_ray_summary rows of the same set
    -- rows that are themselves held to the oracle here -- with sky_deal 1 and 0: the counts exactly, Σg and Σt to 1e-12.  At S.N the
    two settings run one path; at N_DEALT the rays ARE dealt (k_sky_velocities_dealt, three launches, the last chunk partly filled) and
    a factor that did not travel with its ray to the dealt slot would move Σg."""
    from gradus_jl_amd import _lib

    K = G.corona
    L = _lib.load()
    ens.set("kernel", 2).set("precision", 64)
    cfg, rs, pf, keep, _ = S.launch(G, oracle, case, n, ens)
    rows = summary(G, ens, cfg, rs, pf, n)
    isco, _ = S.oracle_table(G, oracle, case)
    S.check(S.compare(rows, S.reference(G, oracle, case, n), isco), f"{case[0]}, n = {n}", n)
    finite = np.isfinite(rows[:, 0])
    g, rho, t = rows[finite, 0], rows[finite, 1], rows[finite, 2]
    for deal in (1, 0):
        ens.set("sky_deal", deal)
        try:
            lim, hits = np.zeros(2), C.c_int64(0)
            _lib.check(L.gr_corona_trace(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), lim.ctypes.data, C.byref(hits), None))
            assert hits.value == finite.sum() and lim[0] == rho.min() and lim[1] == rho.max()
            edges = np.ascontiguousarray(np.linspace(lim[0], lim[1], 32))
            out = np.zeros((3, edges.size))
            _lib.check(L.gr_corona_bin(ens.ctx.handle, edges.ctypes.data, edges.size, out.ctypes.data))
        finally:
            ens.set("sky_deal", 1)
        idx = K._bucket_index(rho, edges)
        np.testing.assert_array_equal(out[0], np.bincount(idx, minlength=edges.size))
        sg, stt = np.bincount(idx, weights=g, minlength=edges.size), np.bincount(idx, weights=t, minlength=edges.size)
        print(f"{case[0]}, n = {n}, sky_deal {deal}: {hits.value} hits, Σg off by {np.max(np.abs(out[1] - sg) / np.maximum(sg, 1e-300)):.2e}, "
              f"Σt by {np.max(np.abs(out[2] - stt) / np.maximum(stt, 1e-300)):.2e}")
        np.testing.assert_allclose(out[1], sg, rtol=1e-12)
        np.testing.assert_allclose(out[2], stt, rtol=1e-12)


def test_energy_ratio_through_the_fp32_kernels(G, ens, oracle):
    """`precision` 32 at tolerance 1e-5 on 3000 DiscCorona samples, by the scheme of tests/f32_scene.py: g of the single-precision
    rows against g from oracle@1e-9 may exceed the BASELINE -- g from oracle@1e-5 end points against the same oracle@1e-9 -- by 1.5 x
    in status mismatches, 1.5 x in the median and 2 x in the 90th percentile (common hits outside 1.05 r_ISCO)."""
    n = 3000
    isco, _ = S.oracle_table(G, oracle, DISC_KERR)
    ref, base = S.reference(G, oracle, DISC_KERR, n), S.reference(G, oracle, DISC_KERR, n, tol=S.F32_TOL)
    try:
        rows = S.device_rows(G, oracle, DISC_KERR, n, ens, precision=32, tol=S.F32_TOL)
    finally:
        ens.set("precision", 64)
    s, b = S.f32_stats(rows[:, 0], rows[:, 3].astype(int), ref, isco), S.f32_stats(base["g"], base["status"], ref, isco)
    print(f"fp32 g: mismatches {s['mism']} / {b['mism']}  median {s['median']:.3e} / {b['median']:.3e}  p90 {s['p90']:.3e} / {b['p90']:.3e}  "
          f"hits {s['hits']} / {b['hits']}  (fp32 / oracle@{S.F32_TOL:g}, both against oracle@1e-9)")
    assert s["hits"] >= 1000 and b["hits"] >= 1000
    assert s["mism"] <= 1.5 * b["mism"]
    assert s["median"] <= 1.5 * b["median"]
    assert s["p90"] <= 2.0 * b["p90"]


def test_entry_points_that_do_not_scale_g_refuse_a_source_with_rows(G, ens, oracle, three):
    """gr_lineprofile, gr_redshift_radius and gr_ray_tangent -- host, _device and _multi -- would return g against the static
    observer for a set with sky_rows: GR_ERR_INVALID_ARGUMENT, the message names sky_rows, nothing is staged (the _device forms are
    called without an output buffer: the refusal comes before that is looked at); gr_rayset_endpoints takes the set; a valid call
    afterwards still works."""
    from gradus_jl_amd import _lib

    L = _lib.load()
    n = 65
    ens.set("kernel", 2).set("precision", 64)
    cfg, rs, pf, keep, _ = S.launch(G, oracle, DISC_KERR, n, ens)
    h = ens.ctx.handle
    arr, sts = _lib.ctx_array(three[0])
    edges = np.ascontiguousarray(np.linspace(0.1, 1.5, 8))
    b = _lib.gr_binning(1.0, 50.0, 3.0, edges.size, edges.ctypes.data)
    flux, pairs, tan = np.zeros(edges.size), np.zeros((n, 2)), np.zeros((n, 8))
    calls = {
        "gr_lineprofile": lambda: L.gr_lineprofile(h, C.byref(cfg), C.byref(rs), C.byref(pf), C.byref(b), flux.ctypes.data, None),
        "gr_lineprofile_device": lambda: L.gr_lineprofile_device(h, C.byref(cfg), C.byref(rs), C.byref(pf), C.byref(b), None, None, None),
        "gr_lineprofile_multi": lambda: L.gr_lineprofile_multi(arr, 3, C.byref(cfg), C.byref(rs), C.byref(pf), C.byref(b), flux.ctypes.data, sts),
        "gr_redshift_radius": lambda: L.gr_redshift_radius(h, C.byref(cfg), C.byref(rs), C.byref(pf), 1.0, 50.0, pairs.ctypes.data, None),
        "gr_redshift_radius_device": lambda: L.gr_redshift_radius_device(h, C.byref(cfg), C.byref(rs), C.byref(pf), 1.0, 50.0, None, None, None),
        "gr_redshift_radius_multi": lambda: L.gr_redshift_radius_multi(arr, 3, C.byref(cfg), C.byref(rs), C.byref(pf), 1.0, 50.0, pairs.ctypes.data, sts),
        "gr_ray_tangent": lambda: L.gr_ray_tangent(h, C.byref(cfg), C.byref(rs), C.byref(pf), tan.ctypes.data, None),
        "gr_ray_tangent_device": lambda: L.gr_ray_tangent_device(h, C.byref(cfg), C.byref(rs), C.byref(pf), None, None, None),
        "gr_ray_tangent_multi": lambda: L.gr_ray_tangent_multi(arr, 3, C.byref(cfg), C.byref(rs), C.byref(pf), tan.ctypes.data, sts),
    }
    for name, call in calls.items():
        assert call() == -1, name                                 # GR_ERR_INVALID_ARGUMENT
        msg = L.gr_last_error().decode()
        assert "sky_rows" in msg and name in msg, (name, msg)
    assert not flux.any() and not pairs.any() and not tan.any()
    pts = np.zeros(n, dtype=G.POINT_DTYPE)
    _lib.check(L.gr_rayset_endpoints(h, C.byref(cfg), C.byref(rs), pts.ctypes.data, None))
    rows = summary(G, ens, cfg, rs, pf, n)
    np.testing.assert_array_equal(pts["status"], rows[:, 3].astype(int))
    assert (pts["status"] == S.HIT).sum() > n // 2


@pytest.fixture(scope="module")
def tabulated(G):
    return G.TabulatedMetric(G.KerrMetric(1.0, 0.9))


def test_a_tabulated_metric_checks_every_row_of_the_source_not_x_obs(G, ens, oracle, tabulated):
    """under GR_METRIC_TABULATED a set with sky_rows whose x_obs is all zero is accepted (x_obs is not read) and gives the bytes of
    the set with x_obs filled in; a set in which ONE sample starts beyond the table's r_max, or below its r_min, is refused with the
    radius in the message -- by every entry point that takes the rows as a host pointer."""
    from gradus_jl_amd import _lib

    L = _lib.load()
    n = 257
    ens.set("kernel", 2).set("precision", 64)
    cfg, rs, pf, keep, src = S.launch(G, oracle, DISC_KERR, n, ens, m=tabulated)
    h = ens.ctx.handle
    filled = summary(G, ens, cfg, rs, pf, n)
    assert rs.x_obs[1] == src[:, 1].max() and (filled[:, 3].astype(int) == S.HIT).sum() > n // 2
    # ... rows of the table against rows of the fused Kerr kernels (the bound of test_corona_of_a_tabulated_metric_equals_the_fused_one
    # outside the ISCO)
    kerr = S.device_rows(G, oracle, DISC_KERR, n, ens)
    both = np.isfinite(filled[:, 0]) & np.isfinite(kerr[:, 0]) & (kerr[:, 1] > S.oracle_table(G, oracle, DISC_KERR)[0])
    assert both.sum() > n // 2
    np.testing.assert_allclose(filled[both, 0], kerr[both, 0], rtol=1e-6)
    blank = type(rs).from_buffer_copy(rs)
    for q in range(4):
        blank.x_obs[q] = 0.0
    assert summary(G, ens, cfg, blank, pf, n).tobytes() == filled.tobytes()
    lim, hits = np.zeros(2), C.c_int64(0)
    _lib.check(L.gr_corona_trace(h, C.byref(cfg), C.byref(blank), C.byref(pf), lim.ctypes.data, C.byref(hits), None))
    assert hits.value == np.isfinite(filled[:, 0]).sum()
    pts = np.zeros(n, dtype=G.POINT_DTYPE)
    arr, sts = _lib.ctx_array([ens.ctx])
    for j, r_bad in ((100, 2.0 * tabulated.r_max), (n - 1, 0.5 * tabulated.r_min), (0, float("nan"))):
        moved = src.copy()
        moved[j, 1] = r_bad
        bad = type(rs).from_buffer_copy(rs)              # x_obs still names the outermost of the ORIGINAL samples: inside the table
        bad.sky_rows = moved.ctypes.data
        out = np.full((n, 4), -7.0)
        calls = {
            "gr_ray_summary": lambda: L.gr_ray_summary(h, C.byref(cfg), C.byref(bad), C.byref(pf), out.ctypes.data, None),
            "gr_ray_summary_multi": lambda: L.gr_ray_summary_multi(arr, 1, C.byref(cfg), C.byref(bad), C.byref(pf), out.ctypes.data, sts),
            "gr_corona_trace": lambda: L.gr_corona_trace(h, C.byref(cfg), C.byref(bad), C.byref(pf), lim.ctypes.data, C.byref(hits), None),
            "gr_corona_trace_multi": lambda: L.gr_corona_trace_multi(arr, 1, C.byref(cfg), C.byref(bad), C.byref(pf), lim.ctypes.data, C.byref(hits), sts),
            "gr_rayset_endpoints": lambda: L.gr_rayset_endpoints(h, C.byref(cfg), C.byref(bad), pts.ctypes.data, None),
            "gr_rayset_endpoints_multi": lambda: L.gr_rayset_endpoints_multi(arr, 1, C.byref(cfg), C.byref(bad), pts.ctypes.data, sts),
        }
        for name, call in calls.items():
            assert call() == -1, (name, r_bad)
            msg = L.gr_last_error().decode()
            assert "metric table" in msg and ("nan" if r_bad != r_bad else f"{r_bad:.6f}"[:8]) in msg, (name, msg)
        assert np.all(out == -7.0)
    # a refused gr_corona_trace leaves no rows behind, and the context still works
    edges, bins = np.array([1.0, 2.0]), np.zeros((3, 2))
    assert L.gr_corona_bin(h, edges.ctypes.data, 2, bins.ctypes.data) != 0
    assert summary(G, ens, cfg, rs, pf, n).tobytes() == filled.tobytes()
