"""`AdaptivePlane(m, x, d)` on the MI355X: the cells of an observer's image plane traced by gr_plane_cells (velocities formed on the
device) against the CPU oracle, the resident plane (gr_sky_create_plane: pair search, refinement and fill as kernels) against the
host route on the same ensemble bit for bit, the refusals, and several contexts.  Scenes: tests/plane_scene.py."""
import ctypes as C
import math

import numpy as np
import pytest

import plane_scene as S

pytestmark = pytest.mark.gpu

FIELDS = ("pos", "level", "children", "neighbours", "parent", "location")
INVALID = -1      # GR_ERR_INVALID_ARGUMENT


def launches(sky, since=0):
    return [n for n, _ in sky.tracer["launches"][since:]]


def state(sky):
    g = sky.grid
    out = {f: getattr(g, f)[:g.n + 1].tobytes() for f in FIELDS}
    out["values"] = sky.values.tobytes()
    out["n"] = (g.n, sky.n_values)
    return out


def assert_same(a, b):
    sa, sb = state(a), state(b)
    for key in sa:
        assert sa[key] == sb[key], key


def download_again(sky):
    """drop the mirrors: the next read fetches every cell from the device"""
    sky._n_values, sky._stale = 0, True


def close(a, b, tol):
    """|a - b| <= tol max(|b|, 1), the largest violation first"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    worst = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))
    print(f"largest deviation {worst:.3e} (bound {tol:g})")
    return worst <= tol


@pytest.fixture(scope="module")
def host_b(G, _ens_session):
    """scene B on the host route after trace_initial and two trace_steps; only ever read"""
    return S.device_plane(G, _ens_session, "B", resident=False, steps=2)


@pytest.fixture(scope="module")
def dev_b(G, _ens_session, host_b):
    """... and resident on the device; only ever read"""
    return S.device_plane(G, _ens_session, "B", resident=True, steps=2)


def test_cells_against_the_oracle(G, ens, oracle):
    """Measured on an MI355X: statuses equal at all 819 cells; 30 cells, all swallowed by the hole (WithinInnerBoundary), differ from
    the oracle by up to 1.5e-2 in x (t and ϕ), 4.3e-2 in v and 1.2e-6 in λ_max -- the oracle differs from itself by 1.1e-2 on the
    same 30 cells when its velocities are moved by one ulp; the device with host-formed velocities gives the same bytes."""
    sky = S.device_plane(G, ens, "A", resident=False, steps=0)
    assert len(sky.grid) == 819 and launches(sky) == [9, 72, 648]
    cells = np.arange(1, 820)
    α, β = sky.grid.pos[cells, 0].copy(), sky.grid.pos[cells, 1].copy()
    mine = sky.values[cells]
    # one launch of all 819 cells gives the rows the three launches of trace_initial gave
    again = sky.calculate_value(α, β)
    assert again.tobytes() == mine.tobytes()
    cfg = S.oracle_config(G, oracle)
    ref = oracle.trace(cfg, S.X_OBS, oracle.map_impact_parameters(cfg, S.X_OBS, -α, β))
    np.testing.assert_array_equal(mine["status"], ref["status"])
    assert {0, 1, 2} >= set(np.unique(mine["status"])) and (mine["status"] == 2).sum() > 100
    # The render's own parity bound against the oracle (README): 1e-6 on λ, end positions and velocities "on every
    # pixel the oracle itself determines to 1e-7".  The oracle is asked here: the same rays with velocities one ulp larger.  What it
    # does not determine must be rays swallowed by the hole and nothing else -- they stop at whichever step first lands inside
    # 1.01 r₊, where t, ϕ and v^t diverge -- and those are held to what tests/test_gpu_parity.py (_compare_points) holds them to.
    v_ref = oracle.map_impact_parameters(cfg, S.X_OBS, -α, β)
    nudged = oracle.trace(cfg, S.X_OBS, np.nextafter(v_ref, np.inf))
    spread = np.zeros(cells.size)
    for f in ("x", "v", "lambda_max"):
        d = np.abs(nudged[f] - ref[f]) / np.maximum(np.abs(ref[f]), 1.0)
        spread = np.maximum(spread, d.reshape(cells.size, -1).max(axis=1))
    determined = (spread < 1e-7) & (nudged["status"] == ref["status"])
    swallowed = ref["status"] == 1
    print(f"{(~determined).sum()} of {cells.size} cells are not determined by the oracle itself (spread up to {spread.max():.3e}); {swallowed.sum()} swallowed")
    assert not (~determined & ~swallowed).any() and determined.sum() > 700
    for f in ("x", "v", "lambda_max"):
        assert close(mine[f][determined], ref[f][determined], 1e-6), f
    rest = ~determined
    np.testing.assert_allclose(mine["lambda_max"][rest], ref["lambda_max"][rest], rtol=1e-4)
    np.testing.assert_allclose(mine["x"][rest, 1], ref["x"][rest, 1], rtol=1e-2)
    # the same cells with host-formed velocities: the device's may differ in the last bit
    m = S.metric(G)
    v = G.map_impact_parameters(m, S.X_OBS, -α, β)
    host = G.tracegeodesics(m, S.X_OBS, v, G.ThinDisc(m.isco(), S.R_OUT), (0.0, S.T_MAX), ensemble=ens, abstol=S.TOL, reltol=S.TOL,
                            chart=G.chart_for_metric(m, 4 * S.X_OBS[1]))
    np.testing.assert_array_equal(mine["status"], host["status"])
    for f in ("x", "v", "lambda_max", "x_init", "v_init"):
        assert close(mine[f], host[f], 1e-9), f


def test_the_resident_plane_equals_the_host_route(G, ens):
    host, dev = (S.device_plane(G, ens, "B", resident=r) for r in (False, True))
    assert dev.resident and dev.is_plane and not host.resident
    G.trace_initial(host)
    G.trace_initial(dev)
    assert launches(dev) == launches(host) == [9, 72, 648] and len(dev.grid) == 819
    assert_same(host, dev)
    for expected in S.REFINED["B"][:2]:
        need = G.find_need_refine(host)
        assert need.size == expected
        np.testing.assert_array_equal(G.find_need_refine(dev), need)
        before = len(launches(dev))
        G.trace_step(host)
        G.trace_step(dev)
        assert launches(dev, before) == [8 * need.size] and launches(dev) == launches(host)
        assert_same(host, dev)
    assert dev.grid.leaves().size == 4753
    download_again(dev)
    assert_same(host, dev)
    for a, b in zip(G.unpack_sky(host), G.unpack_sky(dev)):
        assert a.tobytes() == b.tobytes()
    # the middle children hold their parents' whole points
    refined = np.flatnonzero(dev.grid.children[:dev.grid.n + 1, 0])
    assert dev.values[dev.grid.children[refined, 4]].tobytes() == dev.values[refined].tobytes()


@pytest.mark.parametrize("name", ["plane-20", "plane-5", "callable-10", "level-4"])
def test_the_pair_search_under_each_criterion(G, ens, host_b, dev_b, name):
    criterion = {"plane-20": G.check_refine_plane, "plane-5": G.refine_plane(5),
                 "callable-10": lambda s, a, b: G.check_refine_plane(s, a, b, percentage=10),       # a plain callable: the gr_sky_pairs route
                 "level-4": G.refine_to_level(4)}[name]
    assert (G.adaptive.gr_criterion_of(criterion) is None) == (name == "callable-10")
    need = G.find_need_refine(host_b, criterion)
    np.testing.assert_array_equal(G.find_need_refine(dev_b, criterion), need)
    assert need.size > 0
    if name == "plane-20":
        assert need.size == S.REFINED["B"][2]
    print(f"{name}: {need.size} cells")


def test_refusals_leave_the_sky_as_it_was(G, ens):
    L, lib = G._lib.load(), G._lib
    dev = S.device_plane(G, ens, "A", resident=True, steps=0)
    before, n_launches = state(dev), len(launches(dev))

    def untouched():
        download_again(dev)
        assert state(dev) == before and len(launches(dev)) == n_launches

    for ids in ([100, 100], [100, 1], [1], [0], [820]):       # named twice, refined already, out of range
        with pytest.raises(ValueError):
            G.refine_and_trace(dev, ids)
        untouched()
    # a corona criterion on a plane sky
    count = C.c_int64(-5)
    for criterion in (G.check_refine, G.refine_function(G.RadialBox(2.0, 10.0)), G.fine_refine_function(G.RadialBox(2.0, 10.0))):
        assert L.gr_sky_find_need_refine(dev._dev, C.byref(G.adaptive.gr_criterion_of(criterion)), C.byref(count)) == INVALID
        with pytest.raises(TypeError, match="plane"):
            G.find_need_refine(dev, criterion)
        untouched()
    # the maps, the corona's fill and its rows on a plane sky
    bins, out, counts = np.linspace(1.0, 10.0, 4), np.zeros((4, 4, 6)), np.zeros((4, 4), dtype=np.int64)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    assert L.gr_sky_bin_grid(dev._dev, lib.GR_SKY_MAP_REDSHIFT, ptr(bins), 4, ptr(bins), 4, None, ptr(out), None) == INVALID
    assert L.gr_sky_occupancy(dev._dev, ptr(bins), 4, ptr(bins), 4, None, ptr(counts)) == INVALID
    assert L.gr_sky_fill(dev._dev, ptr(bins), 4, ptr(bins), 4, ptr(out), None) == INVALID
    rows = np.zeros((10, 6))
    assert L.gr_sky_download(dev._dev, 0, 10, None, None, None, None, None, None, ptr(rows), None, None) == INVALID
    assert not rows.any()
    for call in (lambda: G.bin_redshift_grid(bins, bins, dev), lambda: G.step_block(S.metric(G), None, dev)):
        with pytest.raises(TypeError, match="AdaptivePlane"):
            call()
    # gr_sky_fill_plane's own arguments
    image = np.zeros((4, 4))
    assert L.gr_sky_fill_plane(dev._dev, None, None, None, 4, ptr(bins), 4, ptr(image), None) == INVALID
    assert L.gr_sky_fill_plane(dev._dev, None, None, ptr(bins), 0, ptr(bins), 4, ptr(image), None) == INVALID
    assert L.gr_sky_fill_plane(dev._dev, None, None, ptr(bins), 4, ptr(bins), 4, None, None) == INVALID
    untouched()
    # a plane criterion, the plane's fill and its points on a corona sky
    corona = G.AdaptiveSky(G.KerrMetric(1.0, 0.998), G.RingCorona(r=10.0, h=4.0), G.ThinDisc(0.0, math.inf), ensemble=ens, resident=True)
    n_cells = corona.n_cells
    assert L.gr_sky_find_need_refine(corona._dev, C.byref(G.adaptive.gr_criterion_of(G.check_refine_plane)), C.byref(count)) == INVALID
    with pytest.raises(TypeError, match="plane"):
        G.find_need_refine(corona, G.check_refine_plane)
    assert L.gr_sky_fill_plane(corona._dev, None, None, ptr(bins), 4, ptr(bins), 4, ptr(image), None) == INVALID
    points = np.zeros(10, dtype=G.POINT_DTYPE)
    assert L.gr_sky_download_points(corona._dev, 0, 10, ptr(points)) == INVALID
    assert not image.any() and not points["status"].any() and corona.n_cells == n_cells == 9
    # null pointers and an untraced plane
    fresh = S.device_plane(G, ens, "A", resident=True)
    assert L.gr_sky_fill_plane(fresh._dev, None, None, ptr(bins), 4, ptr(bins), 4, ptr(image), None) == INVALID
    tr = fresh.tracer
    assert L.gr_plane_cells(ens.ctx.handle, C.byref(tr["cfg"]), None, ptr(bins), ptr(bins), 4, ptr(points), None) == INVALID
    assert L.gr_plane_cells(ens.ctx.handle, C.byref(tr["cfg"]), C.byref(tr["plane"]), None, ptr(bins), 4, ptr(points), None) == INVALID
    # ... and the plane still works
    host = S.device_plane(G, ens, "A", resident=False, steps=0)
    G.refine_and_trace(host, [100, 700])
    G.refine_and_trace(dev, [100, 700])
    assert len(dev.grid) == 837 and launches(dev)[-1] == 16
    assert_same(host, dev)
    with pytest.raises(ValueError, match="traced already"):
        G.trace_initial(dev)


@pytest.mark.parametrize("shape", [(64, 48), (1, 1)], ids=["64x48", "1x1"])
def test_the_device_fill_equals_numpy(G, ens, dev_b, shape):
    m = S.metric(G)
    if shape == (1, 1):
        x_grid, y_grid = np.array([3.7]), np.array([-2.2])
    else:
        x_grid, y_grid = np.linspace(-60.0, 60.0, shape[0]), np.linspace(-35.0, 35.0, shape[1])[::-1].copy()
    redshift = G.ConstPointFunctions.redshift(m) @ G.ConstPointFunctions.filter_intersected()
    radius = np.where(dev_b.values["status"] == 2, dev_b.values["x"][:, 1], np.nan)
    for name, pf in (("default", None), ("redshift", redshift), ("array", radius)):
        host, (h_lower, h_upper) = G.fill_sky_values(dev_b, (x_grid, y_grid), metric=m, pf=pf, cells=True)
        dev, (d_lower, d_upper) = G.fill_sky_values(dev_b, (x_grid, y_grid), metric=m, pf=pf, cells=True, route="device")
        assert dev.shape == (shape[1], shape[0]) and dev.tobytes() == host.tobytes(), name
        np.testing.assert_array_equal(d_lower, h_lower)
        np.testing.assert_array_equal(d_upper, h_upper)
        assert G.fill_sky_values(dev_b, (x_grid, y_grid), metric=m, pf=pf, route="device").tobytes() == host.tobytes()
        if shape != (1, 1):
            hit = dev_b.values["status"] == 2
            if name == "default":
                # a column on the domain's edge or on a boundary between top-level cells (α = ±20 here) lies in no cell: NaN
                outside = np.isin(x_grid, [-60.0, -20.0, 20.0, 60.0])
                assert outside.sum() == 4 and np.isnan(dev[:, outside]).all() and np.isfinite(dev[:, ~outside]).all()
            else:
                np.testing.assert_array_equal(np.isnan(dev), ~(hit[d_lower] & hit[d_upper]))
                assert np.isfinite(dev).any()
    if shape != (1, 1):
        α, β, image = G.fill_sky_values(dev_b, 17, metric=m, route="device")
        assert image.tobytes() == G.fill_sky_values(dev_b, (α, β), metric=m).tobytes()
        with pytest.raises(ValueError, match="resident"):
            G.fill_sky_values(S.device_plane(G, ens, "A", resident=False), (x_grid, y_grid), route="device")


def test_several_contexts_give_the_bytes_of_one(G, ens, host_b):
    two = G.EnsembleMI355X(devices=[0, 0])
    sky = S.device_plane(G, two, "B", resident=False, steps=2)
    assert launches(sky) == launches(host_b)
    assert_same(host_b, sky)
    with pytest.raises(ValueError, match="ONE context"):
        S.device_plane(G, two, "B", resident=True)
