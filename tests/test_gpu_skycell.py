"""`gr_sky_cells` on the MI355X: the sky-cell instantiation of the tangent kernels (the (θ, ϕ) seed on a source's sky, one
(t, r, ϕ, g, J, status) row per cell) in both shapes -- one lane per ray, a pair of lanes per ray -- under the bars the host
build is held to (tests/test_skycell_host.py; scenes, references and bars: tests/skycell_scene.py)."""
import ctypes as C

import numpy as np
import pytest

import harness_skycell as H
import skycell_scene as S

pytestmark = pytest.mark.gpu

SHAPES = [0, 1]
GR_ERR_INVALID_ARGUMENT = -1


def rows_of(G, ens, shape, su, cosθ, ϕ):
    ens.set("tangent_pairs", shape)
    return S.device_rows(G, ens, su, cosθ, ϕ)


@pytest.mark.parametrize("shape", SHAPES, ids=["lane", "pair"])
def test_flat_space_rows_equal_the_closed_form(G, ens, oracle, shape):
    su = S.setup(G, S.FLAT, oracle)
    cosθ, ϕ = S.FLAT.cells(G)
    rows = rows_of(G, ens, shape, su, cosθ, ϕ)
    S.check_against_flat_space(rows, su, cosθ, ϕ, f"device shape {shape}")
    np.testing.assert_allclose(rows[:, 3], 1.0, rtol=1e-12)


@pytest.mark.parametrize("shape", SHAPES, ids=["lane", "pair"])
@pytest.mark.parametrize("scene", [S.KERR, S.JOHANNSEN], ids=lambda s: s.name)
def test_rows_equal_the_oracle_and_J_its_richardson_differences(G, ens, oracle, scene, shape):
    su, cosθ, ϕ, ref = S.reference(oracle, G, scene)
    rows = rows_of(G, ens, shape, su, cosθ, ϕ)
    S.check_against_oracle(rows, ref, f"{scene.name} shape {shape}")


@pytest.mark.parametrize("scene", [S.FLAT, S.KERR], ids=lambda s: s.name)
def test_the_two_shapes_agree(G, ens, oracle, scene):
    """statuses equal, values to 1e-11, J to 1e-9 of its scale: the bar test_the_two_tangent_shapes_agree holds"""
    su = S.setup(G, scene, oracle)
    cosθ, ϕ = scene.cells(G)
    lane, pair = (rows_of(G, ens, shape, su, cosθ, ϕ) for shape in SHAPES)
    assert np.array_equal(lane[:, 5], pair[:, 5])
    hit = lane[:, 5] == 1.0
    assert hit.sum() >= 50 and np.all(np.isnan(lane[~hit][:, :5])) and np.all(np.isnan(pair[~hit][:, :5]))
    np.testing.assert_allclose(pair[hit, 0:4], lane[hit, 0:4], rtol=1e-11)
    scale = np.abs(lane[hit, 4]).max()
    assert np.abs(pair[hit, 4] - lane[hit, 4]).max() < 1e-9 * scale
    # 729 cells: the library's own choice (tangent_pairs 2) takes the pairs
    auto = rows_of(G, ens, 2, su, cosθ, ϕ)
    assert auto.tobytes() == pair.tobytes()


@pytest.mark.parametrize("shape", SHAPES, ids=["lane", "pair"])
def test_a_shorter_launch_gives_the_first_rows_of_a_longer_one(G, ens, oracle, shape):
    """n = 1, 63, 64, 65 and 729: an odd count ends in the last pair of a wave, 64 and 65 cross a wave of the lane shape"""
    su = S.setup(G, S.KERR, oracle)
    cosθ, ϕ = S.KERR.cells(G)
    # (cells in an order that mixes hits and misses into every prefix)
    order = np.random.default_rng(11).permutation(cosθ.size)
    cosθ, ϕ = np.ascontiguousarray(cosθ[order]), np.ascontiguousarray(ϕ[order])
    full = rows_of(G, ens, shape, su, cosθ, ϕ)
    assert not np.any(full == -777.0)
    for k in (1, 63, 64, 65):
        part = rows_of(G, ens, shape, su, cosθ[:k].copy(), ϕ[:k].copy())
        assert part.tobytes() == full[:k].tobytes(), k
    again = rows_of(G, ens, shape, su, cosθ, ϕ)
    assert again.tobytes() == full.tobytes()
    empty = rows_of(G, ens, shape, su, cosθ[:0].copy(), ϕ[:0].copy())
    assert empty.shape == (0, 6)


@pytest.mark.parametrize("scene", [S.FLAT, S.KERR], ids=lambda s: s.name)
def test_device_rows_equal_the_host_build(G, ens, oracle, scene):
    """Same source, two compilers (hipcc for gfx950, g++ for the host): values to 1e-10, J to 1e-7 of its scale; the seeding kernel
    against the numpy closed form the harness uses on the way"""
    su = S.setup(G, scene, oracle)
    cosθ, ϕ = scene.cells(G)
    host = H.sky_cells(su, cosθ, ϕ)
    for shape in SHAPES:
        dev = rows_of(G, ens, shape, su, cosθ, ϕ)
        assert np.array_equal(dev[:, 5], host[:, 5])
        hit = host[:, 5] == 1.0
        err = np.abs(dev[hit, 0:4] / host[hit, 0:4] - 1.0).max()
        scale = np.abs(host[hit, 4]).max()
        errJ = np.abs(dev[hit, 4] - host[hit, 4]).max() / scale
        print(f"{scene.name} shape {shape}: values {err:.2e}, J {errJ:.2e} of scale {scale:.3g}")
        np.testing.assert_allclose(dev[hit, 0:4], host[hit, 0:4], rtol=1e-10)
        assert errJ < 1e-7


def test_multi_over_1_2_4_contexts_gives_the_bytes_of_one(G, ens, oracle):
    su = S.setup(G, S.KERR, oracle)
    cosθ, ϕ = S.KERR.cells(G)
    cosθ, ϕ = cosθ[:365].copy(), ϕ[:365].copy()          # (an odd count: shares of 92, 91, 91, 91)
    many = G.EnsembleMI355X(devices=[0, 0, 0, 0])
    try:
        for shape in SHAPES:
            one = rows_of(G, ens, shape, su, cosθ, ϕ)
            many.set("tangent_pairs", shape)
            for k in (1, 2, 4):
                got = S.device_rows(G, ens, su, cosθ, ϕ, contexts=many.contexts[:k])
                assert got.tobytes() == one.tobytes(), (shape, k)
    finally:
        for c in many.contexts:
            c.close()


def test_refusals_come_before_any_launch(G, ens, oracle):
    L = G._lib.load()
    su = S.setup(G, S.KERR, oracle)
    cosθ, ϕ = (a[:8].copy() for a in S.KERR.cells(G))
    out = np.full((8, 6), -777.0)
    st = G._lib.gr_stats()

    def call(cfg=None, pf=None, cells=None):
        cells = S.skycells_struct(G, su, cosθ, ϕ) if cells is None else cells
        st.rays = 0
        rc = L.gr_sky_cells(ens.ctx.handle, C.byref(su["cfg"] if cfg is None else cfg), C.byref(cells), C.byref(su["pf"] if pf is None else pf),
                            out.ctypes.data, C.byref(st))
        return rc

    def refused(**kw):
        rc = call(**kw)
        assert rc == GR_ERR_INVALID_ARGUMENT, (rc, L.gr_last_error())
        assert st.rays == 0 and np.all(out == -777.0)          # nothing ran, nothing was written
        return L.gr_last_error().decode()

    # no geometry
    no_disc = S.setup(G, S.KERR, oracle)["config"].abi_config()
    no_disc.disc_id = 0
    assert "geometry" in refused(cfg=no_disc)
    # a point function without the source's velocity
    pf = type(su["pf"]).from_buffer_copy(su["pf"])
    pf.has_u_src = 0
    assert "has_u_src" in refused(pf=pf)
    # a direction on the pole
    for bad in (1.0, -1.0, 1.5, float("nan")):
        c2 = cosθ.copy()
        c2[5] = bad
        assert "cos" in refused(cells=S.skycells_struct(G, su, c2, ϕ))
    # null arrays
    cells = S.skycells_struct(G, su, cosθ, ϕ)
    cells.phi = None
    refused(cells=cells)
    # ... and the same call unharmed goes through
    assert call() == 0 and st.rays == 8 and not np.any(out == -777.0)


def test_a_source_outside_a_tabulated_metrics_range_is_refused(G, ens, oracle):
    L = G._lib.load()
    su = S.setup(G, S.KERR, oracle)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (a coarse table: only its radial range is read here)
        m = G.TabulatedMetric(G.KerrMetric(1.0, 0.5), r_max=8.0, m_r=4, n_theta=8, max_refinements=0, strict=False)
    x_src = su["x_src"]
    config = G.tracing_configuration(m, np.array([0.0, 6.0, 1.0, 0.0]), np.zeros((1, 4)), G.ThinDisc(0.0, 7.0), (0.0, 50.0),
                                     chart=G.chart_for_metric(m, 7.5), callback=G.domain_upper_hemisphere())
    cfg = config.abi_config()
    cosθ, ϕ = (a[:4].copy() for a in S.KERR.cells(G))
    out = np.full((4, 6), -777.0)
    cells = S.skycells_struct(G, su, cosθ, ϕ)          # the source at r = 10.8, the table ends at 8
    assert x_src[1] > 8.0
    rc = L.gr_sky_cells(ens.ctx.handle, C.byref(cfg), C.byref(cells), C.byref(su["pf"]), out.ctypes.data, None)
    assert rc == GR_ERR_INVALID_ARGUMENT and b"metric table" in L.gr_last_error() and np.all(out == -777.0)

