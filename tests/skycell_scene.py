"""The scenes of the sky-cell tests (tests/test_skycell_host.py on the host build of the tangent kernels,
tests/test_gpu_skycell.py through gr_sky_cells), their references and the bars the issue sets.

    python tests/skycell_scene.py          prints the oracle's own Richardson self-consistency, which the J bar rests on

References, none of which has been near the code under test:
  flat space   the straight line from the source to the cone |cos θ| = gtol (the thin disc's wedge) in closed form, its
               Jacobian by complex-step differentiation of that closed form;
  Kerr, ...    `oracle.trace` of `corona.sky_angles_to_velocity` rays for t, r, ϕ, g and the status; J from Richardson-extrapolated
               central differences of the oracle's (r, ϕ) with h = 5e-4 and 2.5e-4 in θ and ϕ_sky.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GTOL = 1e-2
RTOL_ROW = 1e-6        # t, r, ϕ, g against the oracle: the bar of test_corona_rows_equal_oracle_traced_rays_and_their_energy_ratio
RTOL_J = 1e-4          # J against the oracle's Richardson differences (factor 20 over the reference's own self-consistency)
RTOL_FLAT = 2e-7       # flat space, r, ϕ, t: the bar of test_flat_space_exact.py
RTOL_FLAT_J = 1e-6
MAX_STATUS_MISMATCH = 2
MAX_EXCLUDED = 0.05    # of the hit cells, from the J comparison
H_PAIR = (5e-4, 2.5e-4)
STATUS_FLOAT = {2: 1.0, 1: -3.0, 0: 7.0, 3: 0.0}       # GR_STATUS_* -> _tmp_status_to_float (adaptive-sample.jl:16-26)


class Scene:
    def __init__(self, name, oracle_metric, params, metric_class, r, h, vf, disc, t_max, outer, level, cells=None):
        self.name, self.oracle_metric, self.params, self.metric_class = name, oracle_metric, params, metric_class
        self.r, self.h, self.vf, self.disc, self.t_max, self.outer, self.level, self._cells = r, h, vf, disc, t_max, outer, level, cells

    def metric(self, G):
        return getattr(G, self.metric_class)(*self.params)

    def source(self, G):
        vf = getattr(G.SourceVelocities, self.vf)
        return G.RingCorona(r=self.r, h=self.h, vf=vf).sample_position_velocity(self.metric(G))

    def cells(self, G):
        """(cos θ, ϕ) of the scene's cells"""
        if self._cells is not None:
            return self._cells
        return level_centres(G, self.level)

    def oracle_config(self, O, tol=1e-9):
        return O.make_config(self.oracle_metric, self.params, disc=self.disc, lambda_max=self.t_max, upper_hemisphere=True,
                             outer_radius=self.outer, gtol=GTOL, abstol=tol, reltol=tol)


def level_centres(G, level):
    """the centres of all 9^level cells of a sky's level `level` (the order trace_initial makes them in)"""
    grid = G.AdaptiveSky(lambda c, p: None).grid
    for _ in range(1, level):
        grid.refine_many(grid.leaves())
    leaves = grid.leaves()
    return np.ascontiguousarray(grid.pos[leaves, 0]), np.ascontiguousarray(grid.pos[leaves, 1])


def _flat_cells():
    k = np.arange(50)
    return np.ascontiguousarray(0.2 + 0.75 * k / 49.0), np.ascontiguousarray(np.mod(0.7 + 2.399963 * k, 2 * math.pi) - math.pi)


FLAT = Scene("flat", "kerr", (0.0, 0.0), "KerrMetric", 6.0, 4.0, "stationary", (0.0, 1.0e7), 1.0e6, 2.0e6, None, _flat_cells())
KERR = Scene("kerr", "kerr", (1.0, 0.998), "KerrMetric", 10.0, 4.0, "co_rotating", (0.0, 1.0e7), 1.0e6, 2.0e6, 3)
JOHANNSEN = Scene("johannsen", "johannsen", (1.0, 0.7, 1.0, 0.5, -0.5, 1.0), "JohannsenMetric", 10.0, 4.0, "co_rotating", (0.0, 1.0e7), 1.0e6,
                  2.0e6, 2)


def setup(G, scene, O, ensemble=None):
    """What gr_sky_cells and the host harness take for a scene: cfg, pf (redshift against the source's velocity; the disc
    velocity inside the ISCO is Kerr's analytic plunge or, for another metric, the ORACLE's plunging table -- the tests
    compare g outside the ISCO), the source and its sky frame."""
    from gradus_jl_amd.corona import _cart_to_spher_jacobian, tetradframe_matrix
    from gradus_jl_amd.pointfunctions import GR_PF_REDSHIFT, PointFunction
    from gradus_jl_amd.rendering import abi_pointfunction
    from gradus_jl_amd.tracing import tracing_configuration

    m = scene.metric(G)
    x_src, v_src = scene.source(G)
    x_src, v_src = np.array(x_src, dtype=np.float64), np.array(v_src, dtype=np.float64)
    B = np.eye(4)
    B[1:, 1:] = _cart_to_spher_jacobian(x_src[2], x_src[3])
    Mx = np.ascontiguousarray(tetradframe_matrix(m, x_src, v_src) @ B)
    flat = scene.params[0] == 0.0
    chart = G.PolarChart(0.0, scene.outer) if flat else G.chart_for_metric(m, scene.outer)
    kw = {} if ensemble is None else {"ensemble": ensemble}
    config = tracing_configuration(m, x_src, np.zeros((1, 4)), G.ThinDisc(*scene.disc), (0.0, scene.t_max), chart=chart,
                                   callback=G.domain_upper_hemisphere(), gtol=GTOL, **kw)
    r_isco = 1e-3 if flat else m.isco()      # (flat space has no ISCO; the library asks for a positive one: every landing radius lies outside)
    table = None
    if scene.oracle_metric != "kerr":
        ocfg = scene.oracle_config(O)
        table = tuple(O.plunging_table(ocfg, O.isco(ocfg)))
    pf, keep = abi_pointfunction(PointFunction(None, device_pf=GR_PF_REDSHIFT, extra={"r_isco": r_isco, "plunge": table}))
    pf.has_u_src = 1
    for q in range(4):
        pf.u_src[q] = v_src[q]
    return {"m": m, "config": config, "cfg": config.abi_config(), "pf": pf, "keep": keep, "x_src": x_src, "v_src": v_src, "Mx": Mx,
            "r_isco": r_isco}


def skycells_struct(G, su, cosθ, ϕ):
    cells = G._lib.gr_skycells()
    for q in range(4):
        cells.x_src[q] = su["x_src"][q]
    for q, val in enumerate(su["Mx"].ravel()):
        cells.Mx[q] = val
    cells.cos_theta, cells.phi, cells.n = cosθ.ctypes.data, ϕ.ctypes.data, cosθ.size
    return cells


def device_rows(G, ens, su, cosθ, ϕ, contexts=None):
    """(n, 6) rows of gr_sky_cells (or gr_sky_cells_multi over `contexts`)"""
    import ctypes as C

    L = G._lib.load()
    cosθ, ϕ = np.ascontiguousarray(cosθ, dtype=np.float64), np.ascontiguousarray(ϕ, dtype=np.float64)
    cells = skycells_struct(G, su, cosθ, ϕ)
    out = np.full((cosθ.size, 6), -777.0)
    if contexts is None:
        G._lib.check(L.gr_sky_cells(ens.ctx.handle, C.byref(su["cfg"]), C.byref(cells), C.byref(su["pf"]), out.ctypes.data, None))
    else:
        arr, sts = G._lib.ctx_array(contexts)
        G._lib.check(L.gr_sky_cells_multi(arr, len(contexts), C.byref(su["cfg"]), C.byref(cells), C.byref(su["pf"]), out.ctypes.data, sts))
    return out


# ---- flat space: the closed form ----
def flat_landing(x_src, θ, ϕ):
    """(r, ϕ_disc, t) where the ray that leaves x_src = (t, r, θ, ϕ = 0) of flat space in the sky direction (θ, ϕ) first meets
    the cone |cos θ| = gtol; works on complex θ or ϕ (complex-step differentiation).  The sky's axes are the Cartesian axes at
    the source -- sky_angles_to_velocity turns -k̂ into spherical components with the Cartesian -> spherical Jacobian
    (samplers.jl:81-99) -- so the photon moves along -k̂."""
    r0, θ0 = x_src[1], x_src[2]
    X = r0 * np.array([math.sin(θ0), 0.0, math.cos(θ0)])
    V = [-np.sin(θ) * np.cos(ϕ), -np.sin(θ) * np.sin(ϕ), -np.cos(θ)]
    g2 = GTOL * GTOL
    A = V[2] * V[2] - g2 * (V[0] * V[0] + V[1] * V[1] + V[2] * V[2])
    Bq = 2 * (X[2] * V[2] - g2 * (X[0] * V[0] + X[1] * V[1] + X[2] * V[2]))
    Cq = X[2] * X[2] - g2 * r0 * r0
    sq = np.sqrt(Bq * Bq - 4 * A * Cq)
    r1, r2 = (-Bq - sq) / (2 * A), (-Bq + sq) / (2 * A)
    lo = np.where(np.real(r1) < np.real(r2), r1, r2)
    hi = np.where(np.real(r1) < np.real(r2), r2, r1)
    lam = np.where(np.real(lo) > 0, lo, hi)          # the first crossing ahead of the source
    P = [X[i] + V[i] * lam for i in range(3)]
    r = np.sqrt(P[0] * P[0] + P[1] * P[1])        # r |sin θ| of the landing point
    # atan2 for complex arguments: the analytic arctan of the quotient, moved to the quadrant of the real parts
    q = np.arctan(P[1] / P[0])
    ϕd = q + (np.arctan2(np.real(P[1]), np.real(P[0])) - np.real(q))
    return r, ϕd, lam


def flat_reference(x_src, cosθ, ϕ):
    """(t, r, ϕ_disc, J) of the closed form; J = |∂(r, ϕ_disc)/∂(θ, ϕ)| / sin θ by complex steps of 1e-30"""
    θ = np.arccos(cosθ)
    h = 1e-30
    r, ϕd, lam = flat_landing(x_src, θ, ϕ)
    rθ, ϕθ, _ = flat_landing(x_src, θ + 1j * h, ϕ + 0j)
    rϕ, ϕϕ, _ = flat_landing(x_src, θ + 0j, ϕ + 1j * h)
    J = np.abs(np.imag(rθ) / h * np.imag(ϕϕ) / h - np.imag(rϕ) / h * np.imag(ϕθ) / h) / np.sin(θ)
    return np.real(lam), np.real(r), np.real(ϕd), J


# ---- curved space: the oracle ----
def oracle_points(O, G, scene, su, θ, ϕ, tol=1e-9):
    from gradus_jl_amd.corona import sky_angles_to_velocity

    v = sky_angles_to_velocity(su["m"], su["x_src"], su["v_src"], θ, ϕ)
    return O.trace(scene.oracle_config(O, tol), su["x_src"], v)


def oracle_rows(O, G, scene, su, cosθ, ϕ):
    """(t, r, ϕ, g, status float) per cell from the oracle's end points; g by energy_ratio in numpy, NaN inside 1.05 r_isco
    (there the disc velocity is the plunging table's, which no closed form on the host gives)"""
    from gradus_jl_amd import corona as K

    pts = oracle_points(O, G, scene, su, np.arccos(cosθ), ϕ)
    r = pts["x"][:, 1] * np.abs(np.sin(pts["x"][:, 2]))
    status = np.array([STATUS_FLOAT[int(s)] for s in pts["status"]])
    g = np.full(r.size, np.nan)
    out = (status == 1.0) & (r > 1.05 * su["r_isco"])
    if out.any():
        g[out] = K.energy_ratio(su["m"], pts[out], su["v_src"], K.circular_fourvelocity(su["m"], r[out]))
    return pts["x"][:, 0], r, pts["x"][:, 3], g, status


def oracle_central(O, G, scene, su, θ, ϕ, h, tol=1e-9):
    """central differences of the oracle's (r, ϕ_disc) in θ and ϕ_sky with step h: (r_θ, r_ϕ, ϕ_θ, ϕ_ϕ) and the four
    neighbours' statuses (n, 4)"""
    n = θ.size
    θs = np.concatenate([θ + h, θ - h, θ, θ])
    ϕs = np.concatenate([ϕ, ϕ, ϕ + h, ϕ - h])
    pts = oracle_points(O, G, scene, su, θs, ϕs, tol)
    r = (pts["x"][:, 1] * np.abs(np.sin(pts["x"][:, 2]))).reshape(4, n)
    p = pts["x"][:, 3].reshape(4, n)
    d = 1.0 / (2 * h)
    return (r[0] - r[1]) * d, (r[2] - r[3]) * d, (p[0] - p[1]) * d, (p[2] - p[3]) * d, pts["status"].reshape(4, n).T


def oracle_jacobian(O, G, scene, su, cosθ, ϕ, pair=H_PAIR, tol=1e-9):
    """J = |∂(r, ϕ)/∂(θ, ϕ_sky)| / sin θ from Richardson-extrapolated central differences, (4 D(h/2) - D(h)) / 3 per
    derivative; and per cell whether all eight neighbours hit"""
    θ = np.arccos(cosθ)
    a = oracle_central(O, G, scene, su, θ, ϕ, pair[0], tol)
    b = oracle_central(O, G, scene, su, θ, ϕ, pair[1], tol)
    rθ, rϕ, pθ, pϕ = ((4 * y - x) / 3 for x, y in zip(a[:4], b[:4]))
    ok = np.all(a[4] == 2, axis=1) & np.all(b[4] == 2, axis=1)
    return np.abs(rθ * pϕ - rϕ * pθ) / np.sin(θ), ok


# ---- what both test files assert ----
_cache = {}


def reference(oracle, G, scene):
    """the oracle's rows and Jacobian of a scene: computed once, shared, read-only"""
    if scene.name not in _cache:
        su = setup(G, scene, oracle)
        cosθ, ϕ = scene.cells(G)
        t, r, p, g, status = oracle_rows(oracle, G, scene, su, cosθ, ϕ)
        J, ok = oracle_jacobian(oracle, G, scene, su, cosθ, ϕ)
        ref = {"t": t, "r": r, "ϕ": p, "g": g, "status": status, "J": J, "ok": ok}
        for a in ref.values():
            a.setflags(write=False)
        _cache[scene.name] = (su, cosθ, ϕ, ref)
    return _cache[scene.name]


def check_against_oracle(rows, ref, label=""):
    """the bars of the issue: at most 2 status mismatches; t, r, ϕ, g at 1e-6 on cells both sides hit; J at 1e-4 on hit cells with
    r < 100 whose differencing neighbours all hit, which must leave out at most 5 % of the hit cells"""
    assert int(np.sum(rows[:, 5] != ref["status"])) <= MAX_STATUS_MISMATCH, label
    miss = rows[:, 5] != 1.0
    assert np.all(np.isnan(rows[miss][:, :5])), label
    hit = (rows[:, 5] == 1.0) & (ref["status"] == 1.0)
    assert hit.sum() > 0.5 * (ref["status"] == 1.0).sum() > 10
    for k, name in ((0, "t"), (1, "r"), (2, "ϕ")):
        np.testing.assert_allclose(rows[hit, k], ref[name][hit], rtol=RTOL_ROW, err_msg=f"{label} {name}")
    outside = hit & ~np.isnan(ref["g"])
    assert outside.sum() > 0.8 * hit.sum()
    np.testing.assert_allclose(rows[outside, 3], ref["g"][outside], rtol=RTOL_ROW, err_msg=f"{label} g")
    use = hit & (ref["r"] < 100.0) & ref["ok"]
    excluded = 1.0 - use.sum() / hit.sum()
    assert excluded <= MAX_EXCLUDED, (label, excluded)
    err = np.abs(rows[use, 4] / ref["J"][use] - 1.0)
    print(f"{label}: {int(hit.sum())} hit, J on {int(use.sum())} (excluded {excluded:.2%}), max rel err {err.max():.2e}")
    np.testing.assert_allclose(rows[use, 4], ref["J"][use], rtol=RTOL_J, err_msg=f"{label} J")


def check_against_flat_space(rows, su, cosθ, ϕ, label=""):
    t, r, ϕd, J = flat_reference(su["x_src"], cosθ, ϕ)
    assert np.all(rows[:, 5] == 1.0), label
    np.testing.assert_allclose(rows[:, 0], t, rtol=RTOL_FLAT, err_msg=f"{label} t")
    np.testing.assert_allclose(rows[:, 1], r, rtol=RTOL_FLAT, err_msg=f"{label} r")
    np.testing.assert_allclose(rows[:, 2], ϕd, rtol=RTOL_FLAT, err_msg=f"{label} ϕ")
    np.testing.assert_allclose(rows[:, 4], J, rtol=RTOL_FLAT_J, err_msg=f"{label} J")


def main():
    import __graft_entry__ as g

    g.build_oracle()
    import gradus_jl_amd as G
    from oracle import oracle as O

    for scene in (KERR, JOHANNSEN):
        su = setup(G, scene, O)
        cosθ, ϕ = scene.cells(G)
        t, r, p, gg, status = oracle_rows(O, G, scene, su, cosθ, ϕ)
        hit = status == 1.0
        J1, ok1 = oracle_jacobian(O, G, scene, su, cosθ, ϕ, (1e-3, 5e-4))
        J2, ok2 = oracle_jacobian(O, G, scene, su, cosθ, ϕ, H_PAIR)
        J3, ok3 = oracle_jacobian(O, G, scene, su, cosθ, ϕ, H_PAIR, tol=1e-12)
        near = hit & (r < 100.0)
        use = near & ok1 & ok2 & ok3
        print(f"{scene.name}: cells {cosθ.size}, hit {int(hit.sum())}, r < 100: {int(near.sum())}, lost to status changes "
              f"{int(near.sum() - use.sum())}, excluded {1.0 - use.sum() / max(hit.sum(), 1):.3%}")
        print(f"  Richardson pairs (1e-3, 5e-4) vs (5e-4, 2.5e-4): max rel {np.max(np.abs(J1[use] / J2[use] - 1.0)):.2e}")
        print(f"  tolerance 1e-9 vs 1e-12:                        max rel {np.max(np.abs(J2[use] / J3[use] - 1.0)):.2e}")


if __name__ == "__main__":
    main()
