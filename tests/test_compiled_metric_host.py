"""GR_METRIC_COMPILED on the CPU: a user's metric_components recorded, written as the body of GenericMetricT<12>::components and
compiled -- for the host (the device integrator under g++, tests/host_harness_usermetric.cpp) and for gfx950 (hipcc cross-compiles
without a GPU).  Checked:

  the components and their Jacobian through the typed dual numbers against the oracle's dual numbers (the oracle's stand-in
      for a user metric, Kerr and Johannsen as callables, Kerr written through sqrt / exp / log), at 10 x what the catalogue's own
      dual-number path reaches against the oracle on the same points;
  the kernel logic end to end on the 24 x 24 plane of test_tabulated_endpoints_vs_oracle_kernel_logic, at that test's bars;
  the tracer: what it refuses, that it is deterministic, that parameters stay P[i];
  the module: its exports, gr_user_module_info, that a second construction starts no compiler, that a module compiled against
      other kernel sources is refused.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import hostbuild
from test_tabulated_metric import BUMP, X_FAR, bump_components

HERE = os.path.dirname(os.path.abspath(__file__))
MODULES = os.path.join(HERE, "_modules")          # generated bodies and kernel modules of the tests (kept out of git)
R_H_BUMP = 1.0 + math.sqrt(1.0 - 0.81)
JOH = (1.0, 0.7, 2.0, 0.0, 0.0, 1.0)


def kerr_callable(r, th, p=(1.0, 0.998)):
    """kerr-metric.jl:11-28, operation by operation (what the oracle's `kerr` evaluates)"""
    M, a = p
    R = 2.0 * M
    s2 = np.sin(th) ** 2
    Sig = r ** 2 + a ** 2 * (1.0 - s2)
    gam = s2 * R * r * a
    return (-(1.0 - (R * r) / Sig), Sig / (r ** 2 + a ** 2 - R * r), Sig, s2 * (r ** 2 + a ** 2 + (gam * a) / Sig), -gam / Sig)


def johannsen_callable(r, th, p=JOH):
    """johannsen-ad.jl:12-34"""
    M, a, a13, a22, a52, e3 = p
    s2, c2 = np.sin(th) ** 2, np.cos(th) ** 2
    Mr = M / r
    A1, A2, A5 = 1.0 + a13 * Mr ** 3, 1.0 + a22 * Mr ** 2, 1.0 + a52 * Mr ** 2
    Sig = r * r + a * a * c2 + e3 * M ** 3 / r
    Del = r * r - 2.0 * M * r + a * a
    r2a2 = r * r + a * a
    den = (r2a2 * A1 - a * a * A2 * s2) ** 2
    tt = -Sig * (Del - a * a * A2 * A2 * s2) / den
    pp = Sig * s2 * (r2a2 * r2a2 * A1 * A1 - a * a * Del * s2) / den
    tp = -a * (r2a2 * A1 * A2 - Del) * Sig * s2 / den
    return (tt, Sig / (Del * A5), Sig, pp, tp)


def kerr_through_sqrt_exp_log(r, th, p=(1.0, 0.998)):
    """A made-up way of writing Kerr that goes through every elementary function of a component body: Σ = sqrt(Σ²) and
    r = 1 / exp(-log r) where r multiplies 2M.  (Δ keeps the oracle's own operations: what two roundings of Δ differ by is
    amplified by r²/Δ = 1e3 next to the horizon of a = 0.998, where the points start -- that is the formula's conditioning,
    which this test is not about.)"""
    M, a = p
    R = 2.0 * M
    s2 = np.sin(th) ** 2
    S0 = r ** 2 + a ** 2 * (1.0 - s2)
    Sig = np.sqrt(S0 * S0)
    ir = np.exp(-np.log(r))
    gam = s2 * R * a / ir
    return (-(1.0 - (R / ir) / Sig), Sig / (r ** 2 + a ** 2 - R * r), Sig, s2 * (r ** 2 + a ** 2 + (gam * a) / Sig), -gam / Sig)


def _trace(G, f, n_params=0):
    from gradus_jl_amd.compiled_metric import Trace

    return Trace(f, n_params)


def _harness(tr):
    """tests/host_harness_usermetric.cpp built around the generated body of `tr`"""
    os.makedirs(MODULES, exist_ok=True)
    body = os.path.join(MODULES, "host_" + tr.sha256[:16] + ".inc")
    if not os.path.exists(body) or open(body).read() != tr.source:
        with open(body, "w") as f:
            f.write(tr.source)
    return hostbuild.load("host_harness_usermetric.cpp", suffix="_" + tr.sha256[:16], defines=[f'GR_USER_COMPONENTS_FILE="{body}"'])


def _cfg(G, metric_id, params):
    c = G._lib.gr_config()
    c.metric_id = metric_id
    for i, p in enumerate(params):
        c.params[i] = float(p)
    return c


def _points(rng, r_h, n=400):
    """the points of test_tabulated_metric._jacobian_errors on the range a default table has: log-uniform radii from the chart's
    inner radius to 12000, θ uniform on (0, π); r0 (the pole of g_rr the radial derivative is quoted against) as TabulatedMetric"""
    r_min = r_h * (1.0 + 0.9 * 0.01)
    r0 = r_h - 0.1 * (r_min - r_h)
    return r_min * (12000.0 / r_min) ** rng.uniform(0, 1, n), rng.uniform(0.0, math.pi, n), r0


def _jacobian_errors(O, L, cfg, ocfg, rs, ths, r0):
    """test_tabulated_metric._jacobian_errors with the host build of eval() in the table's place: the same scale rule"""
    A, B = [], []
    g, dr, dth = ((C.c_double * 5)() for _ in range(3))
    for r, th in zip(rs, ths):
        assert L.hu_jacobian(C.byref(cfg), C.c_double(r), C.c_double(th), g, dr, dth) == 0
        A.append(np.concatenate([np.array(g), np.array(dr), np.array(dth)]))
        B.append(np.concatenate(O.metric_jacobian(ocfg, r, th)))
    A, B = np.array(A), np.array(B)
    sc = np.abs(B[:, :5]).copy()
    sc[:, 0] = np.maximum(sc[:, 0], 0.1)
    sc[:, 3] = np.maximum(sc[:, 3], 1e-3 * sc[:, 2])
    sc[:, 4] = np.maximum(sc[:, 4], 1e-2 * np.sqrt(sc[:, 0] * sc[:, 3]))
    ev = float(np.max(np.abs(A[:, :5] - B[:, :5]) / sc))
    edr = float(np.max(np.abs(A[:, 5:10] - B[:, 5:10]) * (rs - r0)[:, None] / sc))
    edt = float(np.max(np.abs(A[:, 10:] - B[:, 10:]) / sc))
    return ev, edr, edt


@pytest.fixture(scope="module")
def catalogue_bar(G, oracle):
    """What the parent's own dual-number path -- the catalogue's Johannsen component function through GenericMetricT::eval(), host
    build -- reaches against the oracle's dual numbers on a point set: the yardstick of `only the rounding order differs`.
    Taken at the (M, a) of the metric under test and on its points.  The callables of this file follow the reference's formulas
    operation by operation, as the catalogue's component functions do: a callable that forms Δ = r² - 2Mr + a² in another order
    differs from the oracle by 9e-14 next to the horizon of a = 0.998 (Δ/r² = 1e-3 where the points start), which is that
    formula's conditioning and says nothing about the generated code."""
    L = _harness(_trace(G, kerr_callable))          # (any body: metric ids below 12 take the catalogue's switch)

    def bar(rs, ths, r0, params):
        return _jacobian_errors(oracle, L, _cfg(G, G.metrics.GR_METRIC_JOHANNSEN, params), oracle.make_config("johannsen", params), rs, ths, r0)

    return bar


@pytest.mark.parametrize("which", ["bump", "kerr", "johannsen", "sqrt-exp-log"])
def test_generated_body_matches_the_oracles_dual_numbers(G, oracle, catalogue_bar, which):
    f, name, params, r_h, seed, yard = {
        "bump": (bump_components, "test-bump", BUMP, R_H_BUMP, 7, (1.0, 0.9, 0.0, 0.0, 0.0, 0.0)),
        "kerr": (kerr_callable, "kerr", (1.0, 0.998), 1.0 + math.sqrt(1.0 - 0.998 ** 2), 5, (1.0, 0.998, 0.0, 0.0, 0.0, 0.0)),
        "johannsen": (johannsen_callable, "johannsen", JOH, 1.0 + math.sqrt(1.0 - 0.49), 6, JOH),
        "sqrt-exp-log": (kerr_through_sqrt_exp_log, "kerr", (1.0, 0.998), 1.0 + math.sqrt(1.0 - 0.998 ** 2), 8, (1.0, 0.998, 0.0, 0.0, 0.0, 0.0))}[which]
    rs, ths, r0 = _points(np.random.default_rng(seed), r_h)
    L = _harness(_trace(G, f))
    ocfg = oracle.make_config(name, params)
    if which == "bump":
        with oracle.user_metric_library():
            got = _jacobian_errors(oracle, L, _cfg(G, 12, ()), ocfg, rs, ths, r0)
    else:
        got = _jacobian_errors(oracle, L, _cfg(G, 12, ()), ocfg, rs, ths, r0)
    base = catalogue_bar(rs, ths, r0, yard)
    print(f"compiled {which}: value {got[0]:.3g} d/dr {got[1]:.3g} d/dθ {got[2]:.3g}; catalogue Johannsen at the same (M, a) on the same points: "
          f"{base[0]:.3g} {base[1]:.3g} {base[2]:.3g}")
    assert got[0] <= 10.0 * base[0] and got[1] <= 10.0 * base[1] and got[2] <= 10.0 * base[2], (got, base)
    # ... and the overloads on plain numbers (comps(): values alone) give the values of the dual numbers
    g, gd, dr, dth = ((C.c_double * 5)() for _ in range(4))
    for r, th in zip(rs[:20], ths[:20]):
        L.hu_components(C.byref(_cfg(G, 12, ())), C.c_double(r), C.c_double(th), g)
        L.hu_jacobian(C.byref(_cfg(G, 12, ())), C.c_double(r), C.c_double(th), gd, dr, dth)
        assert list(g) == list(gd)


def test_parameters_reach_the_generated_body(G, oracle):
    """(r, θ, p): the body reads P[i], so one harness build serves two parameter sets"""
    tr = _trace(G, lambda r, th, p: kerr_callable(r, th, p), 2)
    assert "P[0]" in tr.source and "P[1]" in tr.source and "0.998" not in tr.source
    L = _harness(tr)
    g, dr, dth = ((C.c_double * 5)() for _ in range(3))
    for params in ((1.0, 0.998), (1.3, 0.4)):
        L.hu_jacobian(C.byref(_cfg(G, 12, params)), C.c_double(7.0), C.c_double(1.1), g, dr, dth)
        ref = oracle.metric_jacobian(oracle.make_config("kerr", params), 7.0, 1.1)
        np.testing.assert_allclose(np.concatenate([g, dr, dth]), np.concatenate(ref), rtol=1e-13, atol=1e-15)


@pytest.fixture(scope="module")
def cm_bump(G, oracle):
    """the oracle's stand-in for a user metric as a CompiledMetric: its kernel module is built here, once (and the registry is
    left empty behind this file: other tests count on the ids above the catalogue being refused)"""
    from gradus_jl_amd import compiled_metric

    with oracle.user_metric_library():
        isco = oracle.isco(oracle.make_config("test-bump", BUMP))
    yield G.CompiledMetric(bump_components, inner_radius=R_H_BUMP, isco=isco, cache_dir=MODULES)
    compiled_metric.unload_all()


def _compare_endpoints(got, ref, x_rtol=1e-6, max_flips=0, max_outliers=0, r_horizon=None):
    """(tests/test_tabulated_metric.py) status per ray, then positions / velocities / affine time at x_rtol (relative to the
    component, with a floor of 1e-3 of the state's largest) on all but `max_outliers` rays, which must still agree to 1e-3"""
    flips = int(np.sum(got["status"] != ref["status"]))
    assert flips <= max_flips, f"{flips} status flips"
    same = (got["status"] == ref["status"]) & (ref["status"] != 1)
    if r_horizon is not None:
        same &= ref["x"][:, 1] > 1.05 * r_horizon
    worst = np.abs(got["lambda_max"][same] / ref["lambda_max"][same] - 1.0)
    for f in ("x", "v"):
        a, b = got[f][same], ref[f][same]
        scale = np.maximum(np.abs(b), 1e-3 * np.max(np.abs(b), axis=1, keepdims=True))
        worst = np.maximum(worst, np.max(np.abs(a - b) / scale, axis=1))
    assert int(np.sum(worst >= x_rtol)) <= max_outliers, (int(np.sum(worst >= x_rtol)), float(worst.max()))
    assert worst.max() < 1e-3


def test_compiled_endpoints_vs_oracle_kernel_logic(G, oracle, cm_bump):
    """the 24 x 24 plane of test_tabulated_endpoints_vs_oracle_kernel_logic through the generated body on the host build of the
    integrator: with no fit error the compiled route meets what the table meets"""
    W = H = 24
    disc = (3.0, 400.0)
    cfg = G.render_configuration(cm_bump, X_FAR, G.ThinDisc(*disc), 2000.0, image_width=W, image_height=H,
                                 alpha_lims=(-60, 60), beta_lims=(-35, 35))
    c, pl = cfg.abi_config(), cfg.abi_plane()
    assert c.metric_id >= 12
    rg = G._lib.gr_range(0, W * H, W * H, 1)
    got = np.zeros(W * H, dtype=G._lib.POINT_DTYPE)
    assert _harness(cm_bump.trace).hu_render_endpoints(C.byref(c), C.byref(pl), C.byref(rg), C.c_void_p(got.ctypes.data)) == 0
    ocfg = oracle.make_config("test-bump", BUMP, disc=disc, lambda_max=2000.0)
    assert ocfg.r_inner == pytest.approx(cfg.chart.inner_radius, rel=1e-14) and ocfg.r_outer == cfg.chart.outer_radius
    with oracle.user_metric_library():
        vs = oracle.render_velocities(ocfg, X_FAR, (-60, 60), (-35, 35), W, H)
        ref = oracle.trace(ocfg, X_FAR, vs)
    _compare_endpoints(got, ref, max_flips=2, x_rtol=1e-6)


# ---- the tracer ----
@pytest.mark.parametrize("why, f", [
    ("a branch", lambda r, th: (-(1.0 - 2.0 / r) if r > 2.0 else -1.0, 1.0, r * r, r * r, 0.0)),
    ("a comparison", lambda r, th: (-(1.0 - 2.0 / r) * (r >= 3.0), 1.0, r * r, r * r, 0.0)),
    ("a truth value", lambda r, th: (-1.0 if not r else -2.0, 1.0, r * r, r * r, 0.0)),
    ("np.maximum", lambda r, th: (-np.maximum(r, 2.0), 1.0, r * r, r * r, 0.0)),
    ("np.sin(r)", lambda r, th: (-1.0, 1.0, r * r, r * r * np.sin(r), 0.0)),
    ("np.cos(2 θ)", lambda r, th: (-1.0, 1.0, r * r, r * r * np.cos(2.0 * th), 0.0)),
    ("θ itself", lambda r, th: (-1.0, 1.0, r * r, r * r * th, 0.0)),
    ("np.tanh", lambda r, th: (-np.tanh(r), 1.0, r * r, r * r, 0.0)),
    ("math.sqrt", lambda r, th: (-math.sqrt(r), 1.0, r * r, r * r, 0.0)),
    ("a float power", lambda r, th: (-(r ** 0.5), 1.0, r * r, r * r, 0.0)),
    ("four components", lambda r, th: (-1.0, 1.0, r * r, r * r)),
    ("not a tuple", lambda r, th: r),
])
def test_tracer_refuses_what_a_component_body_cannot_say(G, why, f):
    with pytest.raises(G.UntraceableMetric) as e:
        _trace(G, f)
    assert "TabulatedMetric" in str(e.value) and "breaks" in str(e.value), why


def test_tracer_is_deterministic_and_hash_follows_the_constants(G):
    a, b = _trace(G, bump_components), _trace(G, bump_components)
    assert a.source == b.source and a.source.encode() == b.source.encode() and a.sha256 == b.sha256
    other = _trace(G, lambda r, th: bump_components(r, th, (1.0, 0.9, 0.08, 6.0, 2.5)))
    assert other.sha256 != a.sha256
    # straight-line SSA: one statement per line, temporaries, division as a product with inv_, 17-digit literals
    assert "inv_(" in a.source and " / " not in a.source and "0.81000000000000005" in a.source and a.source.count("dput(g[") == 5
    # common sub-expressions are one temporary: Σ of the bump metric is computed once
    body = [l for l in a.source.splitlines() if l.startswith("const auto")]
    assert len(body) == len(set(l.split("=", 1)[1] for l in body))


def test_host_side_quantities_come_from_the_callable(G):
    """metric_components and the generic ISCO of a CompiledMetric are the callable's own (no table, no fit, no module needed)"""
    cm = G.CompiledMetric(kerr_callable, inner_radius=1.0 + math.sqrt(1.0 - 0.998 ** 2))
    km = G.KerrMetric(1.0, 0.998)
    np.testing.assert_allclose(cm.metric_components(5.0, 1.0), km.metric_components(5.0, 1.0), rtol=1e-14)
    assert cm.isco() == pytest.approx(km.isco(), rel=1e-9)
    cat = G.CompiledMetric(G.JohannsenMetric(*JOH))          # a catalogue metric's own formula is recorded
    np.testing.assert_allclose(cat.metric_components(4.0, 0.7), G.JohannsenMetric(*JOH).metric_components(4.0, 0.7), rtol=1e-14)
    assert cat.inner_radius() == G.JohannsenMetric(*JOH).inner_radius()
    with pytest.raises(ValueError):
        G.CompiledMetric(kerr_callable)          # a bare callable must bring its horizon


# ---- the module ----
def test_module_exports_every_launcher_and_says_what_it_is(G, cm_bump):
    import __graft_entry__ as E
    from gradus_jl_amd import compiled_metric as CM

    path = cm_bump.compile()
    assert os.path.dirname(path) == MODULES and os.path.basename(path) == cm_bump.sha256 + ".so"
    names = {l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines() if l.strip()}
    for fn in CM.MODULE_LAUNCHERS + ("gr_user_module_info",):
        assert fn in names, fn
    assert not any(n.startswith("gr32_") for n in names)          # no fp32 flavour
    info = CM.module_info(path)
    assert info == {"abi_version": G._lib.ABI_VERSION, "metric_id": 12, "build_id": cm_bump.build_id, "header_hash": E.csrc_hash()}
    assert info["build_id"] != 0


def test_second_construction_starts_no_compiler(G, cm_bump, monkeypatch):
    path = cm_bump.compile()
    calls = []
    real_popen = subprocess.Popen

    class Counting(real_popen):
        def __init__(self, args, *a, **kw):
            calls.append(args)
            super().__init__(args, *a, **kw)

    monkeypatch.setattr(subprocess, "Popen", Counting)
    again = G.CompiledMetric(bump_components, inner_radius=R_H_BUMP, isco=cm_bump.isco(), cache_dir=MODULES)
    assert again.compile() == path
    assert again.metric_id == cm_bump.metric_id          # ... and the process loads a module once
    assert calls == [], calls


def test_module_compiled_against_other_sources_is_refused(G, cm_bump, tmp_path):
    import __graft_entry__ as E

    L = G._lib.load()
    blob = open(cm_bump.compile(), "rb").read()
    h = bytes.fromhex(E.csrc_hash())
    h = b"".join(h[8 * k:8 * k + 8][::-1] for k in range(4))          # four little-endian words (gr_user_module_info_t.header_hash)
    assert blob.count(h) == 1
    bad = tmp_path / "altered.so"
    bad.write_bytes(blob.replace(h, h[:-1] + bytes([h[-1] ^ 1])))
    mid = C.c_int64(0)
    rc = L.gr_metric_module_load(str(bad).encode(), C.byref(mid))
    assert rc == -1 and mid.value == -1 and b"other kernel sources" in L.gr_last_error()
    rc = L.gr_metric_module_load(str(tmp_path / "missing.so").encode(), C.byref(mid))
    assert rc == -1
    rc = L.gr_metric_module_load(G._lib.LIB_PATH.encode(), C.byref(mid))          # a shared object that is no module
    assert rc == -1 and b"gr_user_module_info" in L.gr_last_error()
    assert L.gr_metric_module_unload(12 + 15) == -1 and L.gr_metric_module_unload(11) == -1
