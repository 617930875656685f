"""The lag transfer function of a time-dependent emissivity (RingCoronaProfile / DiscCoronaProfile; radial.jl:164-324,
ring.jl:857-950) on the host: the profile types against small cases worked by hand, the host route `integrate_lagtransfer`
against an independent scalar restatement and against the device's arithmetic (gradus.jl_amd/csrc/gr_tftd.hpp, what k_tftd_em
and k_tftd run) compiled for the host, a spike in time against the ordinary route, and the refusals of gr_tf_lagtransfer_td.

Measured on these shapes (23 radii, 37 annuli, a disc of three rings with arms of 2 ... 1024 slices), in units of the peak:
harness against host route 1.7e-16 ... 9.0e-16, restatement against host route 2.2e-16 (disc) and 5.1e-16 (its first ring alone),
no deposit moved across a t edge; the harness's ε(time) table equals the host's bit for bit.  The bound of every comparison of two routes is 1e-12 of the peak.
The spike: DESIGN_measurements.md M25."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import harness_tfint as H
import harness_tftd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def TF(G):
    return G.transfer_functions


# ---------------------------------------------------------------------------------------------------------------
# the profile types
# ---------------------------------------------------------------------------------------------------------------
def small_arm(G, curves):
    return G.TimeDependentRadialDiscProfile(np.ones(len(curves)), [c[0] for c in curves], [c[1] for c in curves], [c[2] for c in curves])


def test_an_arm_sorts_its_slices_by_time_stably_with_nan_last(G):
    # at ρ = 2: slice 0 gives t = 5, slice 1 misses (NaN), slice 2 gives t = 3, slice 3 gives t = 5 again (a tie, after slice 0)
    arm = small_arm(G, [([1.0, 3.0], [4.0, 6.0], [10.0, 30.0]), ([2.5, 3.0], [0.0, 1.0], [1.0, 1.0]),
                        ([0.0, 4.0], [1.0, 5.0], [7.0, 9.0]), ([2.0, 4.0], [5.0, 9.0], [40.0, 80.0])])
    f = arm.emissivity_interp(2.0)
    assert f.t[:3].tolist() == [3.0, 5.0, 5.0] and np.isnan(f.t[3])
    assert f.u[:3].tolist() == [8.0, 20.0, 40.0] and np.isnan(f.u[3])
    assert arm.emissivity_interp_limits(2.0) == (3.0, 5.0)
    assert f(4.0) == 14.0                                        # halfway between (3, 8) and (5, 20)
    assert arm.emissivity_at(2.0) == 20.0 + 8.0 + 40.0           # the slices that cover ρ
    assert arm.emissivity_interp_limits(10.0) == (0.0, 0.0)      # nothing covers ρ = 10
    assert G.emissivity_interp_limits(arm, 3.5) == (4.5, 8.0) and G.emissivity_interp(arm, 3.5).t[:2].tolist() == [4.5, 8.0]
    # the same ranks from the header
    t = np.array([5.0, np.nan, 3.0, 5.0, np.nan, -1.0])
    ranks = [T.lib().htftd_rank(C.c_void_p(t.ctypes.data), C.c_int(t.size), C.c_int(i)) for i in range(t.size)]
    assert ranks == np.argsort(np.argsort(t, kind="stable"), kind="stable").tolist() == [2, 4, 1, 3, 5, 0]


def test_a_ring_drops_an_arm_that_misses_a_slice(G):
    left = small_arm(G, [([1.0, 5.0], [2.0, 6.0], [1.0, 1.0]), ([1.0, 5.0], [4.0, 8.0], [3.0, 3.0])])
    right = small_arm(G, [([1.0, 5.0], [1.0, 5.0], [10.0, 10.0]), ([1.0, 2.0], [3.0, 4.0], [20.0, 20.0])])
    ring = G.RingCoronaProfile(left, right)
    # ρ = 1.5: both arms whole.  left knots (2.5, 1), (4.5, 3); right knots (1.5, 10), (3.5, 20)
    f = ring.emissivity_interp(1.5)
    assert ring.emissivity_interp_limits(1.5) == (1.5, 4.5)
    assert f(3.0) == (1.0 + 0.25 * 2.0) + (10.0 + 0.75 * 10.0)
    assert f(2.0) == 0.0 + 12.5 and f(4.0) == 2.5 + 0.0 and f(5.0) == 0.0      # each arm between its own knots only
    assert f(np.array([2.0, 4.0, 5.0])).tolist() == [12.5, 2.5, 0.0]
    # ρ = 3: slice 1 of the right arm misses, so the right arm is 0 at every time -- but its other slice still sets the limits
    f = ring.emissivity_interp(3.0)
    assert ring.emissivity_interp_limits(3.0) == (3.0, 6.0)
    assert f(3.0) == 0.0 and f(5.0) == 2.0 and f(3.5) == 0.0
    assert ring.emissivity_at(3.0) == (1.0 + 3.0) + 10.0
    assert ring.emissivity_interp_limits(7.0) == (0.0, 0.0) and ring.emissivity_interp(7.0)(0.0) == 0.0


def test_a_disc_weighs_and_delays_its_rings(G):
    arm = lambda t0, e: small_arm(G, [([1.0, 5.0], [t0, t0], [e, e]), ([1.0, 5.0], [t0 + 2.0, t0 + 2.0], [e, e])])
    rings = [G.RingCoronaProfile(arm(1.0, 1.0), arm(1.0, 2.0)), G.RingCoronaProfile(arm(2.0, 10.0), arm(7.0, 20.0)),
             G.RingCoronaProfile(arm(0.0, 100.0), small_arm(G, [([8.0, 9.0], [0.0, 0.0], [1.0, 1.0])] * 2))]
    disc = G.DiscCoronaProfile([2.0, 2.5, 3.0], rings)
    assert [disc._ring_weighting(i) for i in range(3)] == [1.0, 1.25, 1.5]
    assert disc.emissivity_interp_limits(2.0) == (0.0, 9.0)      # ring 2's right arm covers nothing: (0, 0) joins the fold
    f = disc.emissivity_interp(2.0)
    assert f(2.5) == (1.0 + 2.0) * 1.0 + (10.0 + 0.0) * 1.25 + (0.0 + 0.0) * 1.5
    assert f(1.5) == 3.0 * 1.0 + 0.0 + 100.0 * 1.5
    assert disc.emissivity_at(2.0) == (2.0 + 4.0) * 1.0 + (20.0 + 40.0) * 1.25 + 200.0 * 1.5
    late = disc.with_propagation_velocity(lambda r: 2.0 * r)     # delays 4, 5, 6
    assert late.rings is not disc.rings or late.radii is disc.radii
    assert late.emissivity_interp_limits(2.0) == (5.0, 14.0)
    g = late.emissivity_interp(2.0)
    assert g(6.5) == f(2.5 - 0.0) - 12.5 - 0.0 + 150.0 and g(6.5) == 3.0 * 1.0 + 0.0 * 1.25 + 100.0 * 1.5      # x - dt = 2.5, 1.5, 0.5
    assert disc.emissivity_interp_limits(2.0) == (0.0, 9.0)      # the original keeps its zero delay
    with pytest.raises(ValueError, match="at least 2 rings"):
        G.DiscCoronaProfile([2.0], rings[:1])


def test_time_samples_are_numpys_linspace():
    f = T.lib().htftd_time_sample
    for a, b, n in ((1.7, 11.06852815, 100), (0.0, 0.0, 33), (3.25, 3.25, 2), (-2.0, 1e-320, 7), (8.884017, 18.8748763, 2), (0.1, 0.7, 33)):
        want = np.linspace(a, b, n)
        got = [f(C.c_double(a), C.c_double(b), C.c_int(n), C.c_int(k)) for k in range(n)]
        assert got == want.tolist(), (a, b, n)


def test_the_keywords_belong_to_the_time_dependent_profiles(TF):
    tfs = T.branches(TF)
    for kw in ({"g_grid_upscale": 1}, {"n_time_steps": 100}):
        with pytest.raises(NotImplementedError, match="time-dependent"):
            TF.integrate_lagtransfer(H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=10, **kw)


# ---------------------------------------------------------------------------------------------------------------
# the synthetic profiles exercise what they are meant to, by the host route's own types
# ---------------------------------------------------------------------------------------------------------------
def test_the_synthetic_profiles_cover_every_case(G):
    disc = T.disc_profile(G)
    assert sorted(len(arm.radii) for ring in disc.rings for arm in (ring.left_arm, ring.right_arm)) == [2, 5, 9, 12, 70, 1024]
    assert all(disc._delays()) and len(disc.rings) == 3
    left = disc.rings[2].left_arm
    assert left.radii[3].tobytes() == left.radii[4].tobytes() and left.t[3].tobytes() == left.t[4].tobytes()
    for kind, prof in (("disc", disc), ("ring", T.ring_profile(G))):
        radii, _ = T.host_table(G, kind, 33)
        both, one_missing, ring_missing = T.coverage(G, prof, radii)
        print(f"{kind}: of {radii.size} annuli {both} with both arms of a ring active, {one_missing} with an arm switched off by one "
              f"missing slice, {ring_missing} with every slice of a ring missing")
        assert 3 * both >= radii.size and one_missing >= 1
        assert ring_missing >= (1 if kind == "disc" else 0)
    # the tie shows at the annuli: two equal times next to each other in the sorted knots of ring 2's left arm
    ts = left.emissivity_interp(10.0).t
    assert np.count_nonzero(np.diff(ts) == 0.0) == 1


# ---------------------------------------------------------------------------------------------------------------
# three voices
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["disc", "ring"])
def test_restatement_against_the_host_route(G, TF, kind):
    grid, n_time, upscale = "20x48", 33, 3
    host, n_host = T.host_case(G, kind, grid, n_time, upscale)
    prof = T.disc_profile(G) if kind == "disc" else T.ring_profile(G)
    third, n_third = T.restated_lagtransfer(prof, T.branches(TF), *T.GRIDS[grid], n_radii=T.N_RADII, t0=T.T0, g_grid_upscale=upscale,
                                            n_time_steps=n_time)
    err, moved = H.lag_error(third, host, n_host)
    print(f"{kind}, restatement - host: {err:.3e} of the peak, {moved} moved; {n_third} / {n_host} deposits")
    assert n_third == n_host > 20000
    assert err <= T.TOL
    assert host[:-1].sum() == pytest.approx(1.0, rel=1e-12) and np.all(host[-1] == 0.0)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: f"{c[0]}-nt{c[1]}-up{c[2]}")
@pytest.mark.parametrize("kind", ["disc", "ring"])
def test_harness_against_the_host_route(G, TF, kind, case):
    grid, n_time, upscale = case
    host, n_host = T.host_case(G, kind, grid, n_time, upscale)
    prof = T.disc_profile(G) if kind == "disc" else T.ring_profile(G)
    got, n_dep, em = T.harness_lagtransfer(TF, prof, T.branches(TF), *T.GRIDS[grid], t0=T.T0, g_grid_upscale=upscale, n_time_steps=n_time)
    same, rel = T.em_error(em, T.host_table(G, kind, n_time)[1])
    err, moved = H.lag_error(got, host, n_host)
    print(f"{kind} {case}: harness - host {err:.3e} of the peak, {moved} moved, {n_dep} / {n_host} deposits; em limits equal: {same}, "
          f"em values: {rel:.3e} relative")
    assert same and rel <= 1e-14
    assert n_dep == n_host > 500
    assert err <= T.TOL


def test_an_early_t_grid_drops_deposits(G):
    """the same g grid, time samples and annuli: three fine bins deposit three times as often where nothing is dropped"""
    early, whole = T.host_case(G, "disc", "early", 33, 1)[1], T.host_case(G, "disc", "20x48", 33, 3)[1]
    print(f"{early} deposits on the early grid, {whole} / 3 on the whole one")
    assert 3 * early < whole


def test_public_entry_dispatches_on_the_profile(G, TF):
    g, t = T.GRIDS["20x48"]
    flux = TF.integrate_lagtransfer(T.ring_profile(G), T.branches(TF), g, t, n_radii=T.N_RADII, t0=T.T0, g_grid_upscale=3, n_time_steps=33)
    assert flux.tobytes() == T.host_case(G, "ring", "20x48", 33, 3)[0].tobytes()
    with pytest.raises(ValueError, match="n_time_steps"):
        TF.integrate_lagtransfer(T.ring_profile(G), T.branches(TF), g, t, n_radii=T.N_RADII, n_time_steps=1)
    with pytest.raises(ValueError, match="g_grid_upscale"):
        TF.integrate_lagtransfer(T.ring_profile(G), T.branches(TF), g, t, n_radii=T.N_RADII, g_grid_upscale=65)


# ---------------------------------------------------------------------------------------------------------------
# a spike in time is the ordinary lag transfer function
# ---------------------------------------------------------------------------------------------------------------
def spike_profiles(G, width):
    """ε(t) at every radius: a triangle of unit area times E(ρ) around T(ρ), half width `width` -- three slices at T - w, T, T + w
    with ε = 0, E / w, 0 in the left arm, a right arm of zeros inside it -- and the RadialDiscProfile with the same E, T"""
    ρ = 1.0 * 60.0 ** (np.arange(200) / 199.0)
    T_, E = np.sqrt(ρ ** 2 + 25.0), ρ ** -3.0
    zero = np.zeros(ρ.size)
    left = G.TimeDependentRadialDiscProfile(np.ones(3), [ρ] * 3, [T_ - width, T_, T_ + width], [zero, E / width, zero])
    right = G.TimeDependentRadialDiscProfile(np.ones(2), [ρ] * 2, [T_ - 0.5 * width, T_ + 0.5 * width], [zero, zero])
    return G.RingCoronaProfile(left, right), G.RadialDiscProfile(ρ, E, T_)


SPIKE_WIDTH, SPIKE_BOUND = 1e-3, 2 * 2.29e-3     # twice the measured difference (2.29e-3 of the peak, M25)


def test_a_spike_in_time_reproduces_the_ordinary_route(G, TF):
    ring, radial = spike_profiles(G, SPIKE_WIDTH)
    tfs = T.branches(TF)
    want = TF.integrate_lagtransfer(radial, tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0)
    got = TF.integrate_lagtransfer(ring, tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0, n_time_steps=33)
    diff = float(np.max(np.abs(got - want)) / np.max(want))
    row = float(np.max(np.abs(got.sum(axis=1) - want.sum(axis=1))) / np.max(want.sum(axis=1)))
    print(f"spike of half width {SPIKE_WIDTH}: largest cell difference {diff:.3e} of the peak, largest difference of a g row's sum {row:.3e}")
    assert diff <= SPIKE_BOUND
    assert got[:-1].sum() == pytest.approx(1.0, rel=1e-12)


# ---------------------------------------------------------------------------------------------------------------
# the C ABI: refusals before the device, header <-> exports <-> ctypes
# ---------------------------------------------------------------------------------------------------------------
def test_argument_checks_come_before_the_device(G, TF):
    """Every refusal of gr_tf_lagtransfer_td, without a context"""
    from gradus_jl_amd import _lib

    L = _lib.load()
    tfs = T.branches(TF)
    r_int = np.linspace(2.0, 40.0, 8)
    X, W = np.polynomial.legendre.leggauss(7)
    g, t = T.G_SMALL, T.T_SMALL
    out = np.zeros((g.size, t.size))
    s, keep = TF._tf_set(tfs, r_int, np.ones(8), np.zeros(8), 2.0, 1.0)
    s.eps_int = s.tsd_int = None                                  # not read
    p0, keep_p = TF._tftd_profile(T.disc_profile(G))
    fields = [f for f, _ in _lib.gr_tfprofile._fields_]

    def prof(**change):
        p = _lib.gr_tfprofile(*[getattr(p0, f) for f in fields])
        for k, v in change.items():
            setattr(p, k, v)
        return p

    def call(p=p0, s_=s, q="default", g_=g, n_g=None, t_=t, n_t=None, up=1, n_time=33, out_=out, ctx=None):
        q = _lib.gr_tfquad(1e-8, 7, X.ctypes.data, W.ctypes.data) if q == "default" else q
        return L.gr_tf_lagtransfer_td(ctx, C.byref(s_) if s_ is not None else None, C.byref(p) if p is not None else None,
                                      C.byref(q) if q is not None else None, g_.ctypes.data if g_ is not None else None,
                                      g.size if n_g is None else n_g, t_.ctypes.data if t_ is not None else None,
                                      t.size if n_t is None else n_t, up, n_time, 3.0, out_.ctypes.data if out_ is not None else None, None)

    def refused(rc, text):
        assert rc == -1 and text in L.gr_last_error().decode(), L.gr_last_error().decode()

    refused(call(), "ctx is null")                                # (everything else in order; eps_int and tsd_int may be null)
    refused(call(p=None), "prof is null")
    refused(call(s_=None), "sets is null")
    refused(call(q=None), "quad is null")
    refused(call(g_=None), "g edges are null")
    refused(call(t_=None), "t edges are null")
    refused(call(out_=None), "out is null")
    refused(call(n_g=1), "g axis: at least two edges")
    refused(call(n_t=1), "t axis: at least two edges")
    refused(call(q=_lib.gr_tfquad(1e-8, 33, X.ctypes.data, W.ctypes.data)), "n_q must be in 1 ... 32")
    refused(call(n_g=4097, n_t=4096), "2^24 cells")
    bad = TF._tf_set(tfs, r_int, np.ones(8), np.zeros(8), 2.0, 1.0)[0]
    bad.r_int = None
    refused(call(s_=bad), "an annulus array is null")
    for n_time in (1, 0, -5, 1025):
        refused(call(n_time=n_time), "n_time must be in 2 ... 1024")
    for up in (0, -1, 65):
        refused(call(up=up), "g_upscale must be in 1 ... 64")
    for n in (0, -1, 1025):
        refused(call(prof(n_rings=n)), "n_rings must be in 1 ... 1024")
    for f in fields[1:]:
        refused(call(prof(**{f: None})), "an array is null")
    arm_off, curve_off = keep_p[2], keep_p[3]
    a = arm_off.copy()
    a[1] = a[0] + 1                                               # an arm of one curve (and its neighbour one longer)
    refused(call(prof(arm_off=a.ctypes.data)), "an arm needs 2 ... 1024 curves")
    a = arm_off.copy()
    a[3] += 1                                                     # the arm of 1024 curves gets 1025
    refused(call(prof(arm_off=a.ctypes.data)), "an arm needs 2 ... 1024 curves")
    a = arm_off.copy()
    a[2] = a[1] - 1
    refused(call(prof(arm_off=a.ctypes.data)), "arm offsets must ascend")
    a = arm_off.copy() - 1
    refused(call(prof(arm_off=a.ctypes.data)), "arm_off[0] >= 0")
    c = curve_off.copy()
    c[5] = c[4] + 1
    refused(call(prof(curve_off=c.ctypes.data)), "a curve needs at least 2 knots")
    c = curve_off.copy()
    c[7] = c[6] - 2
    refused(call(prof(curve_off=c.ctypes.data)), "curve offsets must ascend")
    c = curve_off.copy() - 1
    refused(call(prof(curve_off=c.ctypes.data)), "curve offsets must ascend from an offset >= 0")


def test_header_exports_and_ctypes_agree(G):
    from gradus_jl_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "gradus_mi355x.h"), encoding="utf-8").read()
    assert re.search(r"#define GR_ABI_VERSION (\d+)", hdr).group(1) == "8" == str(_lib.ABI_VERSION)
    lib = C.CDLL(_lib.LIB_PATH)
    assert "gr_tf_lagtransfer_td" in _lib.EXPORTS and hasattr(lib, "gr_tf_lagtransfer_td")
    assert re.search(r"int32_t gr_tf_lagtransfer_td\(gr_ctx\* ctx, const gr_tfset\* set, const gr_tfprofile\* prof, const gr_tfquad\* quad,", hdr)
    body = re.search(r"typedef struct gr_tfprofile \{(.*?)\} gr_tfprofile;", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S), flags=re.S).group(1)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    names = [re.match(r"(?:const )?(?:int64_t|double)\s*\*?\s*(\w+)$", d).group(1) for d in decls]
    assert names == [f for f, _ in _lib.gr_tfprofile._fields_]
    assert [("*" in d) for d in decls] == [t is C.c_void_p for _, t in _lib.gr_tfprofile._fields_]
    assert C.sizeof(_lib.gr_tfprofile) == 8 * 8
    for path in (os.path.join(ROOT, "gradus.jl_amd", "_lib.py"), os.path.join(ROOT, "__graft_entry__.py")):
        assert "gr_tftd.hpp" in open(path, encoding="utf-8").read()
