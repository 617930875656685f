"""Transfer functions integrated into line profiles and lag-energy matrices: a CunninghamTransferGrid (and a point of a
CunninghamTransferTable) is integrable on the host, and the device's arithmetic (gradus.jl_amd/csrc/gr_tfint.hpp, what k_tf runs
per annulus and g bin) compiled for the host agrees with the host route `integrate_lineprofile` / `integrate_lagtransfer` and with
an independent scalar restatement of src/transfer-functions/integration.jl:74-200,336-453.

Measured on these shapes (23 radii, 12-16 knots, 60 g bins, 96 t bins, 200 / 120 annuli), in units of the peak: harness against
host route 5.3e-16 (line profile) and 2.9e-16 (lag), restatement against host route 1.3e-16 and 1.5e-16; 6527 and 5668 deposits,
none moved across a t edge.  The bound of every comparison is 1e-12 of the peak."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import harness_tfint as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def TF(G):
    return G.transfer_functions


@pytest.fixture(scope="module")
def synth(TF):
    """the ragged synthetic branches and the host route's two results on them.  Read-only."""
    tfs = H.synthetic_branches(TF)
    assert tfs.radii.size == 23 and {b.lower_g.size for b in tfs.branches} | {b.upper_g.size for b in tfs.branches} <= set(range(12, 17))
    assert any(b.lower_g.size != b.upper_g.size for b in tfs.branches)
    line = TF.integrate_lineprofile(H.emissivity, tfs, H.G_GRID, n_radii=200)
    lag = TF.integrate_lagtransfer(H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0)
    return tfs, line, lag


# ---------------------------------------------------------------------------------------------------------------
# a grid is integrable
# ---------------------------------------------------------------------------------------------------------------
def test_grid_with_the_branches_own_knots_equals_the_branch_route(TF):
    knots = np.concatenate([[0.0], np.sort(np.random.default_rng(3).uniform(2e-3, 1 - 2e-3, 13)), [1.0]])
    tfs = H.synthetic_branches(TF, shared_knots=knots)
    col = lambda key: np.stack([getattr(b, key) for b in tfs.branches], axis=1)
    grid = TF.CunninghamTransferGrid(tfs.radii.copy(), knots, tfs.gmin.copy(), tfs.gmax.copy(), col("lower_f"), col("upper_f"),
                                     col("lower_t"), col("upper_t"))
    want = TF.integrate_lineprofile(H.emissivity, tfs, H.G_GRID, n_radii=200)
    got = TF.integrate_lineprofile(H.emissivity, grid, H.G_GRID, n_radii=200)
    print(f"grid against branches, line profile: {H.line_error(got, want):.3e} of the peak")
    assert H.line_error(got, want) <= H.TOL
    want = TF.integrate_lagtransfer(H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0)
    got = TF.integrate_lagtransfer(H.Profile(), grid, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0)
    err, moved = H.lag_error(got, want, 6000)
    print(f"grid against branches, lag: {err:.3e} of the peak, {moved} moved")
    assert err <= H.TOL
    # .at itself: what InterpolatingTransferBranches.at returns, and _last set the same way
    gs = np.array([0.0, 0.013, 0.4, 0.77, 1.0])
    for r in (1.3, 2.2, 17.0, 50.0, 60.0):
        a, b = tfs.at(r), grid.at(r)
        assert a[0] == b[0] and a[1] == b[1]
        np.testing.assert_allclose(b[2](gs), a[2](gs), rtol=1e-14)
        assert set(grid._last) == set(tfs._last) == {"lower_f", "upper_f", "lower_t", "upper_t"}
        for key in grid._last:
            np.testing.assert_allclose(grid._last[key](gs), tfs._last[key](gs), rtol=1e-14)


def test_transfer_function_grid_and_a_table_point_are_integrable(TF):
    """integrate_lineprofile(ε, table(a, θ)) is what a spectral fit evaluates per iteration"""
    corners = [H.synthetic_branches(TF, seed=s) for s in (1, 2, 3, 4)]
    grids = np.empty((2, 2), dtype=object)
    for k, tfs in enumerate(corners):
        grids[k // 2, k % 2] = TF.transfer_function_grid(tfs, Ng=20)
    table = TF.CunninghamTransferTable((np.array([0.0, 0.998]), np.array([30.0, 60.0])), grids)
    g = grids[0, 0]
    assert g.lower_f.shape == (20, 23)
    line = TF.integrate_lineprofile(H.emissivity, g, H.G_GRID, n_radii=100)
    # resampling 12-16 knots on 20 changes the curves a little, not the profile's shape
    assert H.line_error(line, TF.integrate_lineprofile(H.emissivity, corners[0], H.G_GRID, n_radii=100)) < 0.05
    point = table(0.4, 41.0)
    assert isinstance(point, TF.CunninghamTransferGrid)
    mid = TF.integrate_lineprofile(H.emissivity, point, H.G_GRID, n_radii=100)
    assert mid.shape == H.G_GRID.shape and np.all(np.isfinite(mid)) and mid[-1] == 0.0
    assert mid[:-1].sum() == pytest.approx(1.0, rel=1e-12)
    lag = TF.integrate_lagtransfer(H.Profile(), point, H.G_GRID, H.T_GRID, n_radii=60, t0=3.0)
    assert lag.shape == (61, 97) and lag[:-1].sum() == pytest.approx(1.0, rel=1e-12) and np.all(lag[-1] == 0.0)
    # the harness takes a grid through the same packer (replicated knots)
    got, _ = H.harness_lineprofile(TF, H.emissivity, point, H.G_GRID, n_radii=100)
    assert H.line_error(got, mid) <= H.TOL
    got, n_dep = H.harness_lagtransfer(TF, H.Profile(), point, H.G_GRID, H.T_GRID, n_radii=60, t0=3.0)
    assert H.lag_error(got, lag, n_dep)[0] <= H.TOL


# ---------------------------------------------------------------------------------------------------------------
# the device's arithmetic against the host route and the restatement
# ---------------------------------------------------------------------------------------------------------------
def test_line_profile_three_voices(TF, synth):
    tfs, host, _ = synth
    got, n_dep = H.harness_lineprofile(TF, H.emissivity, tfs, H.G_GRID, n_radii=200)
    third = H.restated_lineprofile(tfs, H.emissivity, H.G_GRID, n_radii=200)
    e1, e2, e3 = H.line_error(got, host), H.line_error(third, host), H.line_error(got, third)
    print(f"line profile, of the peak: harness - host {e1:.3e}, restatement - host {e2:.3e}, harness - restatement {e3:.3e}; {n_dep} deposits")
    assert n_dep > 5000
    assert e1 <= H.TOL and e2 <= H.TOL and e3 <= H.TOL
    assert got[-1] == 0.0 and got[0] == 0.0 and host[0] == 0.0          # the first bin lies below every gmin


def test_lag_matrix_three_voices(TF, synth):
    tfs, _, host = synth
    got, n_dep = H.harness_lagtransfer(TF, H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0)
    third, n_third = H.restated_lagtransfer(tfs, H.Profile(), H.G_GRID, H.T_GRID, n_radii=120, t0=3.0)
    assert n_dep == n_third > 5000
    (e1, m1), (e2, m2), (e3, m3) = H.lag_error(got, host, n_dep), H.lag_error(third, host, n_dep), H.lag_error(got, third, n_dep)
    print(f"lag, of the peak (moved deposits): harness - host {e1:.3e} ({m1}), restatement - host {e2:.3e} ({m2}), "
          f"harness - restatement {e3:.3e} ({m3}); {n_dep} deposits")
    assert e1 <= H.TOL and e2 <= H.TOL and e3 <= H.TOL
    # deposits past the last t edge are dropped, those before the first land in column 0
    assert host[:, 0].sum() > 0 and np.count_nonzero(host) > 1000


def test_the_pair_rule_accepts_one_moved_deposit_and_nothing_else():
    want = np.zeros((4, 6))
    want[1, 2], want[1, 3], want[2, 4] = 1.0, 0.5, 0.25
    moved = want.copy()
    moved[1, 2] -= 0.125
    moved[1, 3] += 0.125
    assert H.lag_error(moved, want, 1000) == (0.0, 1)
    lost = want.copy()
    lost[1, 2] -= 0.125
    with pytest.raises(AssertionError):
        H.lag_error(lost, want, 1000)
    uneven = moved.copy()
    uneven[1, 3] += 1e-9
    with pytest.raises(AssertionError):
        H.lag_error(uneven, want, 1000)
    two = moved.copy()
    two[2, 4] -= 0.1
    two[2, 5] += 0.1
    with pytest.raises(AssertionError):
        H.lag_error(two, want, 1000)


def test_a_set_gives_the_same_bits_alone_and_in_a_batch(TF):
    a, b = H.synthetic_branches(TF, seed=1), H.synthetic_branches(TF, seed=2, knots=(5, 9))
    eps = [H.emissivity, lambda r: r ** -2.0, H.emissivity]
    c = H.Calls()
    batch = TF.integrate_lineprofiles(eps, [a, b, a], H.G_GRID, rmin=[None, 2.0, 3.0], rmax=40.0, n_radii=70, ensemble=None, _call=c.line)
    assert batch.shape == (3, 61)
    for k, (ε, tfs, r0) in enumerate(zip(eps, [a, b, a], [None, 2.0, 3.0])):
        one = TF.integrate_lineprofiles([ε], [tfs], H.G_GRID, rmin=r0, rmax=40.0, n_radii=70, ensemble=None, _call=c.line)[0]
        assert one.tobytes() == batch[k].tobytes()
    assert batch[0].tobytes() != batch[2].tobytes()
    with pytest.raises(ValueError, match="one per set"):
        TF.integrate_lineprofiles(eps, [a, b, a], H.G_GRID, rmin=[1.0, 2.0], ensemble=None, _call=c.line)


# ---------------------------------------------------------------------------------------------------------------
# integrate_bin, branch by branch, per bin against transfer_functions._integrate_bins
# ---------------------------------------------------------------------------------------------------------------
def host_bin(TF, tfs, r, mode, lo, hi, h):
    gmin, gmax, both = tfs.at(r)
    br = tfs._last
    span = gmax - gmin
    fb = both if mode == 0 else (lambda gs: np.where(np.isnan(br[("lower_f", "upper_f")[mode - 1]](gs)), 0.0, br[("lower_f", "upper_f")[mode - 1]](gs)))

    def S(g):
        gs = (g - gmin) / span
        with np.errstate(all="ignore"):
            return (g * g) * fb(gs) * g / np.sqrt(gs * (1.0 - gs))

    X, W = np.polynomial.legendre.leggauss(7)
    glo, ghi = np.clip(lo, gmin, gmax), np.clip(hi, gmin, gmax)
    if glo == ghi:
        return 0.0
    return float(TF._integrate_bins(S, np.array([lo]), np.array([hi]), gmin, gmax, h, X, W)[0])


@pytest.mark.parametrize("case", ["below gmin", "above gmax", "straddles h", "inside h", "straddles 1 - h", "inside 1 - h",
                                  "interior", "straddles gmin", "whole range"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_integrate_bin_case_by_case(TF, case, mode):
    h = 1e-3          # wide enough that a bin can lie wholly inside an edge
    tfs = H.synthetic_branches(TF)
    r_int = np.array([1.3, 1.9, 4.4, 21.0, 50.0])
    for ia, r in enumerate(r_int):
        gmin, gmax, _ = tfs.at(r)
        span = gmax - gmin
        at = lambda s: gmin + span * s
        lo, hi = {"below gmin": (gmin - 0.2, gmin - 0.1), "above gmax": (gmax + 0.01, gmax + 0.3),
                  "straddles h": (at(0.2 * h), at(0.3)), "inside h": (at(0.1 * h), at(0.7 * h)),
                  "straddles 1 - h": (at(0.6), at(1 - 0.3 * h)), "inside 1 - h": (at(1 - 0.8 * h), at(1 - 0.2 * h)),
                  "interior": (at(0.31), at(0.52)), "straddles gmin": (gmin - 0.1, at(0.2)), "whole range": (gmin - 0.1, gmax + 0.1)}[case]
        got, ann = H.integrate_bin(TF, tfs, r_int, ia, mode, lo, hi, h=h)
        assert ann[0] == gmin and ann[1] == gmax
        want = host_bin(TF, tfs, r, mode, lo, hi, h)
        if case in ("below gmin", "above gmax"):
            assert got == 0.0 and want == 0.0
        else:
            assert want > 0.0 and got == pytest.approx(want, rel=1e-13)


def test_annulus_weight_is_the_host_routes(TF):
    tfs = H.synthetic_branches(TF)
    r_int = np.array([1.5, 1.9, 4.4, 21.0])
    for ia, r in enumerate(r_int):
        _, ann = H.integrate_bin(TF, tfs, r_int, ia, 0, 0.5, 0.6)
        gmin, gmax, _ = tfs.at(r)
        r_prev = r_int[0] - (r_int[1] - r_int[0]) if ia == 0 else r_int[ia - 1]
        assert ann[2] == (r - r_prev) * r * 1.0 * math.pi / (gmax - gmin)


def test_nan_knot_values_count_as_the_interpolator_has_them(TF):
    """a NaN f at a knot: NaNLinearInterpolator falls back to the nearer knot, a NaN pair gives 0 (_zero_if_nan)"""
    tfs = H.synthetic_branches(TF, nan_f=[(3, "lower", 4), (3, "lower", 5), (9, "upper", 2), (10, "upper", 7)])
    assert np.isnan(tfs.branches[3].lower_f[4]) and np.isnan(tfs.branches[9].upper_f[2])
    host = TF.integrate_lineprofile(H.emissivity, tfs, H.G_GRID, n_radii=200)
    got, _ = H.harness_lineprofile(TF, H.emissivity, tfs, H.G_GRID, n_radii=200)
    third = H.restated_lineprofile(tfs, H.emissivity, H.G_GRID, n_radii=200)
    print(f"NaN knots, of the peak: harness - host {H.line_error(got, host):.3e}, restatement - host {H.line_error(third, host):.3e}")
    assert H.line_error(got, host) <= H.TOL and H.line_error(third, host) <= H.TOL
    lag = TF.integrate_lagtransfer(H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0)
    got, n_dep = H.harness_lagtransfer(TF, H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0)
    assert H.lag_error(got, lag, n_dep)[0] <= H.TOL


def test_a_single_bin_and_a_scaled_axis(TF, synth):
    tfs = synth[0]
    for g_grid, scale in ((np.array([0.3, 1.4]), 1.0), (np.array([0.7, 0.9]), 1.0), (6.4 * H.G_GRID, 6.4)):
        host = TF.integrate_lineprofile(H.emissivity, tfs, g_grid, n_radii=50, g_scale=scale)
        got, _ = H.harness_lineprofile(TF, H.emissivity, tfs, g_grid, n_radii=50, g_scale=scale)
        assert H.line_error(got, host) <= H.TOL and got[-1] == 0.0
        lag = TF.integrate_lagtransfer(H.Profile(), tfs, g_grid, H.T_GRID, n_radii=50, g_scale=scale)
        got, n_dep = H.harness_lagtransfer(TF, H.Profile(), tfs, g_grid, H.T_GRID, n_radii=50, g_scale=scale)
        assert H.lag_error(got, lag, n_dep)[0] <= H.TOL


# ---------------------------------------------------------------------------------------------------------------
# the C ABI: refusals before the device, header <-> exports <-> ctypes
# ---------------------------------------------------------------------------------------------------------------
def test_argument_checks_come_before_the_device(G, TF, synth):
    """Every refusal of gr_tf_lineprofile / gr_tf_lagtransfer, without a context"""
    from gradus_jl_amd import _lib

    L = _lib.load()
    tfs = synth[0]
    r_int = np.linspace(2.0, 40.0, 8)
    X, W = np.polynomial.legendre.leggauss(7)
    g, t = H.G_GRID, H.T_GRID
    out = np.zeros((g.size, t.size))

    def make(**change):
        s, keep = TF._tf_set(tfs, r_int, np.ones(8), np.zeros(8), 2.0, 1.0)
        for k, v in change.items():
            setattr(s, k, v)
        return s, keep

    def quad(n=7, x=X, w=W):
        return _lib.gr_tfquad(1e-8, n, x.ctypes.data if x is not None else None, w.ctypes.data if w is not None else None)

    def line(s, q=None, n_sets=1, g_=g, n_g=None, out_=out):
        q = quad() if q is None else q
        return L.gr_tf_lineprofile(None, C.byref(s) if s is not None else None, n_sets, C.byref(q) if q != "null" else None,
                                   g_.ctypes.data if g_ is not None else None, g.size if n_g is None else n_g,
                                   out_.ctypes.data if out_ is not None else None)

    def lag(s, q=None, n_sets=1, g_=g, n_g=None, t_=t, n_t=None, out_=out):
        q = quad() if q is None else q
        return L.gr_tf_lagtransfer(None, C.byref(s) if s is not None else None, n_sets, C.byref(q) if q != "null" else None,
                                   g_.ctypes.data if g_ is not None else None, g.size if n_g is None else n_g,
                                   t_.ctypes.data if t_ is not None else None, t.size if n_t is None else n_t,
                                   out_.ctypes.data if out_ is not None else None)

    def refused(rc, text):
        assert rc == -1 and text in L.gr_last_error().decode(), L.gr_last_error().decode()

    s, keep = make()
    refused(line(s), "ctx is null")                          # (everything else in order)
    refused(lag(s), "ctx is null")
    for call in (line, lag):
        refused(call(None), "sets is null")
        refused(call(s, q="null"), "quad is null")
        refused(call(s, g_=None), "g edges are null")
        refused(call(s, out_=None), "out is null")
        refused(call(s, n_sets=0), "n_sets must be at least 1")
        refused(call(s, n_g=1), "g axis: at least two edges")
        refused(call(s, q=quad(x=None)), "nodes / weights are null")
        refused(call(s, q=quad(w=None)), "nodes / weights are null")
        refused(call(s, q=quad(n=0)), "n_q must be in 1 ... 32")
        refused(call(s, q=quad(n=33)), "n_q must be in 1 ... 32")
        refused(call(make(n_r=1)[0]), "n_r >= 2")
        refused(call(make(n_int=1)[0]), "n_int >= 2")
        for field in ("radii", "gmin", "gmax", "off", "knot_g", "knot_f", "knot_t"):
            refused(call(make(**{field: None})[0]), "a transfer-function array is null")
        for field in ("r_int", "eps_int"):
            refused(call(make(**{field: None})[0]), "an annulus array is null")
        off = keep[3].copy()
        off[5] = off[4] + 1
        refused(call(make(off=off.ctypes.data)[0]), "a branch needs 2 ... 1024 knots")
        off = keep[3].copy()
        off[6:] += 1100
        refused(call(make(off=off.ctypes.data)[0]), "a branch needs 2 ... 1024 knots")
        off = keep[3].copy()
        off[7] = off[6] - 3
        refused(call(make(off=off.ctypes.data)[0]), "offsets must ascend")
        off = keep[3].copy() - 1
        refused(call(make(off=off.ctypes.data)[0]), "off[0] >= 0")
        refused(call(s, n_g=(1 << 24) + 1), "2^24 cells")
    refused(lag(s, t_=None), "t edges are null")
    refused(lag(s, n_t=1), "t axis: at least two edges")
    refused(lag(make(tsd_int=None)[0]), "an annulus array is null")
    refused(lag(s, n_g=4097, n_t=4096), "2^24 cells")
    refused(line(s, n_sets=1 << 20, n_g=17), "2^24 cells")
    assert line(make(tsd_int=None)[0]) == -1 and "ctx is null" in L.gr_last_error().decode()      # a line profile needs no times


def c_struct(hdr, name):
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            m = re.match(r"(const )?(int32_t|int64_t|double)\s*(\*)?\s*(\w+)$", decl)
            assert m, decl
            fields.append((m.group(4), "ptr" if m.group(3) else {"int32_t": "i32", "int64_t": "i64", "double": "f64"}[m.group(2)]))
    return fields


def test_header_exports_and_ctypes_agree(G):
    from gradus_jl_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "gradus_mi355x.h"), encoding="utf-8").read()
    assert re.search(r"#define GR_ABI_VERSION (\d+)", hdr).group(1) == "8" == str(_lib.ABI_VERSION)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("gr_tf_lineprofile", "gr_tf_lagtransfer"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(r"int32_t " + name + r"\(gr_ctx\* ctx, const gr_tfset\* sets,", hdr)
    kind = {C.c_int32: "i32", C.c_int64: "i64", C.c_double: "f64", C.c_void_p: "ptr"}
    for name in ("gr_tfset", "gr_tfquad"):
        got = [(f, kind[t]) for f, t in getattr(_lib, name)._fields_]
        assert got == c_struct(hdr, name), name
    assert C.sizeof(_lib.gr_tfset) == 14 * 8 and C.sizeof(_lib.gr_tfquad) == 4 * 8
    assert "gradus.jl_amd/csrc/gr_tfint.hpp" in open(os.path.join(ROOT, "gradus.jl_amd", "_lib.py"), encoding="utf-8").read()
    assert '"tf_chunk"' in hdr
