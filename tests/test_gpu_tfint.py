"""Transfer functions integrated on the device (integrate_lineprofile / integrate_lagtransfer / integrate_lineprofiles with
`ensemble=`: gr_tf_lineprofile, gr_tf_lagtransfer) against the host route, the numpy loop of transfer_functions.py, on the same
transfer functions.  The bound is 1e-12 of the peak everywhere (harness_tfint.TOL): the host build of the same arithmetic differs
from the host route by 5e-16 (tests/test_tfint_host.py), the rest is margin for the device's sqrt and division.  A lag matrix may
differ beyond that only by a deposit moved across a t edge (harness_tfint.lag_error).

Every parity test prints what it measures before it asserts.  k_tf stages no knots in LDS, so there is no knot count at which
the kernel changes path; the accumulators change path at 40 KB (2560 cells), and both sides of that are run."""
import math

import numpy as np
import pytest

import harness_tfint as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def TF(G):
    return G.transfer_functions


@pytest.fixture(scope="module")
def synth(TF):
    """the ragged synthetic branches of the CPU tests and the host route's results on them.  Read-only."""
    tfs = H.synthetic_branches(TF)
    line = TF.integrate_lineprofile(H.emissivity, tfs, H.G_GRID, n_radii=200)
    lag = TF.integrate_lagtransfer(H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0)
    return tfs, line, lag


def check_line(got, want, what):
    err = H.line_error(got, want)
    print(f"{what}: device - host {err:.3e} of the peak")
    assert err <= H.TOL
    return err


def check_lag(got, want, what, n_deposits=6000):
    err, moved = H.lag_error(got, want, n_deposits)
    print(f"{what}: device - host {err:.3e} of the peak, {moved} deposits moved across a t edge")
    assert err <= H.TOL


def test_line_profile_against_the_host_route(TF, ens, synth):
    tfs, host, _ = synth
    got = TF.integrate_lineprofile(H.emissivity, tfs, H.G_GRID, n_radii=200, ensemble=ens)
    check_line(got, host, "line profile, 23 radii x 12-16 knots, 60 bins, 200 annuli")
    assert got[-1] == 0.0 and got[:-1].sum() == pytest.approx(1.0, rel=1e-12)


def test_lag_matrix_against_the_host_route(TF, ens, synth):
    tfs, _, host = synth
    got = TF.integrate_lagtransfer(H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0, ensemble=ens)
    check_lag(got, host, "lag, 60 x 96 bins, 120 annuli (global accumulators)", 5668)
    assert np.all(got[-1] == 0.0)
    # 20 x 49 bins: the accumulators fit LDS
    g, t = np.linspace(0.3, 1.3, 21), H.T_GRID[::2]
    want = TF.integrate_lagtransfer(H.Profile(), tfs, g, t, n_radii=120, t0=3.0)
    check_lag(TF.integrate_lagtransfer(H.Profile(), tfs, g, t, n_radii=120, t0=3.0, ensemble=ens), want, "lag, 20 x 48 bins (LDS accumulators)")


def test_long_branches_and_odd_sizes(TF, ens):
    """one branch of 300 knots, one of 1024 (the most a branch may have); 37 bins and 131 annuli in chunks of 7: neither a
    multiple of the wave, of the workgroup's four waves or of the chunk"""
    tfs = H.synthetic_branches(TF, knots_of={(4, "lower"): 300, (11, "upper"): 1024, (12, "upper"): 2})
    assert tfs.branches[4].lower_g.size == 300 and tfs.branches[11].upper_g.size == 1024 and tfs.branches[12].upper_g.size == 2
    g = np.linspace(0.15, 1.45, 38)
    prof = H.Profile()
    want_line = TF.integrate_lineprofile(H.emissivity, tfs, g, n_radii=131)
    want_lag = TF.integrate_lagtransfer(prof, tfs, g, H.T_GRID, n_radii=131, t0=3.0)
    try:
        for chunk in (7, 0):
            ens.ctx.set("tf_chunk", chunk)
            check_line(TF.integrate_lineprofile(H.emissivity, tfs, g, n_radii=131, ensemble=ens), want_line, f"line, tf_chunk {chunk}")
            check_lag(TF.integrate_lagtransfer(prof, tfs, g, H.T_GRID, n_radii=131, t0=3.0, ensemble=ens), want_lag, f"lag, tf_chunk {chunk}")
    finally:
        ens.ctx.set("tf_chunk", 0)
    # more bins than a wave has lanes, and a single bin
    for g in (np.linspace(0.1, 1.5, 151), np.array([0.4, 1.3])):
        check_line(TF.integrate_lineprofile(H.emissivity, tfs, g, n_radii=131, ensemble=ens),
                   TF.integrate_lineprofile(H.emissivity, tfs, g, n_radii=131), f"line, {g.size - 1} bins")


def test_real_transfer_functions(G, TF, ens):
    m = G.KerrMetric(M=1.0, a=0.998)
    x = np.array([0.0, 1000.0, math.radians(60), 0.0])
    d = G.ThinDisc(0.0, 1000.0)
    tfs = TF.transferfunctions(m, x, d, numrₑ=6, N=20, ensemble=ens)
    bins = np.linspace(0.1, 1.5, 101)
    ε = lambda r: r ** -3.0
    host = TF.integrate_lineprofile(ε, tfs, bins, h=2e-8, n_radii=300)
    check_line(TF.integrate_lineprofile(ε, tfs, bins, h=2e-8, n_radii=300, ensemble=ens), host, "Kerr a = 0.998, 60 deg, 6 radii")
    t_grid = np.linspace(0.0, 150.0, 76) + 1.0 / 3.0
    want = TF.integrate_lagtransfer(H.Profile(), tfs, bins, t_grid, n_radii=100, t0=x[1])
    check_lag(TF.integrate_lagtransfer(H.Profile(), tfs, bins, t_grid, n_radii=100, t0=x[1], ensemble=ens), want, "Kerr lag, 100 x 75 bins")
    _, default = G.lineprofile(bins, ε, m, x, d, numrₑ=6, N=20, n_radii=300, ensemble=ens)
    _, device = G.lineprofile(bins, ε, m, x, d, numrₑ=6, N=20, n_radii=300, ensemble=ens, integrate_on_device=True)
    check_line(device, default, "lineprofile(integrate_on_device=True) against the default")


def test_a_batch_is_its_sets_bit_for_bit(TF, ens):
    """two corners of a table and a point between them, each with its own emissivity and inner radius"""
    grids = np.empty((2, 1), dtype=object)
    for k, seed in enumerate((1, 2)):
        grids[k, 0] = TF.transfer_function_grid(H.synthetic_branches(TF, seed=seed), Ng=20)
    table = TF.CunninghamTransferTable((np.array([0.0, 0.998]), np.array([30.0])), grids)
    tfs = [table(0.0, 30.0), table(0.998, 30.0), table(0.37, 30.0)]
    εs = [lambda r: r ** -3.0, lambda r: r ** -2.0, lambda r: r ** -3.0 if r > 6.0 else 6.0 ** -3.0 * (r / 6.0) ** -1.5]
    rmins = [None, 2.5, 4.0]
    batch = TF.integrate_lineprofiles(εs, tfs, H.G_GRID, rmin=rmins, n_radii=150, ensemble=ens)
    assert batch.shape == (3, 61)
    for k in range(3):
        one = TF.integrate_lineprofile(εs[k], tfs[k], H.G_GRID, rmin=rmins[k], n_radii=150, ensemble=ens)
        assert one.tobytes() == batch[k].tobytes()
        check_line(one, TF.integrate_lineprofile(εs[k], tfs[k], H.G_GRID, rmin=rmins[k], n_radii=150), f"set {k} of the batch")
    assert len({batch[k].tobytes() for k in range(3)}) == 3


def test_same_bytes_on_every_run_and_launch_shape(TF, ens, synth):
    tfs = synth[0]
    prof = H.Profile()
    small_g, small_t = np.linspace(0.3, 1.3, 21), H.T_GRID[::2]

    def run():
        return [TF.integrate_lineprofile(H.emissivity, tfs, H.G_GRID, n_radii=200, ensemble=ens),
                TF.integrate_lagtransfer(prof, tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0, ensemble=ens),
                TF.integrate_lagtransfer(prof, tfs, small_g, small_t, n_radii=120, t0=3.0, ensemble=ens)]

    first, again = run(), run()
    shaped = []
    try:
        for chunk in (1, 7):
            ens.ctx.set("tf_chunk", chunk)
            shaped.append(run())
    finally:
        ens.ctx.set("tf_chunk", 0)
    for other in [again] + shaped:
        for a, b in zip(first, other):
            assert a.tobytes() == b.tobytes()
    with pytest.raises(Exception, match="tf_chunk must be in"):
        ens.ctx.set("tf_chunk", -1)


def test_nothing_is_kept_on_the_context(G, TF, ens, synth):
    """a render and a gr_lagtransfer_trace between two integrations change nothing, and the integrations leave the trace's rows"""
    tfs = synth[0]
    before = TF.integrate_lineprofile(H.emissivity, tfs, H.G_GRID, n_radii=200, ensemble=ens)
    m = G.KerrMetric(M=1.0, a=0.998)
    x = np.array([0.0, 1000.0, math.radians(60), 0.0])
    d = G.ThinDisc(m.isco(), 500.0)
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    G.rendergeodesics(m, x, d, 2000.0, image_width=16, image_height=16, alpha_lims=(-30, 30), beta_lims=(-20, 20), pf=pf, ensemble=ens)
    plane = G.PolarPlane(G.GeometricGrid(), Nr=16, Nθ=16, r_max=50.0)
    sampler = G.EvenSampler(domain=G.BothHemispheres(), generator=G.GoldenSpiralGenerator())
    tf = G.lagtransfer_device(m, x, d, G.LampPostModel(h=10.0, θ=math.radians(0.0001)), ensemble=ens, plane=plane, n_samples=200,
                              sampler=sampler)
    rows = G.reverberation.lag_rows(tf)
    after = TF.integrate_lineprofile(H.emissivity, tfs, H.G_GRID, n_radii=200, ensemble=ens)
    assert after.tobytes() == before.tobytes()
    lag = TF.integrate_lagtransfer(H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0, ensemble=ens)
    check_lag(lag, synth[2], "lag after a render and a trace", 5668)
    assert G.reverberation.lag_rows(tf).tobytes() == rows.tobytes()
    assert G.binflux(tf, N_E=8, N_t=8)[2].shape == (8, 8)
