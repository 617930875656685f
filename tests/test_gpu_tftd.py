"""The lag transfer function of a time-dependent emissivity on the device (integrate_lagtransfer of a RingCoronaProfile / a
DiscCoronaProfile with `ensemble=`: gr_tf_lagtransfer_td, kernels k_tftd_em and k_tftd) against the host route on the same
inputs: harness_tftd's synthetic profiles (arms of 2, 70 and 1024 slices, slices that miss, a tie in t, nonzero delays), 37
annuli, n_time 2 / 33 / 100, g_upscale 1 / 3, accumulators in LDS (20 x 48 bins) and in global memory (70 x 40), a t grid that
drops deposits.  The bound is 1e-12 of the peak (harness_tfint.TOL; the host build of the same arithmetic differs from the host
route by 9e-16, tests/test_tftd_host.py); a cell may differ beyond it only as a deposit moved across a t edge
(harness_tfint.lag_error).  The ε(time) table: limits bit for bit, values to 1e-14 relative.

Every parity test prints what it measures before it asserts."""
import numpy as np
import pytest

import harness_tfint as H
import harness_tftd as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def TF(G):
    return G.transfer_functions


def profile(G, kind):
    return T.disc_profile(G) if kind == "disc" else T.ring_profile(G)


def device(G, ens, kind, case, em=None):
    TF = G.transfer_functions
    grid, n_time, upscale = case
    g, t = T.GRIDS[grid]
    if em is None:
        return TF.integrate_lagtransfer(profile(G, kind), T.branches(TF), g, t, n_radii=T.N_RADII, t0=T.T0, g_grid_upscale=upscale,
                                        n_time_steps=n_time, ensemble=ens)
    return TF._integrate_lagtransfer_td_device(profile(G, kind), T.branches(TF), g, t, rmin=None, rmax=None, g_scale=1.0, h=1e-8,
                                               n_radii=T.N_RADII, quadrature_points=7, t0=T.T0, g_grid_upscale=upscale, n_time_steps=n_time,
                                               call=TF._tftd_library_call(ens), em_out=em)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: f"{c[0]}-nt{c[1]}-up{c[2]}")
@pytest.mark.parametrize("kind", ["disc", "ring"])
def test_device_against_the_host_route(G, ens, kind, case):
    host, n_host = T.host_case(G, kind, *case)
    em = []
    try:
        got = {}
        for chunk in (7, 0):
            ens.ctx.set("tf_chunk", chunk)
            got[chunk] = device(G, ens, kind, case, em)
    finally:
        ens.ctx.set("tf_chunk", 0)
    same, rel = T.em_error(em[0], T.host_table(G, kind, case[1])[1])
    err, moved = H.lag_error(got[7], host, n_host)
    print(f"{kind} {case}: device - host {err:.3e} of the peak, {moved} of {n_host} deposits moved across a t edge; em limits equal: {same}, "
          f"em values: {rel:.3e} relative")
    assert same and rel <= 1e-14
    assert err <= T.TOL
    assert got[7].tobytes() == got[0].tobytes() and em[0].tobytes() == em[1].tobytes()      # tf_chunk is the launch shape only
    assert np.all(got[0][-1] == 0.0) and got[0][:-1].sum() == pytest.approx(1.0, rel=1e-12)


def test_same_bytes_on_every_run(G, ens):
    for kind, case in (("disc", T.CASES[1]), ("ring", T.CASES[2])):
        first, again = device(G, ens, kind, case), device(G, ens, kind, case)
        assert first.tobytes() == again.tobytes()
        assert first.tobytes() == device(G, ens, kind, case, []).tobytes()      # with and without em_out


def test_nothing_is_kept_on_the_context(G, TF, ens):
    """an ordinary integrate_lagtransfer before and after gives the same bytes, and so does the time-dependent one around it"""
    tfs = T.branches(TF)
    before = TF.integrate_lagtransfer(H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0, ensemble=ens)
    td = device(G, ens, "disc", T.CASES[2])
    after = TF.integrate_lagtransfer(H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0, ensemble=ens)
    assert after.tobytes() == before.tobytes()
    assert device(G, ens, "disc", T.CASES[2]).tobytes() == td.tobytes()
    with pytest.raises(NotImplementedError, match="time-dependent"):
        TF.integrate_lagtransfer(H.Profile(), tfs, H.G_GRID, H.T_GRID, n_radii=120, t0=3.0, ensemble=ens, n_time_steps=33)
