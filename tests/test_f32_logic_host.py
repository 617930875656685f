"""The SINGLE-PRECISION text of the HIP integrator (gr_device.hpp under GR_REAL_IS_FLOAT: what the twelve kernels32_m*.o hold)
compiled for the host (tests/host_harness_f32.cpp) and compared with the oracle, for every catalogue metric.  Runs without a
GPU.  That text is not the fp64 text with another typedef: dilaton-axion and NoZ keep the dual-number right-hand side, Kerr
forms its inverse components first, the stage sums are packed pairs, every literal is a float.  Criteria and margins:
tests/f32_scene.py."""
import numpy as np
import pytest

import f32_scene as S
import harness_f32 as Hf


def _host_points(G, cls, params, tol):
    cfg = G.render_configuration(S.metric(G, cls, params), S.X_OBS, G.ThinDisc(*S.DISC), S.LAMBDA_MAX, **S.render_kwargs(tol))
    return Hf.render_endpoints(G, cfg)


@pytest.mark.parametrize("name,params,cls", S.CASES, ids=S.CASE_IDS)
def test_f32_text_is_as_good_as_the_oracle_at_its_tolerance(G, oracle, name, params, cls):
    """End points of the 48 x 48 thin-disc scene at tolerance 1e-5: against the oracle at 1e-9 the single-precision text is
    at most a stated factor worse than the oracle at 1e-5 is (measured on this build: mismatches <= 1.19 x, median <= 1.08 x,
    p90 <= 1.05 x the baseline; at most 1.3 % of the rays flagged, all for dt < dtmin)."""
    S.check_against_baseline(oracle, name, params, _host_points(G, cls, params, S.TOL), "host f32")


@pytest.mark.parametrize("tol", [1e-4, 1e-3])
@pytest.mark.parametrize("name,params,cls", S.NAN_CASES, ids=S.NAN_CASE_IDS)
def test_f32_rejects_an_overflowed_trial_step(G, oracle, name, params, cls, tol):
    """At loose tolerances the controller proposes h ≈ r to an ingoing ray at r ≈ 25: the trial step's stage points lie inside the
    hole, the single-precision right-hand side overflows there and the error norm is NaN.  That is a step to reject, as the
    fp64 kernels and the oracle do (they see EEst² ~ 1e22): before Ray::step did so under GR_REAL_IS_FLOAT, 13 / 3 NoZ, 7 / 1
    dilaton-axion and 2 / 0 Kerr rays of this scene ended at r = 20 .. 27, λ = 175 .. 200 with GR_FLAG_NAN and status NoStatus at
    1e-3 / 1e-4 (central pixels, e.g. rays 1110, 1125 and 1173 of the NoZ plane at 1e-4)."""
    S.check_no_midflight_nan(oracle, name, params, _host_points(G, cls, params, tol), tol, "host f32")


def test_f32_step_log_follows_a_rejected_overflow(G):
    """The per-ray step log of the harness on the ray that showed the defect (NoZ, 1e-4, ray 1125): the step proposed at
    r = 26.3 with h = 27.9 has a NaN error norm, is rejected with the largest shrink factor (h / 5) and the ray goes on to an
    end that carries no flag."""
    name, params, cls = S.CASES[10]
    cfg = G.render_configuration(S.metric(G, cls, params), S.X_OBS, G.ThinDisc(*S.DISC), S.LAMBDA_MAX, **S.render_kwargs(1e-4))
    pt, log = Hf.step_log(G, cfg, 1125)
    col = {c: i for i, c in enumerate(Hf.LOG_COLS)}
    nan_rows = np.nonzero(np.isnan(log[:, col["e2"]]))[0]
    assert nan_rows.size >= 1
    k = int(nan_rows[0])
    assert k + 1 < log.shape[0]                                             # the ray went on
    assert log[k, col["flags"]] == 0 and log[k, col["r"]] > 20.0
    assert log[k, col["t"]] == log[k - 1, col["t"]]                         # rejected: no progress in λ
    assert log[k, col["dt"]] == pytest.approx(log[k, col["h"]] / 5.0, rel=1e-6)
    assert np.isfinite(log[k + 1, col["e2"]])
    assert (pt["flags"] & S.FLAG_MASK) == 0
    assert np.all(np.diff(log[:, col["t"]]) >= 0.0)


def test_f32_johannsen_redshift_image_reads_the_plunging_table(G, oracle):
    """The fused point-function entry of the harness (out_mode 0): the Johannsen redshift image of
    test_gpu_f32_metrics.py::test_f32_johannsen_redshift_reads_the_plunging_table, 64 x 64 at 1e-5, the disc reaching inside the
    ISCO, with the oracle's plunging table handed to the float text and to the oracle alike.  Bounds as there: against the
    oracle@1e-9 image the NaN pattern differs in at most 1.5 x as many pixels as the oracle@1e-5 image's does, the median
    relative redshift error over the common hits is at most 1.5 x that image's (measured: 50 / 62 pixels, 5.28e-6 / 5.18e-6)."""
    import math

    from gradus_jl_amd.pointfunctions import GR_PF_REDSHIFT, PointFunction

    joh = (1.0, 0.7, 2.0, 0.0, 0.0, 1.0)
    alims, blims = (-60.0, 60.0), (-35.0, 35.0)
    m = G.JohannsenMetric(*joh)
    isco = m.isco()
    x = np.array([0.0, 1000.0, math.radians(70), 0.0])
    ocfg = {tol: oracle.make_config("johannsen", joh, disc=(2.0, 50.0), lambda_max=2000.0, abstol=tol, reltol=tol) for tol in (1e-9, 1e-5)}
    table = tuple(oracle.plunging_table(ocfg[1e-9], isco))
    pf = PointFunction(lambda *a, **k: None, device_pf=GR_PF_REDSHIFT, extra={"r_isco": isco, "plunge": table})
    pf = pf @ G.ConstPointFunctions.filter_intersected()
    cfg = G.render_configuration(m, x, G.ThinDisc(2.0, 50.0), 2000.0, image_width=64, image_height=64, alpha_lims=alims,
                                 beta_lims=blims, abstol=1e-5, reltol=1e-5)
    img = Hf.render(G, cfg, pf)
    ref, pts = oracle.rendergeodesics(ocfg[1e-9], x, alims, blims, 64, 64, pf_id=oracle.PF_REDSHIFT, filter_id=oracle.FILTER_INTERSECTED,
                                      r_isco=isco, plunge=table, return_points=True)
    base = oracle.rendergeodesics(ocfg[1e-5], x, alims, blims, 64, 64, pf_id=oracle.PF_REDSHIFT, filter_id=oracle.FILTER_INTERSECTED,
                                  r_isco=isco, plunge=table)
    rho = pts["x"][:, 1] * np.abs(np.sin(pts["x"][:, 2]))
    assert ((pts["status"] == 2) & (rho < isco)).sum() >= 8        # the interpolated branch is exercised

    def against_ref(a):
        both = ~np.isnan(a) & ~np.isnan(ref)
        return int((np.isnan(a) != np.isnan(ref)).sum()), float(np.median(np.abs(a[both] / ref[both] - 1.0))), int(both.sum())

    (d, e, n), (d0, e0, n0) = against_ref(img), against_ref(base)
    print(f"host f32 johannsen redshift: NaN pattern differs in {d} / {d0} pixels, median relative error {e:.3e} / {e0:.3e}, "
          f"common hits {n} / {n0}  (f32 / oracle@1e-5, both against oracle@1e-9)")
    assert n > 200
    assert d <= 1.5 * d0
    assert e <= 1.5 * e0
