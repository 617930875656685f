"""The single-precision kernel objects (kernels32_m0 .. m10) of every catalogue metric on the device, against the oracle:
the criteria of tests/f32_scene.py that tests/test_f32_logic_host.py applies to the CPU build of the same text.  The device
build differs from that one in its reciprocal / rsqrt seeds, the hardware log2 / exp2 of the controller and the compiler's
contraction, so it is held to the same bounds on its own."""
import math

import numpy as np
import pytest

import f32_scene as S

pytestmark = pytest.mark.gpu


def _device_points(G, ens, cls, params, tol, kernel):
    ens.set("kernel", kernel).set("precision", 32)
    try:
        _, _, cache = G.prerendergeodesics(S.metric(G, cls, params), S.X_OBS, G.ThinDisc(*S.DISC), S.LAMBDA_MAX, ensemble=ens,
                                           **S.render_kwargs(tol))
        return np.ascontiguousarray(cache.points.T).ravel()
    finally:
        ens.set("precision", 64).set("kernel", 2)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("name,params,cls", S.CASES, ids=S.CASE_IDS)
def test_f32_kernels_are_as_good_as_the_oracle_at_its_tolerance(G, oracle, ens, kernel, name, params, cls):
    """End points of the 48 x 48 thin-disc scene at tolerance 1e-5 through the lane kernel (0) and the persistent kernel (1) of
    each metric's fp32 object."""
    S.check_against_baseline(oracle, name, params, _device_points(G, ens, cls, params, S.TOL, kernel), f"device f32 kernel {kernel}")


@pytest.mark.parametrize("name,params,cls", S.NAN_CASES, ids=S.NAN_CASE_IDS)
def test_f32_kernels_reject_an_overflowed_trial_step(G, oracle, ens, name, params, cls):
    """tests/test_f32_logic_host.py::test_f32_rejects_an_overflowed_trial_step on the device at 1e-4."""
    S.check_no_midflight_nan(oracle, name, params, _device_points(G, ens, cls, params, 1e-4, 1), 1e-4, "device f32")


JOH = (1.0, 0.7, 2.0, 0.0, 0.0, 1.0)          # the metric and scene of test_gpu_parity.py::test_johannsen_redshift_matches_oracle
J_ALIMS, J_BLIMS = (-60.0, 60.0), (-35.0, 35.0)
_johannsen_cache = {}


def _johannsen_references(G, oracle, ens):
    """The plunging table (traced once, by the fp64 kernels) and the oracle's redshift images at 1e-9 and 1e-5 with that table."""
    if not _johannsen_cache:
        m = G.JohannsenMetric(*JOH)
        x = np.array([0.0, 1000.0, math.radians(70), 0.0])
        pf = G.ConstPointFunctions.redshift(m, x, ensemble=ens) @ G.ConstPointFunctions.filter_intersected()
        imgs = {}
        for tol in (1e-9, 1e-5):
            ocfg = oracle.make_config("johannsen", JOH, disc=(2.0, 50.0), lambda_max=2000.0, abstol=tol, reltol=tol)
            imgs[tol], pts = oracle.rendergeodesics(ocfg, x, J_ALIMS, J_BLIMS, 64, 64, pf_id=oracle.PF_REDSHIFT,
                                                    filter_id=oracle.FILTER_INTERSECTED, r_isco=m.isco(),
                                                    plunge=pf.extra["plunge"], return_points=True)
            if tol == 1e-9:
                rho = pts["x"][:, 1] * np.abs(np.sin(pts["x"][:, 2]))
                _johannsen_cache["plunging_hits"] = int(((pts["status"] == 2) & (rho < m.isco())).sum())
        _johannsen_cache.update(m=m, x=x, pf=pf, ref=imgs[1e-9], base=imgs[1e-5])
    return _johannsen_cache


@pytest.mark.parametrize("lds", [1, 0])
def test_f32_johannsen_redshift_reads_the_plunging_table(G, oracle, ens, lds):
    """One fused redshift image by the Johannsen fp32 kernel, 64 x 64 at 1e-5, the disc reaching inside the ISCO so that the
    plunging table is read -- out of LDS (lds = 1) and out of global memory (lds = 0).  Against the oracle@1e-9 image with the
    same table: the NaN pattern differs in at most 1.5 x as many pixels as the oracle@1e-5 image's does, the median relative
    redshift error over the common hits is at most 1.5 x that image's."""
    c = _johannsen_references(G, oracle, ens)
    ens.set("kernel", 1).set("lds", lds).set("precision", 32)
    try:
        _, _, img = G.rendergeodesics(c["m"], c["x"], G.ThinDisc(2.0, 50.0), 2000.0, image_width=64, image_height=64,
                                      alpha_lims=J_ALIMS, beta_lims=J_BLIMS, pf=c["pf"], ensemble=ens, abstol=1e-5, reltol=1e-5)
    finally:
        ens.set("precision", 64).set("lds", 1).set("kernel", 2)
    ref, base = c["ref"], c["base"]

    def against_ref(a):
        both = ~np.isnan(a) & ~np.isnan(ref)
        return int((np.isnan(a) != np.isnan(ref)).sum()), float(np.median(np.abs(a[both] / ref[both] - 1.0))), int(both.sum())

    (d, e, n), (d0, e0, n0) = against_ref(img), against_ref(base)
    print(f"device f32 johannsen redshift lds={lds}: NaN pattern differs in {d} / {d0} pixels, median relative error {e:.3e} / {e0:.3e}, "
          f"common hits {n} / {n0}, hits inside the ISCO {c['plunging_hits']}  (f32 / oracle@1e-5, both against oracle@1e-9)")
    assert c["plunging_hits"] >= 8        # the interpolated branch is exercised (> 20 at 96 x 96 in test_gpu_parity.py: x 4/9)
    assert n > 200
    assert d <= 1.5 * d0
    assert e <= 1.5 * e0
