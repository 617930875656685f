"""The scenes of the adaptive image plane's tests (tests/test_planegrid_host.py, tests/test_gpu_adaptive_plane.py): a Kerr hole with
a = 0.998 seen from (0, 1000, 75°, 0), ThinDisc(isco, 50), λ_max 2000, tolerances 1e-9, x_periodic = False.  Scene A is the window
(-12, 12)², scene B (-60, 60) x (-35, 35).  A CPU-oracle prototype found for both: trace_initial(level = 3) gives 819 cells, four
trace_steps refine 89, 229, 497, 1101 cells (A) and 125, 378, 1098, 3269 cells (B; 4753 leaves after two steps), and no both-hit
pair of these steps lies within 1e-9 (relative) of the criterion's threshold."""
import math

import numpy as np

SPIN = 0.998
X_OBS = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
LIMITS = {"A": (-12.0, 12.0, -12.0, 12.0), "B": (-60.0, 60.0, -35.0, 35.0)}
REFINED = {"A": [89, 229, 497, 1101], "B": [125, 378, 1098, 3269]}
T_MAX, TOL, R_OUT = 2000.0, 1e-9, 50.0


def metric(G):
    return G.KerrMetric(1.0, SPIN)


def oracle_config(G, O, r_in=None, r_out=R_OUT):
    """the oracle's configuration of the scene: the chart of AdaptivePlane, chart_for_metric(m, 2 * 2 x[1])"""
    m = metric(G)
    return O.make_config("kerr", (1.0, SPIN), disc=(m.isco() if r_in is None else r_in, r_out), lambda_max=T_MAX, abstol=TOL, reltol=TOL,
                         outer_radius=2 * 2 * X_OBS[1])


def oracle_plane(G, O, scene, steps=0, x_periodic=False, level=3):
    """the scene traced on the oracle through the generic form of AdaptiveSky: trace_initial and `steps` trace_steps"""
    cfg = oracle_config(G, O)
    null = G.adaptive.make_null(1, G.POINT_DTYPE)

    def calc_values(α, β):
        return O.trace(cfg, X_OBS, O.map_impact_parameters(cfg, X_OBS, -np.asarray(α), β)).astype(G.POINT_DTYPE, copy=False)

    sky = G.AdaptiveSky(calc_values, G.check_refine_plane, limits=LIMITS[scene], x_periodic=x_periodic, null=null)
    G.trace_initial(sky, level=level)
    for _ in range(steps):
        G.trace_step(sky)
    return sky


def device_plane(G, ens, scene, resident, steps=None, **kw):
    """AdaptivePlane of the scene on the ensemble; steps = None: not traced yet"""
    m = metric(G)
    x1, x2, y1, y2 = LIMITS[scene]
    sky = G.AdaptivePlane(m, X_OBS, G.ThinDisc(m.isco(), R_OUT), α_lims=(x1, x2), β_lims=(y1, y2), ensemble=ens, t_max=T_MAX, abstol=TOL,
                          reltol=TOL, resident=resident, **kw)
    if steps is not None:
        G.trace_initial(sky)
        for _ in range(steps):
            G.trace_step(sky)
    return sky


def threshold_margin(sky, i1, i2, percentage=20):
    """per both-hit pair the smallest relative distance of |a - b| from rtol max(|a|, |b|) over the criterion's two terms"""
    v1, v2 = sky.values[i1], sky.values[i2]
    both = (v1["status"] == 2) & (v2["status"] == 2)
    margins = []
    for a, b in ((np.log10(v1["x"][both, 1]), np.log10(v2["x"][both, 1])),
                 (np.mod(v1["x"][both, 2], 2 * math.pi), np.mod(v2["x"][both, 2], 2 * math.pi))):
        bound = percentage / 100 * np.maximum(np.abs(a), np.abs(b))
        with np.errstate(invalid="ignore", divide="ignore"):
            margins.append(np.where(bound > 0, np.abs(np.abs(a - b) - bound) / bound, np.inf))
    return np.minimum(*margins)
