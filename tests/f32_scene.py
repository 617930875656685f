"""The scene, the cases and the criteria that pin the single-precision kernels of all eleven catalogue metrics against the oracle
(tests/test_f32_logic_host.py on the CPU build of that text, tests/test_gpu_f32_metrics.py on the device).

A single-precision trace at tolerance 1e-5 cannot agree with the oracle at 1e-9 to rounding.  What it can be held to is the
oracle's OWN error at that tolerance: `baseline` = oracle@tol against oracle@1e-9, `f32` = the kernel text @tol against the same
oracle@1e-9, and f32 may be worse than the baseline by a stated factor only.  The margins:
  * status mismatches: rim pixels flip between hit and miss between any two step sequences; the count is counting noise around
    ~150 (sigma ~12) on this scene and the worst ratio measured on the CPU build is 1.19 -- 1.5 x is about six sigma;
  * median and 90th percentile of the end-point error: a wrong term, a truncated constant or a bad reciprocal seed in a
    right-hand side moves them by orders of magnitude, not by 50 % (bounds 1.5 x and 2 x);
  * >= 800 common hits keeps the statistics from being vacuous;
  * <= 4 % of the rays flagged: a condition, not a measurement (the project's record at this tolerance is 3.5 % of C5's rays
    dropped for dt < dtmin; the CPU build stays at or below 1.5 % here, the oracle flags 3 Bumblebee rays and none elsewhere);
  * no GR_FLAG_NAN at 1e-5.
"""
import math

import numpy as np

# (oracle name, parameters, class of the package): metric ids 0..10 of include/gradus_mi355x.h, in that order
CASES = [
    ("kerr", (1.0, 0.9), "KerrMetric"),
    ("johannsen", (1.0, 0.7, 1.0, 0.5, -0.5, 1.0), "JohannsenMetric"),
    ("morris-thorne", (1.5,), "MorrisThorneWormhole"),
    ("bumblebee", (1.0, 0.2, 0.3), "BumblebeeMetric"),
    ("kerr-newman", (1.0, 0.6, 0.5), "KerrNewmanMetric"),
    ("johannsen-psaltis", (1.0, 0.6, 1.0), "JohannsenPsaltisMetric"),
    ("dilaton-axion", (1.0, 0.5, 0.2, 0.8), "DilatonAxion"),
    ("spherical", (), "SphericalMetric"),
    ("kerr-dark-matter", (1.0, 0.6, 2.0, 20.0, 10.0), "KerrDarkMatter"),
    ("kerr-refractive", (1.0, 0.6, 1.2, 20.0), "KerrRefractive"),
    ("noz", (1.0, 0.7, 0.5), "NoZMetric"),
]
CASE_IDS = [c[0] for c in CASES]
# the metrics whose single-precision rays ended NaN-flagged in mid-flight at loose tolerances before the rejected-step fix
NAN_CASES = [c for c in CASES if c[0] in ("kerr", "noz", "dilaton-axion")]
NAN_CASE_IDS = [c[0] for c in NAN_CASES]

# the scene of test_remaining_metrics_on_device_vs_oracle
X_OBS = np.array([0.0, 200.0, math.radians(70), 0.0])
W = H = 48
DISC = (3.0, 60.0)
LAMBDA_MAX = 500.0
ALIMS, BLIMS = (-40, 40), (-30, 30)
TOL = 1e-5
FLAG_MASK, FLAG_NAN = 0xFFFF, 4       # GR_FLAG_MASK, GR_FLAG_NAN == ORC_FLAG_NAN

_oracle_cache = {}


def metric(G, cls, params):
    return getattr(G, cls)(*params)


def render_kwargs(tol):
    return dict(image_width=W, image_height=H, alpha_lims=ALIMS, beta_lims=BLIMS, abstol=tol, reltol=tol)


def oracle_points(oracle, name, params, tol):
    """(end points of the scene's W x H rays by the oracle at `tol`, its configuration): computed once per session."""
    key = (name, tol)
    if key not in _oracle_cache:
        ocfg = oracle.make_config(name, params, disc=DISC, lambda_max=LAMBDA_MAX, abstol=tol, reltol=tol)
        pts = oracle.trace(ocfg, X_OBS, oracle.render_velocities(ocfg, X_OBS, ALIMS, BLIMS, W, H))
        pts.setflags(write=False)
        _oracle_cache[key] = (pts, ocfg)
    return _oracle_cache[key]


def stats(pts, ref):
    """pts against ref (the oracle at 1e-9): status mismatches over the rays pts does not flag; median and 90th percentile of
    the per-hit error max over (r, θ) of |x - x_ref| / max(|x_ref|, 1) over the common hits; the number of common hits; the
    rays flagged; the rays NaN-flagged."""
    flagged = (pts["flags"] & FLAG_MASK) != 0
    mism = int(((pts["status"] != ref["status"]) & ~flagged).sum())
    hit = ~flagged & (pts["status"] == 2) & (ref["status"] == 2)
    a, b = pts["x"][hit][:, 1:3], ref["x"][hit][:, 1:3]
    err = np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0), axis=1)
    return dict(mism=mism, median=float(np.median(err)), p90=float(np.percentile(err, 90)), hits=int(hit.sum()),
                flagged=int(flagged.sum()), nan=int(((pts["flags"] & FLAG_NAN) != 0).sum()))


def check_against_baseline(oracle, name, params, got, label):
    """The criteria of the module docstring for `got`, the scene's end points at TOL by the code under test."""
    ref, _ = oracle_points(oracle, name, params, 1e-9)
    base, _ = oracle_points(oracle, name, params, TOL)
    s, b = stats(got, ref), stats(base, ref)
    print(f"{label} {name}: mismatches {s['mism']} / {b['mism']}  median {s['median']:.3e} / {b['median']:.3e}  "
          f"p90 {s['p90']:.3e} / {b['p90']:.3e}  hits {s['hits']} / {b['hits']}  flagged {s['flagged']} / {b['flagged']}  "
          f"nan {s['nan']}  (f32 / oracle@{TOL:g}, both against oracle@1e-9)")
    assert s["hits"] >= 800
    assert s["mism"] <= 1.5 * b["mism"]
    assert s["median"] <= 1.5 * b["median"]
    assert s["p90"] <= 2.0 * b["p90"]
    assert s["flagged"] <= 0.04 * got.size
    assert s["nan"] == 0
    return s, b


def check_no_midflight_nan(oracle, name, params, got, tol, label):
    """No ray of `got` (the scene at `tol` by the code under test) is NaN-flagged where its last radius is above twice the chart's
    inner radius and the oracle at the same tolerance flags nothing for it: out there nothing is singular, and a ray that ends
    with GR_FLAG_NAN becomes a silent NaN pixel."""
    base, ocfg = oracle_points(oracle, name, params, tol)
    nan = (got["flags"] & FLAG_NAN) != 0
    bad = nan & (got["x"][:, 1] > 2.0 * ocfg.r_inner) & ((base["flags"] & FLAG_MASK) == 0)
    print(f"{label} {name} @ {tol:g}: NaN-flagged {int(nan.sum())}, of them in mid-flight {int(bad.sum())}"
          + "".join(f"\n    ray {i}: r = {got['x'][i, 1]:.3f}, lambda = {got['lambda_max'][i]:.2f}, oracle status {base['status'][i]}"
                    for i in np.nonzero(bad)[0][:8]))
    assert not bad.any()
