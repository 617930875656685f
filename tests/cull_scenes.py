"""The scenes that pin the miss culls of the fused fp64 Kerr kernels (Ray::start_decided, Ray::step) to the uncut
trace over the whole domain their gate lets them act in (tests/test_cull_domain_host.py on the host build of the integrator,
tests/test_gpu_cull_domain.py on the device): one table for both, so that the device is asked what the host was.

Every length is given in units of M and scaled by it: the observer's radius, the disc's edges, the window, max_time and the
chart's outer radius.  A scene is the bench scene (a = 0.998 M, observer (1000 M, 75°), ThinDisc(isco, 50 M), window
(-60, 60) x (-35, 35) M, max_time 2000 M, chart 12000 M, the default tolerance and gtol) with the differences NAMED lists.

FIRES says which of the four mechanisms must end at least one ray of a named scene: "start" (decided before the first step),
"defer" (ended at the first accepted step), "entry" (ended on entering R_cull), "step" (the step loop's escape and polar-rate
culls: a ray none of the other three ended that takes fewer steps than in the uncut trace).  It was filled from `python
tests/cull_scenes.py`, the host build at 64 x 64 over all 64 tiles, the size tests/test_cull_domain_host.py runs -- not from the
device and not from a larger image.  Where the set is empty the culls must leave every step count alone.

The older host tests of the single culls (tests/test_cull_host.py and the pass, entry and defer cull's) and scripts/cull_census.py
trace the bench scene itself under the default chart, at 2048² (bench_scene) or at 64² with one parameter changed (bench_variant, SCENES).
"""
import math

import numpy as np

# name -> what differs from the bench scene.  M; a, r_obs, r_in, r_out, window, max_time, outer in units of M; r_in None = the ISCO
BENCH = dict(M=1.0, a=0.998, r_obs=1000.0, theta=75.0, r_in=None, r_out=50.0, alims=(-60.0, 60.0), blims=(-35.0, 35.0),
             max_time=2000.0, outer=12000.0, tol=None, gtol=None)
NAMED = {
    "bench": dict(),
    "M2.5": dict(M=2.5),
    "M0.4_a-0.5": dict(M=0.4, a=-0.5),
    "a1": dict(a=1.0),
    "a0.5_th5": dict(a=0.5, theta=5.0),
    "th89.9": dict(theta=89.9),
    "th90": dict(theta=90.0),
    "a-0.7_th150": dict(a=-0.7, theta=150.0),
    "obs60": dict(r_obs=60.0),
    "obs51": dict(r_obs=51.0),
    "obs50": dict(r_obs=50.0),
    "obs200": dict(r_obs=200.0, max_time=600.0),
    "ring20": dict(r_in=20.0),
    "rin0": dict(r_in=0.0),
    "rout3": dict(r_in=0.0, r_out=3.0),
    "rout4": dict(r_in=0.0, r_out=4.0),
    "rout12": dict(r_out=12.0),
    "zoom8": dict(alims=(-8.0, 8.0), blims=(-8.0, 8.0)),
    "offdisc": dict(alims=(100.0, 160.0), blims=(40.0, 80.0)),
    "offcentre": dict(alims=(-10.0, 70.0), blims=(-5.0, 30.0)),
    "tol1e-6": dict(tol=1e-6),
    "tol1e-12": dict(tol=1e-12),
    "t1050": dict(max_time=1050.0),
    "t11500": dict(max_time=11500.0),
    "t20000": dict(max_time=20000.0),
    "outer1100": dict(outer=1100.0),
    "outer1010": dict(outer=1010.0),
    "gtol0.5": dict(gtol=0.5),
    "gtol0.9": dict(gtol=0.9),
    "obs1e5": dict(r_obs=1e5, max_time=2e5, outer=2e5),
}
MECHANISMS = ("start", "defer", "entry", "step")
# the host build at 64 x 64, every tile (`python tests/cull_scenes.py`); see the module docstring
FIRES = {
    "bench": {"start", "defer", "entry", "step"},
    "M2.5": {"start", "defer", "entry", "step"},
    "M0.4_a-0.5": {"start", "defer", "entry", "step"},
    "a1": {"start", "defer", "entry", "step"},
    "a0.5_th5": {"start", "entry"},
    "th89.9": {"start", "entry", "step"},
    "th90": {"start", "entry", "step"},
    "a-0.7_th150": {"start", "entry", "step"},
    "obs60": {"start", "defer", "entry", "step"},
    "obs51": {"start", "defer", "step"},
    "obs50": {"step"},
    "obs200": {"start", "defer", "entry", "step"},
    "ring20": {"start", "defer", "entry", "step"},
    "rin0": {"start", "defer", "entry", "step"},
    "rout3": {"start", "step"},
    "rout4": {"start", "step"},
    "rout12": {"start", "entry", "step"},
    "zoom8": set(),
    "offdisc": {"start"},
    "offcentre": {"start", "defer", "entry", "step"},
    "tol1e-6": {"start", "defer", "entry", "step"},
    "tol1e-12": {"start", "defer", "entry", "step"},
    "t1050": {"start", "defer", "entry", "step"},
    "t11500": {"entry", "step"},
    "t20000": set(),
    "outer1100": {"entry", "step"},
    "outer1010": {"step"},
    "gtol0.5": {"start", "entry", "step"},
    "gtol0.9": {"step"},
    "obs1e5": {"entry", "step"},
}
# the scenes in which the start's "λ1 comes first" bound fails for every ray while the entry cull's, formed later along the path
# with less affine time left, holds for some: both outcomes of that condition in one launch
LAMBDA1_BOUNDARY = ("t11500", "outer1100")
# random_scenes(SEED, N_RANDOM): on the host build (16 tiles of the seed's choice per scene) at most a quarter of the 40 end no
# ray early; `python tests/cull_scenes.py --random` prints the count
SEED = 20261019
N_RANDOM = 40
# ... and these are the scenes in which nothing fires at all on those tiles, the step loop's culls included; in every other one
# the culls take steps away
RANDOM_QUIET = (5, 9, 25)
ESCAPE_RADIUS_M = 4.0          # KerrMetric::kEscapeRadiusM
# the bench plane: its edge in pixels, its window and its observer
SIZE, ALIMS, BLIMS = 2048, (-60.0, 60.0), (-35.0, 35.0)
X_OBS = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
# the bench scene at 64² and its variants chosen for where the signs and closed forms of the pass cull can go wrong: a wider wedge,
# a = 0 (Ω_lo = Ω_hi, the a -> 0 form of μ+), a retrograde hole, an observer nearer the axis, one below the plane (μ0 < 0)
SCENES = {
    "bench64": dict(),
    "gtol0.1": dict(gtol=0.1),
    "a0": dict(a=0.0),
    "a-0.998": dict(a=-0.998),
    "theta30": dict(theta=30.0),
    "theta105": dict(theta=105.0),
}


def bench_scene(G, size=SIZE, x=X_OBS, r_out=50.0, a=0.998, **kw):
    """(configuration, point function) of the bench scene at `size`², with another observer, outer edge, spin or render keyword."""
    m = G.KerrMetric(1.0, a)
    cfg = G.render_configuration(m, x, G.ThinDisc(m.isco(), r_out), 2000.0, image_width=size, image_height=size,
                                 alpha_lims=ALIMS, beta_lims=BLIMS, **kw)
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    return cfg, pf


def bench_variant(G, a=0.998, theta=75.0, size=64, r_obs=1000.0, r_out=50.0, **kw):
    """(configuration, point function, a) of bench_scene at 64² with the observer given by radius and inclination (degrees):
    `bench_variant(G, **SCENES[name])`."""
    return (*bench_scene(G, size, np.array([0.0, r_obs, math.radians(theta), 0.0]), r_out, a, **kw), a)


def gate_radius_closed_form(M, r_out, gtol):
    """cull_gate_radius of gr_device.hpp for a scene inside the gate: what the drawing of random scenes places the observer by."""
    return (1.0 + 1e-6) * max(ESCAPE_RADIUS_M * M, r_out / math.sqrt(1.0 - gtol * gtol))


def _build(G, p, size):
    """(metric, observer, disc, max_time, render keywords) of the parameter set `p` (BENCH's keys, lengths in units of M)."""
    M = float(p["M"])
    w, h = (size, size) if np.isscalar(size) else size
    m = G.KerrMetric(M, p["a"] * M)
    x = np.array([0.0, p["r_obs"] * M, math.radians(p["theta"]), 0.0])
    r_in = m.isco() if p["r_in"] is None else p["r_in"] * M
    d = G.ThinDisc(r_in, p["r_out"] * M)
    kw = dict(image_width=int(w), image_height=int(h), alpha_lims=tuple(v * M for v in p["alims"]),
              beta_lims=tuple(v * M for v in p["blims"]), chart=G.chart_for_metric(m, p["outer"] * M))
    if p["tol"] is not None:
        kw["abstol"] = kw["reltol"] = p["tol"]
    if p["gtol"] is not None:
        kw["gtol"] = p["gtol"]
    return m, x, d, p["max_time"] * M, kw


def parameters(name):
    return {**BENCH, **NAMED[name]}


def scene(G, name, size):
    """(metric, observer, disc, max_time, render keywords) of the named scene at `size` (an edge, or (width, height))."""
    return _build(G, parameters(name), size)


def random_parameters(seed, n):
    """`n` parameter sets drawn inside the gate's domain (lengths in units of M; the ranges are listed in DESIGN_measurements.md §M28)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        M = float(rng.uniform(0.3, 3.0))
        a = float(rng.uniform(-1.0, 1.0))
        theta = float(rng.uniform(3.0, 177.0))
        r_out = float(rng.uniform(2.0, 80.0))
        gtol = float(math.exp(rng.uniform(math.log(1e-3), math.log(0.6))))
        r_in = (0.0, None, 0.4 * r_out)[int(rng.integers(3))]
        r_cull = gate_radius_closed_form(1.0, r_out, gtol)
        r_obs = float(r_cull * rng.uniform(1.001, 1.5)) if rng.integers(2) else float(rng.uniform(200.0, 2000.0))
        max_time = float(rng.uniform(1.05, 12.0)) * r_obs
        hw = float(rng.uniform(5.0, 1.5 * r_out)) if 1.5 * r_out > 5.0 else 5.0
        ca, cb = float(rng.uniform(-r_out, r_out)), float(rng.uniform(-r_out, r_out))
        tol = (1e-7, 1e-9, 1e-11)[int(rng.integers(3))]
        out.append(dict(M=M, a=a, r_obs=r_obs, theta=theta, r_in=r_in, r_out=r_out, alims=(ca - hw, ca + hw), blims=(cb - hw, cb + hw),
                        max_time=max_time, outer=12000.0, tol=tol, gtol=gtol, tile_seed=int(rng.integers(1 << 31))))
    return out


def random_scenes(G, seed, n, size=64):
    """[(parameters, (metric, observer, disc, max_time, render keywords))], the same draw for the same seed."""
    return [(p, _build(G, p, size)) for p in random_parameters(seed, n)]


def random_tiles(p, size=64, count=16):
    """The 8 x 8 tiles of a random scene's image the host traces: `count` of them, chosen by the scene's own seed."""
    nt = (size // 8) ** 2
    return np.sort(np.random.default_rng(p["tile_seed"]).choice(nt, size=min(count, nt), replace=False))


def configuration(G, built):
    """The TracingConfiguration and the point function of a scene as _build returns it; its gate must be finite: a scene the gate
    switches off compares nothing, and is a bug in this file."""
    import harness_culls as H

    m, x, d, max_time, kw = built
    cfg = G.render_configuration(m, x, d, max_time, **kw)
    rc = H.gate_radius(cfg)
    assert math.isfinite(rc), ("gated off", m, x, d, kw)
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    return cfg, pf, rc


def host_arms(G, built, tiles):
    """(configuration, R_cull, the library as shipped, every cull off) on the host build: harness_culls.render_tiles with
    the arms "all" and "full" of its DEFER table."""
    import harness_culls as H

    cfg, pf, rc = configuration(G, built)
    on = H.render_tiles(G, cfg, pf, tiles, *H.DEFER[0]["all"][:4], -1.0)
    off = H.render_tiles(G, cfg, pf, tiles, *H.DEFER[0]["full"])
    return cfg, rc, on, off


def counts(G, on, off):
    """What each mechanism ended, and what that left of the uncut trace's work."""
    hit = int(G.StatusCodes.IntersectedWithGeometry)
    start, defer, entry = on["at_start"] == 1, on["defer_end"] == 1, on["entry_step"] > 0
    early = start | defer | entry
    att_on = on["nacc"].astype(np.int64) + on["nrej"]
    att_off = off["nacc"].astype(np.int64) + off["nrej"]
    nacc_off = int(off["nacc"].sum())
    return {"start": int(start.sum()), "defer": int(defer.sum()), "entry": int(entry.sum()),
            "step": int(np.sum(~early & (att_on < att_off))),
            "wrongly_ended": int(np.sum(early & (off["status"] == hit))),
            "hit_share": float(np.mean(off["status"] == hit)),
            "whole_tiles_decided": int(np.sum(att_on.max(axis=1) == 0)),
            "attempted_on": int(att_on.sum()), "attempted_off": int(att_off.sum()),
            "accepted_on": int(on["nacc"].sum()), "accepted_off": nacc_off,
            "step_ratio": float(on["nacc"].sum() / nacc_off) if nacc_off else 1.0}


def fired(c):
    return {k for k in MECHANISMS if c[k] > 0}


if __name__ == "__main__":
    import os
    import sys
    import time

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gradus_jl_amd as G

    if "--random" in sys.argv:
        silent = 0
        for i, (p, built) in enumerate(random_scenes(G, SEED, N_RANDOM)):
            _, rc, on, off = host_arms(G, built, random_tiles(p))
            c = counts(G, on, off)
            silent += not (c["start"] or c["defer"] or c["entry"])
            print(i, f"M {p['M']:.2f} a {p['a']:+.2f} th {p['theta']:.0f} r_obs {p['r_obs']:.1f} R_cull {rc / p['M']:.2f} "
                     f"t/r {p['max_time'] / p['r_obs']:.1f}", {k: c[k] for k in MECHANISMS}, f"{c['step_ratio']:.3f}",
                  "same" if on["image"].tobytes() == off["image"].tobytes() and np.array_equal(on["status"], off["status"]) else "DIFFERENT")
        print(f"seed {SEED}: {silent} of {N_RANDOM} scenes end no ray early")
    else:
        size = int(sys.argv[1]) if len(sys.argv) > 1 else 64
        print("| scene | R_cull / M | hit share | start | defer | entry | step | whole tiles | accepted steps on / off | ratio | s |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        table = {}
        for name in NAMED:
            t0 = time.time()
            _, rc, on, off = host_arms(G, scene(G, name, size), np.arange((size // 8) ** 2))
            c = table[name] = counts(G, on, off)
            same = on["image"].tobytes() == off["image"].tobytes() and np.array_equal(on["status"], off["status"])
            print(f"| `{name}` | {rc / parameters(name)['M']:.4g} | {c['hit_share']:.3f} | {c['start']} | {c['defer']} | {c['entry']} | "
                  f"{c['step']} | {c['whole_tiles_decided']} | {c['accepted_on']} / {c['accepted_off']} | {c['step_ratio']:.3f} | "
                  f"{time.time() - t0:.1f} |" + ("" if same and c["wrongly_ended"] == 0 else "  DIFFERENT"), flush=True)
        print("FIRES = {")
        for name in NAMED:
            f = [k for k in MECHANISMS if k in fired(table[name])]
            print(f'    "{name}": ' + ("{" + ", ".join(f'"{k}"' for k in f) + "}" if f else "set()") + ",")
        print("}")
