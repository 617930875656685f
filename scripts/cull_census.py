#!/usr/bin/env python3
"""CPU census of the start cull and the step loop's culls (Ray::init, Ray::step) on the bench plane.

Random whole 8 x 8 tiles of the 2048² bench image (Kerr a = 0.998, observer r = 1000, θ = 75°, ThinDisc(isco, 50), λ1 = 2000),
lanes as the one-ray-per-lane kernel lays them out, are stepped through the KERNEL's own logic compiled for the host
(tests/host_harness_culls.cpp) four times: both mechanisms off, the start cull alone, the step loop's culls alone, both.  Printed:
steps per arm, the sum over tiles of the longest lane's steps (the cost of one wave per tile), how many rays each arm ended early
and how many of those the full trace says hit the disc (must be 0), whether pixels and statuses are the same bytes in all arms,
and the ratio of accepted steps that GRADUS_MI355X_ESCAPE_CULL unset / =0 shows on this build.  The step loop's arm here holds the
escape cull (r > R_cull) and the polar-rate cull together, as the switch does.  CPU only.  Every arm's record has the keys of
tests/harness_culls.py census(), whichever mechanism it belongs to.

With --pass-cull the same tiles are traced with the pass cull (Ray::start_decided) on
against off under the start cull alone and under all culls, and the result gains a "pass_cull" entry: steps and wave-steps of
the four arms, how many rays the pass cull decided (and how many of those hit the disc: must be 0), the ratio of wave-steps it
leaves, and the GRADUS_MI355X_ESCAPE_CULL switch ratio with it on.  --zeta tries another R_pass = ζ R_cull than the library's.

With --entry-cull the same tiles are traced by the library as shipped ("all"), the entry cull
(Ray::step) off alone ("no-entry") and the step loop's culls off ("start"), at the library's ζ or at --zeta.  The result gains an
"entry_cull" entry: steps and wave-steps of the arms, how many rays ended on entry, at which steps, and how many of those hit
the disc (must be 0), the ratios the entry cull leaves and the GRADUS_MI355X_ESCAPE_CULL switch ratio.  --ref-zeta Z adds the
wave-steps and accepted steps relative to a library with R_pass = Z R_cull and no entry cull (0.75: the one before the entry cull).

With --defer-cull the same tiles are traced by the library as shipped ("all"), the defer cull
(Ray::start_decided, Ray::step) off alone ("no-defer"), the step loop's culls off ("start") and every cull off ("full"), at the
library's ζ and ζ_defer or at --zeta and --defer-zeta (the latter builds the harness with that constant).  The result gains a
"defer_cull" entry: steps and wave-steps of the arms, how many rays the start marked, how many the defer cull and the entry cull
ended (and how many of all early ends hit the disc: must be 0), the ratios the defer cull leaves and the
GRADUS_MI355X_ESCAPE_CULL switch ratio.  --ref-zeta Z adds the steps relative to R_pass = Z R_cull without the defer cull (0.55:
the library before it).

    python scripts/cull_census.py [--tiles 1000] [--seed 1] [--pass-cull [--zeta 0.72] [--pass-only]]
    python scripts/cull_census.py --tiles 1500 --seed 3 --entry-cull --pass-only [--zeta 0.60] [--ref-zeta 0.75]
    python scripts/cull_census.py --tiles 1500 --seed 3 --defer-cull --pass-only [--zeta 0.50] [--defer-zeta 0.35] [--ref-zeta 0.55]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _bench(tiles, seed):
    """(G, the harness, the bench scene's configuration and point function, `tiles` of its tiles drawn with `seed`)"""
    import gradus_jl_amd as G
    import harness_culls as H
    from cull_scenes import SIZE, bench_scene

    cfg, pf = bench_scene(G)
    nt = SIZE // 8
    return G, H, cfg, pf, np.random.default_rng(seed).choice(nt * nt, size=tiles, replace=False)


def census(tiles=1000, seed=1):
    G, H, cfg, pf, picks = _bench(tiles, seed)
    res, _ = H.census(G, cfg, pf, picks, *H.STEP)
    res["seed"] = int(seed)
    res["r_cull"] = H.gate_radius(cfg)
    return res


def pass_census(tiles=1000, seed=1, zeta=-1.0):
    """The pass cull's arms on the tiles census() draws for the same arguments (zeta < 0: the library's)."""
    G, H, cfg, pf, picks = _bench(tiles, seed)
    res, _ = H.census(G, cfg, pf, picks, *H.PASS, zeta=zeta)
    res["seed"] = int(seed)
    res["zeta"] = H.zeta() if zeta < 0 else float(zeta)
    res["r_cull"] = H.gate_radius(cfg)
    res["r_pass"] = res["zeta"] * res["r_cull"]
    return res


def entry_census(tiles=1000, seed=1, zeta=-1.0, ref_zeta=None):
    """The entry cull's arms on the tiles census() draws for the same arguments (zeta < 0: the library's)."""
    G, H, cfg, pf, picks = _bench(tiles, seed)
    res, _ = H.census(G, cfg, pf, picks, *H.ENTRY, zeta=zeta)
    res["seed"] = int(seed)
    res["zeta"] = H.zeta() if zeta < 0 else float(zeta)
    res["zeta_dip"] = H.zeta_dip()
    res["r_cull"] = H.gate_radius(cfg)
    if ref_zeta is not None:
        ref = H.render_tiles(G, cfg, pf, picks, entry=0, zeta=ref_zeta)
        att = ref["nacc"].astype(np.int64) + ref["nrej"]
        res["ref_zeta"] = float(ref_zeta)
        res["wave_steps_vs_ref"] = res["arms"]["all"]["wave_steps"] / int(att.max(axis=1).sum())
        res["accepted_steps_vs_ref"] = res["arms"]["all"]["accepted_steps"] / int(ref["nacc"].sum())
        res["no_entry_wave_steps_vs_ref"] = res["arms"]["no-entry"]["wave_steps"] / int(att.max(axis=1).sum())
    return res


def defer_census(tiles=1000, seed=1, zeta=-1.0, defer_zeta=None, ref_zeta=None):
    """The defer cull's arms on the tiles census() draws for the same arguments (zeta < 0, defer_zeta None: the library's)."""
    G, H, cfg, pf, picks = _bench(tiles, seed)
    res, _ = H.census(G, cfg, pf, picks, *H.DEFER, zeta=zeta, defer_zeta=defer_zeta)
    res["seed"] = int(seed)
    res["zeta"] = H.zeta() if zeta < 0 else float(zeta)
    res["zeta_defer"] = H.zeta_defer(defer_zeta)
    res["zeta_dip"] = H.zeta_dip()
    res["r_cull"] = H.gate_radius(cfg)
    if ref_zeta is not None:
        ref = H.render_tiles(G, cfg, pf, picks, defer=0, zeta=ref_zeta, defer_zeta=defer_zeta)
        att = ref["nacc"].astype(np.int64) + ref["nrej"]
        res["ref_zeta"] = float(ref_zeta)
        res["wave_steps_vs_ref"] = res["arms"]["all"]["wave_steps"] / int(att.max(axis=1).sum())
        res["accepted_steps_vs_ref"] = res["arms"]["all"]["accepted_steps"] / int(ref["nacc"].sum())
        res["attempted_steps_vs_ref"] = res["arms"]["all"]["attempted_steps"] / int(att.sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--pass-cull", action="store_true", help="add the pass cull's arms")
    ap.add_argument("--zeta", type=float, default=-1.0, help="R_pass / R_cull (default: the library's constant)")
    ap.add_argument("--pass-only", action="store_true", help="with --pass-cull, --entry-cull or --defer-cull: skip the four arms of the older culls")
    ap.add_argument("--entry-cull", action="store_true", help="add the entry cull's arms")
    ap.add_argument("--ref-zeta", type=float, default=None,
                    help="with --entry-cull / --defer-cull: compare with R_pass / R_cull = this and no entry / defer cull")
    ap.add_argument("--defer-cull", action="store_true", help="add the defer cull's arms")
    ap.add_argument("--defer-zeta", type=float, default=None, help="R_defer / R_cull (default: the library's constant)")
    a = ap.parse_args()
    res = {} if ((a.pass_cull or a.entry_cull or a.defer_cull) and a.pass_only) else census(a.tiles, a.seed)
    if a.pass_cull:
        res["pass_cull"] = pass_census(a.tiles, a.seed, a.zeta)
    if a.entry_cull:
        res["entry_cull"] = entry_census(a.tiles, a.seed, a.zeta, a.ref_zeta)
    if a.defer_cull:
        res["defer_cull"] = defer_census(a.tiles, a.seed, a.zeta, a.defer_zeta, a.ref_zeta)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
