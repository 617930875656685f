#!/usr/bin/env python3
"""CPU census of the escape cull (Ray::step) on oracle-traced rays of the bench plane.

Random whole 8 x 8 tiles of the 2048² bench image (Kerr a = 0.998, observer r = 1000, θ = 75°, ThinDisc(isco, 50), λ1 = 2000),
lanes column-major as the one-ray-per-lane kernel lays them out, are traced step by step with the oracle.  A ray meets the cull
test at the first accepted step k whose end lies beyond R_cull with r rising (the stand-in for v^r > 0 here: the oracle records
r and λ per accepted step only).  Printed: accepted steps per ray and the sum over tiles of the longest lane's steps (the cost of
one wave per tile), for the full trace and for the trace up to the cull; plus the checks that make the cull exact on these rays:
no ray that hits the disc meets the test before its event, no accepted step after the test has r <= R_cull, and r stays under
the bound r_k + B(r_k) (λ - λ_k) of the E/L speed bound.  CPU only.

    python scripts/escape_census.py [--tiles 1000] [--seed 1]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O  # noqa: E402

M, A = 1.0, 0.998
SIZE, ALIMS, BLIMS = 2048, (-60.0, 60.0), (-35.0, 35.0)
X_OBS = np.array([0.0, 1000.0, math.radians(75.0), 0.0])


def bench_config():
    isco = O.isco(O.make_config("kerr", (M, A)))
    return O.make_config("kerr", (M, A), disc=(isco, 50.0), lambda_max=2000.0)


def r_cull(cfg):
    """What the host passes for this scene (escape_cull_radius): (1 + 1e-6) max(4M, r_out / sqrt(1 - gtol²))."""
    return (1.0 + 1e-6) * max(4.0 * M, cfg.disc_r_out / math.sqrt(1.0 - cfg.gtol ** 2))


def speed_bound(r, E, L):
    """KerrFamily::radial_speed_bound: |dr/dλ| <= (|E| (r² + a²) + |a L|) / r² for every r' >= r."""
    return abs(E) + (abs(E) * A * A + abs(A * L)) / (r * r)


def census(tiles=1000, seed=1):
    cfg = bench_config()
    R = r_cull(cfg)
    rng = np.random.default_rng(seed)
    nt = SIZE // 8
    picks = rng.choice(nt * nt, size=tiles, replace=False)
    g0, _, _ = O.metric_jacobian(cfg, X_OBS[1], X_OBS[2])
    full_steps = cull_steps = 0
    wave_full = wave_cull = 0
    rays = hits = 0
    hit_meets_test = after_inside = bound_broken = 0
    for tile in picks:
        tc, tr = divmod(int(tile), nt)
        lane_full, lane_cull = [], []
        for col in range(8 * tc, 8 * tc + 8):
            i0 = col * SIZE + 8 * tr
            vs = O.render_velocities(cfg, X_OBS, ALIMS, BLIMS, SIZE, SIZE, i0, 8)
            for v in vs:
                pt, t, r = O.trace_steps(cfg, X_OBS, v)
                n = len(t) - 1                          # accepted steps (t[0], r[0]: the start)
                hit = int(pt["status"]) == O.INTERSECTED_WITH_GEOMETRY
                k = next((j for j in range(1, n + 1) if r[j] > R and r[j] > r[j - 1]), None)
                if hit and k is not None and k < n:
                    hit_meets_test += 1
                if k is not None and not hit:
                    after_inside += int(np.sum(r[k + 1:] <= R))
                    E = -(g0[0] * v[0] + g0[4] * v[3])      # conserved: formed at the start
                    L = g0[4] * v[0] + g0[3] * v[3]
                    lim = r[k] + speed_bound(r[k], E, L) * (t[k:] - t[k])
                    bound_broken += int(np.sum(r[k:] > lim * (1.0 + 1e-12)))
                c = k if (k is not None and not hit) else n
                lane_full.append(n)
                lane_cull.append(c)
                rays += 1
                hits += int(hit)
        full_steps += sum(lane_full)
        cull_steps += sum(lane_cull)
        wave_full += max(lane_full)
        wave_cull += max(lane_cull)
    return {"tiles": int(tiles), "seed": int(seed), "rays": rays, "hit_fraction": hits / rays, "r_cull": R,
            "accepted_steps_per_ray_full": full_steps / rays, "accepted_steps_per_ray_culled": cull_steps / rays,
            "steps_ratio": cull_steps / full_steps, "wave_steps_full": wave_full, "wave_steps_culled": wave_cull,
            "wave_steps_ratio": wave_cull / wave_full, "hits_meeting_test_before_event": hit_meets_test,
            "steps_inside_r_cull_after_test": after_inside, "steps_beyond_speed_bound": bound_broken}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    print(json.dumps(census(a.tiles, a.seed), indent=1))


if __name__ == "__main__":
    main()
