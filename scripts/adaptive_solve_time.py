#!/usr/bin/env python3
"""The resident adaptive sky against the host route, and one full adaptive_solve.  The walk-through scene of
scripts/adaptive_sky_time.py (RingCorona r = 10, h = 4, Kerr a = 0.998, ThinDisc(0, ∞)):

  * trace_step 1 ... `--steps` on a host-route sky and on a resident one, in this one run: wall time of the step, the part of it
    on the device up to the end of the trace launch (host route: gr_stats.call_ms of gr_sky_cells; resident: from the children
    kernel to the end of the gr_sky_cells_device launch) and the share outside it;
  * adaptive_solve with the reference's defaults (N = 500) on a resident sky: iterations, cells, time per iteration.

    python scripts/adaptive_solve_time.py [--steps 3] [--pairs 0|1|2] [--no-solve]

Needs an MI355X.  Its numbers are reported in DESIGN_measurements.md §M32 (next to those of §M31)."""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M31_MS = (15.4, 20.8, 156.7)        # DESIGN_measurements.md §M31: wall time of trace_step 1, 2, 3 on the host route


def steps(G, ens, scene, resident, n_steps):
    sky = G.AdaptiveSky(*scene, ensemble=ens, resident=resident)
    launches = sky.tracer["launches"]
    G.trace_initial(sky)
    out = []
    for _ in range(n_steps):
        first = len(launches)
        t0 = time.perf_counter()
        G.trace_step(sky)
        wall = 1e3 * (time.perf_counter() - t0)
        out.append((sum(n for n, _ in launches[first:]), wall, sum(ms for _, ms in launches[first:]), sky.n_cells))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=2, help="gr_ctx_set tangent_pairs: 0 one lane per ray, 1 a pair of lanes, 2 by launch size")
    ap.add_argument("--no-solve", action="store_true")
    args = ap.parse_args()

    import gradus_jl_amd as G

    ens = G.EnsembleMI355X(0, tangent_pairs=args.pairs)
    scene = (G.KerrMetric(1.0, 0.998), G.RingCorona(r=10.0, h=4.0), G.ThinDisc(0.0, math.inf))
    steps(G, ens, scene, True, 1)           # (warm-up: the context, the plunging table, the kernels' code objects)
    for label, resident in (("host", False), ("resident", True)):
        for k, (cells, wall, inside, grid) in enumerate(steps(G, ens, scene, resident, args.steps)):
            was = f"  (§M31: {M31_MS[k]:6.1f} ms)" if not resident and k < len(M31_MS) else ""
            print(f"{label:<9} trace_step {k + 1}  cells traced {cells:>8}  wall {wall:9.2f} ms  to the end of the launch {inside:9.2f} ms  "
                  f"outside {1.0 - inside / wall:6.1%}  grid {grid:>8} cells{was}")
    if args.no_solve:
        return
    m, _, d = scene
    sky = G.AdaptiveSky(*scene, ensemble=ens, resident=True)
    t0 = time.perf_counter()
    n = G.adaptive_solve(m, d, sky, verbose=True)       # (one line per iteration on stderr, with the time since the start)
    wall = time.perf_counter() - t0
    print(f"adaptive_solve (resident, N = 500): {n} iterations, {sky.n_cells} cells, {wall:.2f} s")


if __name__ == "__main__":
    main()
