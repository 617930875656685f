#!/usr/bin/env python3
"""Where does an adaptive sky's time go?  The walk-through scene of the reference's adaptive-tracing docs -- RingCorona r = 10,
h = 4, Kerr a = 0.998, ThinDisc(0, ∞) -- traced to its initial level and refined `--steps` times with the default criterion.
Per refinement step: cells traced, wall time of the step, the part of it inside the gr_sky_cells calls (host staging, the
launch, the copy home: gr_stats.call_ms) and the share outside them (find_need_refine, the grid's bookkeeping).

    python scripts/adaptive_sky_time.py [--steps 3] [--level 3] [--pairs 0|1|2]

Needs an MI355X.  Its numbers are reported in DESIGN_measurements.md §M31."""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=2, help="gr_ctx_set tangent_pairs: 0 one lane per ray, 1 a pair of lanes, 2 by launch size")
    args = ap.parse_args()

    import gradus_jl_amd as G

    ens = G.EnsembleMI355X(0, tangent_pairs=args.pairs)
    m, corona, d = G.KerrMetric(1.0, 0.998), G.RingCorona(r=10.0, h=4.0), G.ThinDisc(0.0, math.inf)
    t0 = time.perf_counter()
    sky = G.AdaptiveSky(m, corona, d, ensemble=ens)
    print(f"setup (context, plunging table): {1e3 * (time.perf_counter() - t0):.1f} ms")
    launches = sky.tracer["launches"]

    def report(label, wall, first):
        cells = sum(n for n, _ in launches[first:])
        inside = sum(ms for _, ms in launches[first:])
        share = 1.0 - inside / wall if wall > 0 else 0.0
        print(f"{label:<14} cells traced {cells:>8}  wall {wall:9.2f} ms  in gr_sky_cells {inside:9.2f} ms  outside {share:6.1%}  "
              f"grid {len(sky.grid):>8} cells")

    t0 = time.perf_counter()
    G.trace_initial(sky, level=args.level)
    report(f"initial (L{args.level})", 1e3 * (time.perf_counter() - t0), 0)
    for k in range(args.steps):
        first = len(launches)
        t0 = time.perf_counter()
        G.trace_step(sky)
        report(f"trace_step {k + 1}", 1e3 * (time.perf_counter() - t0), first)


if __name__ == "__main__":
    main()
