#!/usr/bin/env python3
"""Time a TraceRadiativeTransfer render of the torus scene beside the plain fp64 end-point trace of the same plane and geometry
(DESIGN_measurements.md §M40).

    python scripts/transfer_time.py [--size 1024] [--reps 10] [--plain-only]

The scene is scene A of tests/transfer_scene.py (Schwarzschild, observer r = 100 at 85°, the torus of radius 1 round ρ = 10) on the
plane α in [-14, 14], β in [-5, 5].  Both traces are warmed up once and then alternated `reps` times; the figure per launch is
gr_stats.kernel_ms (device events round the call's device work).  --plain-only: the plain trace alone, for a library that has no
radiative-transfer kernels (GRADUS_MI355X_LIB names the library to load).
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process: tests/conftest.py)

    import gradus_jl_amd as G

    m = G.KerrMetric(1.0, 0.0)
    x = np.array([0.0, 100.0, math.radians(85.0), 0.0])
    d = G.ThickDisc(lambda r: math.sqrt(max(1.0 - (r - 10.0) ** 2, 0.0)) if 9.0 <= r <= 11.0 else -1.0, ρ_range=(9.0, 11.0), samples=1 << 16)
    ens = G.EnsembleMI355X(0)
    kw = dict(image_width=args.size, image_height=args.size, alpha_lims=(-14.0, 14.0), beta_lims=(-5.0, 5.0), ensemble=ens)

    def plain():
        cfg = G.render_configuration(m, x, d, 200.0, **kw)
        return G.ensemble_solve_tracing_problem(ens, cfg, stats=True)[1]

    def transfer():
        trace = G.TraceRadiativeTransfer(I0=0.0, medium=G.PowerLawMedium(j0=0.1))
        return G.rendergeodesics(m, x, d, 200.0, trace=trace, stats=True, **kw)[3]

    runs = {"plain_endpoints": plain} if args.plain_only else {"plain_endpoints": plain, "transfer_render": transfer}
    for f in runs.values():
        f()
    ms = {k: [] for k in runs}
    steps = {}
    for _ in range(args.reps):
        for k, f in runs.items():
            st = f()
            ms[k].append(st["kernel_ms"])
            steps[k] = (st["accepted_steps"] + st["rejected_steps"]) / max(st["rays"], 1)
    out = {"library": G._lib.LIB_PATH, "size": args.size, "reps": args.reps}
    for k, v in ms.items():
        out[k] = {"kernel_ms_median": float(np.median(v)), "kernel_ms_min": float(np.min(v)), "kernel_ms_max": float(np.max(v)),
                  "steps_per_ray": steps[k]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
