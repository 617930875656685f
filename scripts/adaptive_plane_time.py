#!/usr/bin/env python3
"""An adaptive image plane against the uniform render it stands in for.  Scene: Kerr a = 0.998 seen from (0, 1000, 75°, 0),
ThinDisc(isco, 50), window (-60, 60) x (-35, 35), λ_max 2000.  In this one run, on one device:

  * a resident AdaptivePlane: trace_initial(level = 3), then trace_step (check_refine_plane, 20 %) until its finest cell is no
    wider than a pixel of a `--width`-wide uniform image (120 / 3^level <= 120 / width: level 7 for 2048), then the filled
    redshift image on that pixel grid (route="device");
  * rendergeodesics of the uniform image with redshift ∘ filter_intersected.

Reported for both: rays traced, trace launches, wall time.

    python scripts/adaptive_plane_time.py [--width 2048] [--repeat 2]

Needs an MI355X.  Its numbers are reported in DESIGN_measurements.md §M34."""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=2)
    args = ap.parse_args()

    import gradus_jl_amd as G

    ens = G.EnsembleMI355X(0)
    m = G.KerrMetric(1.0, 0.998)
    x = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
    d = G.ThinDisc(m.isco(), 50.0)
    α_lims, β_lims = (-60.0, 60.0), (-35.0, 35.0)
    width = args.width
    height = int(round(width * (β_lims[1] - β_lims[0]) / (α_lims[1] - α_lims[0])))
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    level = math.ceil(math.log(width) / math.log(3.0))

    for run in range(args.repeat):
        t0 = time.perf_counter()
        sky = G.AdaptivePlane(m, x, d, α_lims=α_lims, β_lims=β_lims, ensemble=ens, t_max=2000.0, resident=True)
        G.trace_initial(sky)
        steps = 0
        while True:
            before = sky.n_cells
            G.trace_step(sky)
            steps += 1
            if sky.n_cells == before or steps >= level - 3:
                break
        t_refine = time.perf_counter() - t0
        sizes = [n for n, _ in sky.tracer["launches"]]
        t1 = time.perf_counter()
        α_grid, β_grid = np.linspace(*α_lims, width), np.linspace(*β_lims, height)
        image = G.fill_sky_values(sky, (α_grid, β_grid), metric=m, pf=pf, route="device")
        t_fill = time.perf_counter() - t1
        finest = (α_lims[1] - α_lims[0]) / 3.0 ** (3 + steps)
        print(f"adaptive run {run}: {steps} steps, {sky.n_cells} cells, finest cell {finest:.4f} wide (pixel {120.0 / width:.4f}), rays traced {sum(sizes)} in "
              f"{len(sizes)} launches {sizes}, refinement {1e3 * t_refine:.1f} ms, fill {width} x {height} {1e3 * t_fill:.1f} ms "
              f"({np.isfinite(image).sum()} finite pixels), total {1e3 * (t_refine + t_fill):.1f} ms")
        del sky

    for run in range(args.repeat):
        t0 = time.perf_counter()
        _, _, img, st = G.rendergeodesics(m, x, d, 2000.0, image_width=width, image_height=height, alpha_lims=α_lims, beta_lims=β_lims, pf=pf,
                                          ensemble=ens, stats=True)
        t_render = time.perf_counter() - t0
        print(f"uniform run {run}: {width} x {height}, rays traced {st['rays']} in 1 launch, wall {1e3 * t_render:.1f} ms (kernel {st['kernel_ms']:.1f} ms, "
              f"{np.isfinite(img).sum()} finite pixels)")


if __name__ == "__main__":
    main()
