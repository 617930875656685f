#!/usr/bin/env python3
"""The (r, ϕ) maps and the filled image of a resident adaptive sky, formed on the device against the numpy route on the mirror.
Scene: the default adaptive_solve sky of scripts/adaptive_solve_time.py (RingCorona r = 10, h = 4, Kerr a = 0.998,
ThinDisc(0, ∞), N = 500), resident.  In this one run:

  * route="device": bin_emissivity_grid, bin_redshift_grid, bin_time_grid on 500 x 500 bins and fill_sky_values(sky, 1080) -- the
    first call (it allocates the work buffers) and the best of `--repeat` more;
  * route="host": the download of the mirror (a single run: it happens once per sky), then the three maps on it (single runs)
    and fill_sky_values on `--columns` of the 1080 columns (a subsample: the whole image is 1.17 million get_parent_index
    calls), scaled to 1080;
  * the bytes each route brings back from the device.

    python scripts/sky_maps_time.py [--repeat 3] [--columns 64] [--N 500] [--fill 1080]

Needs an MI355X.  Its numbers are reported in DESIGN_measurements.md §M33."""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--N", type=int, default=500)
    ap.add_argument("--fill", type=int, default=1080)
    args = ap.parse_args()

    import gradus_jl_amd as G

    ens = G.EnsembleMI355X(0)
    m, corona, d = G.KerrMetric(1.0, 0.998), G.RingCorona(r=10.0, h=4.0), G.ThinDisc(0.0, math.inf)
    sky = G.AdaptiveSky(m, corona, d, ensemble=ens, resident=True)
    (n_iter), solve_ms = timed(lambda: G.adaptive_solve(m, d, sky, verbose=False))
    cells = sky.n_cells
    print(f"adaptive_solve (resident, N = 500): {n_iter} iterations, {cells} cells, {solve_ms / 1e3:.2f} s")
    r_bins, ϕ_bins = np.geomspace(m.isco(), 1000.0, args.N), np.linspace(0.0, 2.0 * math.pi, args.N)
    ϕ_grid, θ_grid = np.linspace(-math.pi, math.pi, args.fill), np.linspace(0.0, math.pi, args.fill)
    maps = {"bin_emissivity_grid": lambda route: G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, sky, route=route),
            "bin_redshift_grid": lambda route: G.bin_redshift_grid(r_bins, ϕ_bins, sky, route=route),
            "bin_time_grid": lambda route: G.bin_time_grid(r_bins, ϕ_bins, sky, route=route)}

    device, device_ms = {}, {}
    for name, f in maps.items():
        device[name], first = timed(lambda: f("device"))
        best = min(timed(lambda: f("device"))[1] for _ in range(args.repeat))
        device_ms[name] = best
        print(f"device  {name:<20} {args.N} x {args.N}: first call {first:9.2f} ms, best of {args.repeat} more {best:9.2f} ms")
    filled, first = timed(lambda: G.fill_sky_values(sky, (ϕ_grid, θ_grid), route="device"))
    best = min(timed(lambda: G.fill_sky_values(sky, (ϕ_grid, θ_grid), route="device"))[1] for _ in range(args.repeat))
    device_ms["fill_sky_values"] = best
    print(f"device  {'fill_sky_values':<20} {args.fill} x {args.fill}: first call {first:9.2f} ms, best of {args.repeat} more {best:9.2f} ms")
    bins, points = args.N * args.N, args.fill * args.fill
    print(f"device  bytes brought back: {bins * (4 * 8 + 4 + 4)} per map (4 integers, a count and 4 flag bytes per bin), "
          f"{points * (6 * 8 + 2 * 8)} for the image (6 doubles and 2 cell indices per point)")

    _, download = timed(lambda: sky.grid)
    per_cell = 2 * 8 + 4 + 9 * 8 + 4 * 8 + 8 + 1 + 6 * 8
    print(f"host    download of the mirror (single run): {download:9.2f} ms, {cells * per_cell} bytes ({per_cell} per cell)")
    host_ms = {}
    for name, f in maps.items():
        ref, host_ms[name] = timed(lambda: f("host"))
        with np.errstate(invalid="ignore", divide="ignore"):
            both = (ref != 0) & np.isfinite(ref)
            worst = float(np.max(np.abs(device[name][both] / ref[both] - 1.0))) if both.any() else 0.0
        same = np.array_equal(ref != 0, device[name] != 0)
        print(f"host    {name:<20} {args.N} x {args.N}: single run {host_ms[name]:9.2f} ms; device against it: worst relative difference "
              f"{worst:.2e}, lit pattern {'equal' if same else 'DIFFERS'}")
    cols = np.linspace(0, args.fill - 1, args.columns).astype(int)
    (ref, ref_cells), sub = timed(lambda: G.fill_sky_values(sky, (ϕ_grid[cols], θ_grid), route="host", cells=True))
    host_ms["fill_sky_values"] = sub * args.fill / args.columns
    ok = all(np.array_equal(np.isnan(filled[f][:, cols]), np.isnan(ref[f])) for f in ref.dtype.names)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = max(float(np.nanmax(np.abs(filled[f][:, cols] - ref[f]) / np.maximum(np.abs(ref[f]), 1e-300), initial=0.0)) for f in ref.dtype.names)
    print(f"host    {'fill_sky_values':<20} {args.columns} of {args.fill} columns (a subsample, single run): {sub:9.2f} ms -> scaled to {args.fill} "
          f"columns {host_ms['fill_sky_values']:9.2f} ms; device against it: NaN pattern {'equal' if ok else 'DIFFERS'}, worst relative difference {worst:.2e}")
    for name in device_ms:
        with_download = host_ms[name] + download
        print(f"{name:<20} device {device_ms[name]:9.2f} ms   host {host_ms[name]:9.2f} ms (+ download {with_download:9.2f} ms)   "
              f"{'device not slower' if device_ms[name] <= with_download else 'DEVICE SLOWER'}")


if __name__ == "__main__":
    main()
