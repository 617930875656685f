#!/usr/bin/env python3
"""Wall time of `integrate_lagtransfer` for a time-dependent emissivity: a DiscCoronaProfile of 10 rings x 2 arms x 100 slices
(closed-form curves of 8 knots, no tracing) over a synthetic table of transfer functions (150 radii x 20 knots), 1000 annuli x
180 g bins x 400 t bins x 100 time samples -- by the host route (the numpy loop of transfer_functions.py, once: it takes about a
minute) and by the device call (`ensemble=`: gr_tf_lagtransfer_td), one warm-up and `--reps` repetitions; every device call
ends in a synchronise inside the library.  Prints one JSON line: ms per route and the largest difference between the routes in
units of the peak.  For the two kernels alone run it under
`rocprofv3 --kernel-trace --stats -- python scripts/tftd_time.py --reps 3 --no-host` and read k_tftd_em and k_tftd off the
statistics."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: the order tests/conftest.py has)

import gradus_jl_amd as G

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--n-radii", type=int, default=1000)
ap.add_argument("--n-rings", type=int, default=10)
ap.add_argument("--n-slices", type=int, default=100)
ap.add_argument("--n-time", type=int, default=100)
ap.add_argument("--no-host", action="store_true", help="skip the numpy route")
args = ap.parse_args()

TF = G.transfer_functions
bins = np.linspace(0.1, 1.5, 181)
t_grid = np.linspace(0.0, 400.0, 401)
HEIGHT = 5.0


def table_point(n_r=150, n_k=20):
    gs = np.linspace(0.0, 1.0, n_k)
    r = np.asarray(G.InverseGrid()(1.25, 500.0, n_r))
    u = 1.0 - r[0] / r
    f_lo = (0.3 + 2.0 * gs * (1.0 - gs))[:, None] * (1.0 + 0.1 * np.sin(r))[None, :]
    f_up = (0.5 + 1.2 * np.sqrt(gs * (1.0 - gs)))[:, None] * (1.0 + 0.1 * np.cos(r))[None, :]
    t_lo = 40.0 + r[None, :] * (1.0 - 0.6 * np.cos(math.pi * gs))[:, None]
    t_up = 40.0 + r[None, :] * (1.0 + 0.8 * np.sin(math.pi * gs) - 0.6 * np.cos(math.pi * gs))[:, None]
    return TF.CunninghamTransferGrid(r, gs, 0.2 + 0.55 * u, 1.35 - 0.3 * u, f_lo, f_up, t_lo, t_up)


def arm(R, side, n):
    """n slices of the ring of radius R at height 5: the light travel time to the disc point (ρ, β away), on 8 knots from 1 to 600"""
    βs = (np.arange(n) + 0.5) / n * math.pi + (math.pi if side == "right" else 0.0)
    ρ = 1.0 * 600.0 ** (np.arange(8) / 7.0)
    t = [np.sqrt(HEIGHT ** 2 + ρ ** 2 + R ** 2 - 2.0 * ρ * R * math.cos(β)) for β in βs]
    ε = [(1.0 + 0.3 * math.cos(β)) * (HEIGHT ** 2 + ρ ** 2) ** -1.5 for β in βs]
    return G.TimeDependentRadialDiscProfile(np.ones(n), [ρ] * n, t, ε)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


ring_radii = np.linspace(1e-2, 5.0, args.n_rings)
prof = G.DiscCoronaProfile(ring_radii, [G.RingCoronaProfile(arm(R, "left", args.n_slices), arm(R, "right", args.n_slices)) for R in ring_radii])
tfs = table_point()
kw = dict(n_radii=args.n_radii, n_time_steps=args.n_time, rmax=50.0)
ens = G.EnsembleMI355X(0)
device = lambda: TF.integrate_lagtransfer(prof, tfs, bins, t_grid, ensemble=ens, **kw)
got = device()          # warm-up
times = []
for _ in range(args.reps):
    got, dt = timed(device)
    times.append(dt)
out = {"n_radii": args.n_radii, "g_bins": bins.size - 1, "t_bins": t_grid.size - 1, "n_time": args.n_time, "rings": args.n_rings,
       "slices_per_arm": args.n_slices, "reps": args.reps,
       "device_ms": {"median": round(statistics.median(times), 2), "min": round(min(times), 2), "max": round(max(times), 2)}}
assert np.max(got) > 0.0
if not args.no_host:
    want, out["host_ms"] = timed(lambda: TF.integrate_lagtransfer(prof, tfs, bins, t_grid, **kw))
    out["host_ms"] = round(out["host_ms"], 1)
    out["device_minus_host_of_peak"] = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
print(json.dumps(out))
