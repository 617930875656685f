#!/usr/bin/env python3
"""Wall time of integrating transfer functions into a line profile -- `integrate_lineprofile`, 1000 annuli, 7 quadrature nodes --
by the host route (the numpy loop over the annuli), by one device call (`ensemble=`: gr_tf_lineprofile) and by a batch of 64
sets in one call (`integrate_lineprofiles`: the shape of a spectral fit), on two inputs:

  scene   the default line profile: Kerr a = 0.998 seen from 40 degrees, 100 transfer functions out to r = 50 traced on the
          device (ragged branches), 180 g bins
  table   a point of a transfer-function table: 150 radii x 20 knots on one g* axis (synthetic, no tracing), 180 g bins

and of `integrate_lagtransfer` with 400 t bins on the scene.  One warm-up of every route, then `--reps` repetitions with the
routes alternating; every device call ends in a synchronise inside the library.  Prints one JSON line: median, min and max per
piece in ms and the largest difference between the routes in units of the peak.  For the kernels alone run it under
`rocprofv3 --kernel-trace --stats -- python scripts/tfint_time.py --reps 3` and read k_tf off the statistics."""
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
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--n-radii", type=int, default=1000)
args = ap.parse_args()

TF = G.transfer_functions
ens = G.EnsembleMI355X(0)
bins = np.linspace(0.1, 1.5, 181)
t_grid = np.linspace(0.0, 400.0, 401)
ε = lambda r: r ** -3.0


class Prof:
    def emissivity_at(self, r):
        return r ** -3.0

    def coordtime_at(self, r):
        return math.sqrt(r * r + 100.0)


def table_point(n_r=150, n_k=20):
    gs = np.linspace(0.0, 1.0, n_k)
    r = np.asarray(G.InverseGrid()(1.25, 500.0, n_r))
    u = 1.0 - r[0] / r
    f_lo = (0.3 + 2.0 * gs * (1.0 - gs))[:, None] * (1.0 + 0.1 * np.sin(r))[None, :]
    f_up = (0.5 + 1.2 * np.sqrt(gs * (1.0 - gs)))[:, None] * (1.0 + 0.1 * np.cos(r))[None, :]
    t_lo = 40.0 + r[None, :] * (1.0 - 0.6 * np.cos(math.pi * gs))[:, None]
    t_up = 40.0 + r[None, :] * (1.0 + 0.8 * np.sin(math.pi * gs) - 0.6 * np.cos(math.pi * gs))[:, None]
    return TF.CunninghamTransferGrid(r, gs, 0.2 + 0.55 * u, 1.35 - 0.3 * u, f_lo, f_up, t_lo, t_up)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


m = G.KerrMetric(1.0, 0.998)
x = np.array([0.0, 1000.0, math.radians(40), 0.0])
tfs_scene, t_trace = timed(lambda: TF.transferfunctions(m, x, G.ThinDisc(0.0, 400.0), maxrₑ=50.0, numrₑ=100, ensemble=ens))
inputs = {"scene": tfs_scene, "table": table_point()}
kw = dict(n_radii=args.n_radii)
routes = {}
for name, tfs in inputs.items():
    routes[f"{name}_host"] = lambda tfs=tfs: TF.integrate_lineprofile(ε, tfs, bins, **kw)
    routes[f"{name}_device"] = lambda tfs=tfs: TF.integrate_lineprofile(ε, tfs, bins, ensemble=ens, **kw)
    routes[f"{name}_device_batch{args.batch}"] = lambda tfs=tfs: TF.integrate_lineprofiles([ε] * args.batch, [tfs] * args.batch, bins,
                                                                                             ensemble=ens, **kw)
routes["scene_lag_host"] = lambda: TF.integrate_lagtransfer(Prof(), tfs_scene, bins, t_grid, t0=x[1], **kw)
routes["scene_lag_device"] = lambda: TF.integrate_lagtransfer(Prof(), tfs_scene, bins, t_grid, t0=x[1], ensemble=ens, **kw)

results = {k: f() for k, f in routes.items()}          # warm-up
times = {}
for _ in range(args.reps):
    for k, f in routes.items():
        results[k], dt = timed(f)
        times.setdefault(k, []).append(dt)
peak = lambda a: float(np.max(np.abs(a)))
assert all(peak(results[f"{name}_host"]) > 0.0 for name in ("scene", "table", "scene_lag"))
diff = {name: float(np.max(np.abs(results[f"{name}_device"] - results[f"{name}_host"]))) / peak(results[f"{name}_host"])
        for name in ("scene", "table", "scene_lag")}
for name in inputs:
    b = results[f"{name}_device_batch{args.batch}"]
    assert all(row.tobytes() == results[f"{name}_device"].tobytes() for row in b)
print(json.dumps({"n_radii": args.n_radii, "g_bins": bins.size - 1, "t_bins": t_grid.size - 1, "reps": args.reps, "batch": args.batch,
                  "transferfunctions_ms": round(t_trace, 1), "device_minus_host_of_peak": diff,
                  "ms": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                         for k, v in times.items()}}))
