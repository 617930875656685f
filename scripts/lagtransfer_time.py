#!/usr/bin/env python3
"""Wall time of the reference's default lag-energy call -- lagtransfer on an 800 x 800 geometric polar plane with 10^4 corona
samples, binflux into 300 x 300 cells -- by the host route (`lagtransfer` + `binflux`: 152-byte end points back, a second call
for the redshift, np.add.at) and by the device route (`lagtransfer_device` + `binflux`: the rows stay on the device), and of
the device route's reductions by themselves.

One warm-up of every route, then `--reps` repetitions with the two routes alternating (other work shares the box: a
difference counts only against the spread); every timed call ends in a device synchronise inside the library.  Prints one
JSON line: median, min and max per piece in ms, and the two routes' sums of the matrix (they must agree: same rays, same
point function).  For the kernels alone run it under `rocprofv3 --kernel-trace --stats -- python scripts/lagtransfer_time.py
--reps 3` and read k_lag_prepare / k_lag_extrema / k_lag_bin off the statistics."""
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
ap.add_argument("--plane", type=int, default=800)
ap.add_argument("--samples", type=int, default=10_000)
ap.add_argument("--cells", type=int, default=300)
args = ap.parse_args()

ens = G.EnsembleMI355X(0)
m = G.KerrMetric(1.0, 0.998)
x = np.array([0.0, 1000.0, math.radians(60), 0.0])
d = G.ThinDisc(0.0, 1000.0)
model = G.LampPostModel(h=10.0)
plane = G.PolarPlane(G.GeometricGrid(), Nr=args.plane, Nθ=args.plane, r_max=50.0)


def kw():
    return dict(plane=plane, n_samples=args.samples, ensemble=ens,
                sampler=G.EvenSampler(G.BothHemispheres(), G.RandomGenerator(seed=1)))


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def host_route():
    tf, t_trace = timed(lambda: G.lagtransfer(m, x, d, model, **kw()))
    out, t_bin = timed(lambda: G.binflux(tf, N_E=args.cells, N_t=args.cells, ensemble=ens))
    return out, {"host_lagtransfer": t_trace, "host_binflux": t_bin, "host_total": t_trace + t_bin}


def device_route():
    tf, t_trace = timed(lambda: G.lagtransfer_device(m, x, d, model, **kw()))
    out, t_bin = timed(lambda: G.binflux(tf, N_E=args.cells, N_t=args.cells))
    # the reductions once more: gr_lagtransfer_extrema + gr_lagtransfer_bin without the trace in front
    _, t_again = timed(lambda: G.binflux(tf, N_E=args.cells, N_t=args.cells))
    _, t_lds = timed(lambda: G.binflux(tf, N_E=32, N_t=32))          # 1024 cells: the histogram in LDS
    return out, {"device_lagtransfer": t_trace, "device_binflux": t_bin, "device_total": t_trace + t_bin,
                 "device_binflux_again": t_again, "device_binflux_32x32_lds": t_lds, "hits": tf.n_hits}


host_route(), device_route()          # warm-up: code objects, the plunging table, page-locked blocks
times = {}
sums = {}
for _ in range(args.reps):
    for name, route in (("host", host_route), ("device", device_route)):
        (t, E, f), ts = route()
        sums[name] = float(np.nansum(f))
        for k, v in ts.items():
            times.setdefault(k, []).append(v)
res = {"plane": f"{args.plane}x{args.plane}", "samples": args.samples, "cells": f"{args.cells}x{args.cells}", "reps": args.reps,
       "hits": int(times.pop("hits")[0]), "nansum_host": sums["host"], "nansum_device": sums["device"],
       "ms": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()}}
print(json.dumps(res))
