"""Time the producer of a DiscCorona's arms on the device: by default the reference's default case, 10 rings x 100 β slices x 1000
samples with 80 extremum iterations (src/corona/models/extended.jl:187-200).

    python scripts/ringarms_time.py [--rings 10] [--slices 100] [--samples 1000] [--extrema-iter 80] [--repeat 3]

Prints one JSON line: route "device" (one gr_ring_arms call) against route "lockstep" (the same searches in numpy, every row through
gr_ring_rays), the number of trace launches and of rays traced, the time inside the trace launches (the sum of the lock-step calls'
kernel_ms: the same rays in the same launches) and the share of the device call spent outside them, and the host post-processing of
the cache into a DiscCoronaProfile."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (one HIP runtime per process: torch first, as the tests and bench.py have it)

import gradus_jl_amd as G  # noqa: E402
from gradus_jl_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=10)
    ap.add_argument("--slices", type=int, default=100)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--extrema-iter", type=int, default=80)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--spin", type=float, default=0.998)
    a = ap.parse_args()
    K = G.corona
    m, d, model = G.KerrMetric(1.0, a.spin), G.ThinDisc(0.0, 1000.0), G.DiscCorona(G.SourceVelocities.co_rotating, 5.0, 5.0)
    models = [G.RingCorona(model.vf, float(r), model.h) for r in np.linspace(1e-2, model.r, a.rings)]
    βs = K.DEFAULT_β_ANGLES(a.slices)
    base = K.ring_base_angles(a.samples, a.extrema_iter)
    ens = G.EnsembleMI355X(0)
    tracer = K.RingTracer(m, d, models, βs, ensemble=ens)
    device = []
    for _ in range(a.repeat):
        st = _lib.gr_stats()
        t0 = time.perf_counter()
        rows, counts = tracer.arms(base, a.extrema_iter, stats=st)
        device.append({"wall_ms": 1e3 * (time.perf_counter() - t0), "call_ms": st.call_ms, "rays": int(st.rays),
                       "steps_per_ray": st.accepted_steps / max(st.rays, 1)})
    trace_ms, calls = [], []

    def timed(ring, slice_, angles):
        st = _lib.gr_stats()
        out = tracer(ring, slice_, angles, stats=st)
        trace_ms.append(st.kernel_ms)
        calls.append(len(angles))
        return out

    t0 = time.perf_counter()
    rows_ls, counts_ls = K.lockstep_arm_traces(timed, len(models), βs.size, base, a.extrema_iter)
    lockstep_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    try:
        prof = G.disc_corona_profile(m, d, model, βs, n_rings=a.rings, n_samples=a.samples, extrema_iter=a.extrema_iter, ensemble=ens)
        profile = {"rings": len(prof.rings)}
    except ValueError as e:          # (a slice whose arm has fewer than 2 points: reported, the timings above stand)
        profile = {"error": str(e)}
    profile_ms = 1e3 * (time.perf_counter() - t0)
    best = min(device, key=lambda r: r["wall_ms"])
    print(json.dumps({
        "case": {"rings": a.rings, "slices": a.slices, "samples": a.samples, "extrema_iter": a.extrema_iter, "spin": a.spin},
        "device_runs": device,
        "device_wall_ms": best["wall_ms"],
        "lockstep_wall_ms": lockstep_ms,
        "trace_launches": len(calls),
        "rays_traced": int(sum(calls)),
        "rays_per_launch_after_base": calls[1:6] + ["..."] + calls[-3:] if len(calls) > 9 else calls[1:],
        "trace_launch_ms_sum": float(sum(trace_ms)),
        "base_launch_ms": float(trace_ms[0]),
        "share_outside_trace_launches": 1.0 - float(sum(trace_ms)) / best["wall_ms"],
        "same_bits": bool(rows.tobytes() == rows_ls.tobytes() and np.array_equal(counts, counts_ls)),
        "kept_probes": int(counts[..., 1:].sum()),
        "model_to_profile_ms": profile_ms,
        "profile": profile,
    }))


if __name__ == "__main__":
    main()
