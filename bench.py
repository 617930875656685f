#!/usr/bin/env python3
"""Headline benchmark: null geodesics / second on a 2048 x 2048 Kerr image plane (BASELINE.json).

One "step" = one complete render of the image plane: every rank traces its share of the
2048² = 4 194 304 rays (KerrMetric a = 0.998, observer r = 1000, θ = 75°, ThinDisc(r_isco, 50),
redshift ∘ filter_intersected, Tsit5 abstol = reltol = 1e-9) with the HIP kernels, results stay
in HBM, then ONE RCCL gather assembles the image on rank 0.  Total work is fixed as N grows
("scaling": "strong").  When the image is sharded (N > 1) two renders are kept in flight on two HIP streams,
so the tail of one render's shallow launch overlaps the head of the next; every render is
still traced, gathered and assembled in full inside the timed region.

A plain run sets up, warms up, times the steps and prints one JSON line.  --full adds, on one GPU, the
legs the headline does not need: the blocking host call (`host_call`), the other BASELINE configurations
(`configs`, `configs_brief`) and the CPU baseline (`cpu_baseline`).  --dump-outputs DIR writes the image
of the last timed step (DIR/image_hit.npy, DIR/image_redshift.npy) so that two builds can be compared
output for output.

    python bench.py --gpus 1 --steps 10 --warmup 2 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# the host driver only supports dmabuf IPC: without this RCCL fails with hipIpcGetMemHandle: invalid argument
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch
import torch.distributed as dist

# MI355X peaks (/opt/skills/guides/MI355X_MICROARCH.md chip table): FP32 vector 157.3 TFLOP/s
# => FP64 vector = half rate; HBM3E 8.0 TB/s spec.
PEAK_FP64_VALU_TFLOPS = 78.6
PEAK_HBM_GBS = 8000.0

# Algorithmic flops of the reference formulation, counted by the oracle compiled on a counting
# scalar (oracle/flopcount.cpp, `make -C oracle count`): per attempted Tsit5 step
# and per ray outside the step loop, for the bench workload.  Reported as `roofline.algorithmic_equivalent`,
# never as the hardware fraction.
FLOPS_JSON = os.path.join(ROOT, "oracle", "flopcount.json")
# The FP64 work the kernel actually EXECUTES comes from the committed rocprofv3 PMC passes of THIS build of the
# kernels: profiles/CURRENT names the summary (written by scripts/profile_pmc.sh + summarize_pmc.py), whose
# `source_sha16` must equal the hash of the kernel sources in this tree and whose kernel must be the one launched.
PROFILE_POINTER = os.path.join(ROOT, "profiles", "CURRENT")


def profile_index():
    """{name: relative path} of the committed rocprofv3 summaries of THIS build: profiles/CURRENT is a small JSON index
    ({"head": ..., "C2": ..., "C4": ..., "C5_f64": ..., "C5_f32": ..., "C2_tabulated": ..., "C4_tabulated": ...}); a bare path
    (rounds 1-4) names the head summary only."""
    txt = open(PROFILE_POINTER).read().strip()
    try:
        idx = json.loads(txt)
        return idx if isinstance(idx, dict) else {"head": str(idx)}
    except ValueError:
        return {"head": txt}


def load_summary(name, kernel_substr, rays):
    """(summary, relative path) of the index entry `name` if it belongs to this build (kernel source hash), profiles the
    kernel that is launched and a launch of `rays` rays; else (None, reason)."""
    from gradus_jl_amd._lib import kernel_source_sha16

    try:
        rel = profile_index()[name]
        with open(os.path.join(ROOT, rel)) as f:
            summ = json.load(f)
    except Exception as e:      # noqa: BLE001
        return None, f"no committed profile summary for {name} ({type(e).__name__}: {e})"
    sha = kernel_source_sha16()
    if summ.get("source_sha16") != sha:
        return None, f"{rel} was taken from kernel sources {summ.get('source_sha16')}, this tree is {sha}: re-profile"
    if kernel_substr not in (summ.get("kernel") or ""):
        return None, f"{rel} profiles {summ.get('kernel')}, not {kernel_substr}"
    if summ.get("rays_per_launch") != rays:
        return None, f"{rel} is a {summ.get('rays_per_launch')}-ray launch; this run launches {rays}"
    for k in ("valu_issue_per_4clk", "avg_ms"):
        if k not in summ:
            return None, f"{rel} lacks {k}"
    return summ, rel


def profile_evidence(size, world):
    """(summary dict, relative path) of the committed profile that belongs to this build and workload, or
    (None, reason)."""
    if world != 1:
        return None, f"the committed head profile is a one-GPU launch; this run launches {size * size // world} rays per GPU"
    summ, rel = load_summary("head", "k_trace_lane<gr::KerrFamily<false>, 1>", size * size)
    if summ is not None and "executed_fp64_flops_per_launch" not in summ:
        return None, f"{rel} lacks executed_fp64_flops_per_launch"
    return summ, rel


PEAK_FP32_VALU_TFLOPS = 157.3


def baseline_configs(G, ens, reps=3):
    """The other BASELINE.json configurations, each as a few launches of its own kernel next to the headline:
    launch duration measured HERE (gr_stats.kernel_ms of the blocking call: start of the call's device work -> end of its trace
    kernel, fastest of `reps` after one warm-up), fraction of the vector-ALU peak from the executed flops of the committed,
    source-hash-checked rocprofv3 summary of that kernel.  ~1.5 s of GPU time in all.
        C2            KerrMetric(a = 0.998) 1024², ThinDisc(isco, 50), redshift                       fp64 fused kernel
        C4            JohannsenMetric(a = 0.7, α13 = 2, ϵ3 = 1) 1024², ThinDisc, interpolated redshift   fp64 fused kernel
        C5_f64 / f32  line profile, 4096² polar-plane rays, tol 1e-9 (fp64) / 1e-5 (fp32 kernels)
        C2_tabulated / C4_tabulated   the same two metrics as USER-DEFINED metrics: through GR_METRIC_TABULATED's table
        corona_1e6    the per-ray half of emissivity_profile at 10⁶ sky samples on the device (not a BASELINE configuration)
    """
    out = {}
    ALIMS, BLIMS = (-60.0, 60.0), (-35.0, 35.0)

    def price(name, kernel_substr, rays, ms, f32=False):
        rec = {"ms": ms, "rays": rays, "rays_per_s": rays / (ms * 1e-3)}
        summ, rel = load_summary(name, kernel_substr, rays)
        key = "executed_fp32_flops_per_launch" if f32 else "executed_fp64_flops_per_launch"
        peak = PEAK_FP32_VALU_TFLOPS if f32 else PEAK_FP64_VALU_TFLOPS
        if summ is not None and key in summ:
            tf = summ[key] / (ms * 1e-3) / 1e12
            rec["roofline"] = {"bound": "fp32-valu" if f32 else "fp64-valu", "achieved": tf, "peak": peak, "unit": "TFLOP/s",
                               "frac": tf / peak, "valu_issue_per_4clk": summ["valu_issue_per_4clk"],
                               "valu_lane_utilization": summ.get("valu_lane_utilization"), "profile": rel,
                               "profile_avg_ms": summ["avg_ms"], "profile_source_sha16": summ["source_sha16"]}
        else:
            rec["roofline"] = {"frac": None, "profile_error": rel if summ is None else f"{rel} lacks {key}"}
        out[name] = rec

    def render_ms(m, x, S):
        pf = G.ConstPointFunctions.redshift(m, x, ensemble=ens) @ G.ConstPointFunctions.filter_intersected()
        disc = G.ThinDisc(m.isco(), 50.0)
        ms = []
        for rep in range(reps + 1):
            _, _, img, st = G.rendergeodesics(m, x, disc, 2000.0, image_width=S, image_height=S, alpha_lims=ALIMS, beta_lims=BLIMS,
                                              pf=pf, ensemble=ens, stats=True)
            if rep:
                ms.append(st["kernel_ms"])
        return min(ms)

    kerr, joh = G.KerrMetric(1.0, 0.998), G.JohannsenMetric(1.0, 0.7, 2.0, 0.0, 0.0, 1.0)
    x75, x70 = np.array([0.0, 1000.0, math.radians(75.0), 0.0]), np.array([0.0, 1000.0, math.radians(70.0), 0.0])
    price("C2", "k_trace_lane<gr::KerrFamily<false>, 1>", 1024 * 1024, render_ms(kerr, x75, 1024))
    price("C4", "k_trace_lane<gr::JohannsenMetric", 1024 * 1024, render_ms(joh, x70, 1024))
    # C5: the line profile on 4096² rays (scripts/sibling_workloads.py c5 / c5f32)
    u = np.array([0.0, 1000.0, math.radians(60), 0.0])
    plane = G.PolarPlane(G.GeometricGrid(), Nr=4096, Nθ=4096, r_min=1.0, r_max=250.0)
    bins = np.linspace(0.1, 1.5, 180)
    for name, prec, tol, sub in (("C5_f64", 64, 1e-9, "k_trace_"), ("C5_f32", 32, 1e-5, "gr32::")):
        ens.set("precision", prec)
        try:
            ms = []
            for rep in range(reps + 1):
                _, _, st = G.lineprofile(bins, G.PowerLawEmissivity(3), kerr, u, G.ThinDisc(kerr.isco(), 250.0), G.BinningMethod(), plane=plane,
                                         maxrₑ=250.0, ensemble=ens, stats=True, abstol=tol, reltol=tol)
                if rep:
                    ms.append(st["kernel_ms"])
        finally:
            ens.set("precision", 64)
        price(name, sub, 4096 * 4096, min(ms), f32=(prec == 32))
    # the same two metrics given to the library as SAMPLES of metric_components: the AbstractMetric plugin path
    for name, base, x in (("C2_tabulated", kerr, x75), ("C4_tabulated", joh, x70)):
        tm = G.TabulatedMetric(base)
        price(name, "k_trace_lane<gr::TabulatedMetric", 1024 * 1024, render_ms(tm, x, 1024))
        out[name]["table"] = {"grid_m_r_n_theta": [tm.m_r, tm.n_theta], "mb": tm.table.nbytes / 1e6, "fit_error_estimates": list(tm.errors)}
        ref = name.split("_")[0]
        out[name]["slowdown_vs_fused"] = out[name]["ms"] / out[ref]["ms"]
    # corona -> disc on the device (<= 10 ms at 10⁶ samples): emissivity_profile(m, d, LampPostModel(h = 10);
    # n_samples = 10⁶, golden-spiral EvenSampler on both hemispheres, N = 100) -- sky rays formed, traced, reduced, binned on the GPU
    sampler = G.EvenSampler(G.BothHemispheres(), G.GoldenSpiralGenerator())
    disc, lamp, n_sky = G.ThinDisc(0.0, 500.0), G.LampPostModel(h=10.0), 1_000_000
    G.corona.device_radial_profile(kerr, disc, lamp, sampler=sampler, n_samples=10_000, N=100, ensemble=ens)      # plunging table, contexts
    best = None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        prof, st = G.corona.device_radial_profile(kerr, disc, lamp, sampler=sampler, n_samples=n_sky, N=100, ensemble=ens, stats=True)
        wall = (time.perf_counter() - t0) * 1e3
        if rep and (best is None or st.call_ms < best[1]):
            best = (st.kernel_ms, st.call_ms, wall, (st.accepted_steps + st.rejected_steps) / n_sky)
    price("corona_1e6", "k_trace_lane<gr::KerrFamily<false>, 1>", n_sky, best[0])      # (sky rays dealt by direction: the one-ray-per-lane kernel)
    out["corona_1e6"].update({"device_call_ms": best[1], "python_wall_ms_incl_binning_and_host_tail": best[2], "steps_per_ray": best[3],
                              "finite_bins": int(np.isfinite(prof.ε).sum()),
                              "what": "emissivity_profile(KerrMetric(a = 0.998), ThinDisc(0, 500), LampPostModel(h = 10); n_samples = 10^6, N = 100): "
                                      "ms = trace kernel, device_call_ms = staging + trace + min/max reduction + copy back"})
    return out


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048, help="image is size x size")
    ap.add_argument("--kernel", type=int, default=2, help="0 = one ray per lane, 1 = persistent, 2 = auto by launch depth")
    ap.add_argument("--lpt-lane", type=int, default=None)
    ap.add_argument("--refill-threshold", type=int, default=None)
    ap.add_argument("--waves-per-simd", type=int, default=None)
    ap.add_argument("--block", type=int, default=None, help="workgroup size (64..256, diagnostic)")
    ap.add_argument("--block-cols", type=int, default=8)
    ap.add_argument("--tile-rows", type=int, default=None, help="pixel tile of a wave: 8 (8 x 8) or 16 (16 x 4: whole 128-B lines per store)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-configs", action="store_true",
                    help="skip the third leg (the other BASELINE configurations, a few launches each: `configs` of the line)")
    ap.add_argument("--no-host-call", action="store_true",
                    help="skip the second timed leg (blocking gr_render into a host buffer, D2H included)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--streams", type=int, default=0,
                    help="renders in flight: 2 = consecutive renders alternate between two HIP streams, so the next render's "
                         "waves fill the SIMDs that the draining one leaves idle (worth 13 %% on a 1/8 shard, 1.5 %% on the "
                         "whole image); 0 = auto: 1 on one GPU (per-launch durations stay comparable with rocprofv3), 2 "
                         "when the image is sharded")
    ap.add_argument("--emulate-shard", type=str, default=None,
                    help="WORLD:RANK -- time one rank's shard of the image on a single GPU (diagnostic, no gather)")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs the headline does not need (N = 1): the blocking host call, the other BASELINE "
                         "configurations and the CPU baseline (each still switched off by its --no-* option)")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="write the image of the last timed step to DIR/image_hit.npy (float32) and DIR/image_redshift.npy "
                         "(float64), both finite; a fixed sample of them above 64 MB")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.emulate_shard:
        ap.error("--dump-outputs writes the assembled image: not with --emulate-shard")
    return args


DUMP_CAP_BYTES = 64_000_000      # every file of one dump together, .npy headers included


def dump_outputs(outdir, image):
    """What the timed path hands its caller: the (H, W) redshift image of the last timed step, NaN where no ray hit.  Written
    as two finite arrays that together hold every pixel: image_hit.npy (float32, 1 = the ray hit the disc, 0 = NaN in the
    image) and image_redshift.npy (float64, 0 where no ray hit).  Above DUMP_CAP_BYTES a fixed, seeded sample of the
    flattened image is written instead, with its flat indices (image_sample_index.npy)."""
    os.makedirs(outdir, exist_ok=True)
    img = np.asarray(image, dtype=np.float64)
    hit = np.isfinite(img)
    out = {"image_hit": hit.astype(np.float32), "image_redshift": np.where(hit, img, 0.0)}
    if img.size * 12 + 8192 > DUMP_CAP_BYTES:
        k = (DUMP_CAP_BYTES - 8192) // 20           # per sample: 8 B value, 4 B hit, 8 B index
        idx = np.sort(np.random.default_rng(0).choice(img.size, size=k, replace=False))
        out = {name: a.reshape(-1)[idx] for name, a in out.items()}
        out["image_sample_index"] = idx.astype(np.float64)
    for name, a in out.items():
        np.save(os.path.join(outdir, name + ".npy"), np.ascontiguousarray(a))


def workload(G, size, ens):
    m = G.KerrMetric(M=1.0, a=0.998)
    x = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
    d = G.ThinDisc(m.isco(), 50.0)
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    cfg = G.render_configuration(m, x, d, 2000.0, image_width=size, image_height=size, alpha_lims=(-60.0, 60.0),
                                 beta_lims=(-35.0, 35.0), ensemble=ens)
    return m, x, d, pf, cfg


def cpu_baseline(size, seconds):
    """The oracle (OpenMP port of the reference algorithm -- NOT the Julia package) timed on this
    host's cores on a strided sub-grid of the same image plane."""
    from oracle import oracle as O

    isco = 1.2369706551751847
    cfg = O.make_config("kerr", (1.0, 0.998), disc=(isco, 50.0), lambda_max=2000.0)
    x = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
    threads = O.lib().orc_max_threads()

    def run(S):
        # S x S pixels spread evenly over the same α/β window => same mix of ray lengths
        v = O.render_velocities(cfg, x, (-60.0, 60.0), (-35.0, 35.0), S, S)
        t0 = time.perf_counter()
        pts = O.trace(cfg, x, v)
        img = O.apply_pf(cfg, pts, 2000.0, pf_id=O.PF_REDSHIFT, filter_id=O.FILTER_INTERSECTED, r_isco=isco)
        return S * S / (time.perf_counter() - t0), img

    rate, _ = run(48)
    S = int(min(1024, max(48, math.sqrt(rate * seconds))))
    rate, _ = run(S)
    import shutil

    return {
        "value": rate, "unit": "geodesics/s", "cores": threads, "kind": "port",
        "julia_on_host": shutil.which("julia") is not None,     # the reference itself could only be timed if it were
        "sample": f"{S}x{S} pixels spanning the same image plane, C oracle with OpenMP on {threads} threads "
                  f"(restatement of the reference algorithm; Julia is not available on this box)",
    }


def flop_model():
    if os.path.exists(FLOPS_JSON):
        with open(FLOPS_JSON) as f:
            return json.load(f)
    return None


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N > 1")
        args.gpus = world
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    launched = "RANK" in os.environ and "MASTER_PORT" in os.environ     # under torch.distributed.run
    if world > 1 or launched:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    import gradus_jl_amd as G
    from gradus_jl_amd import device as gdev

    ens = G.EnsembleMI355X(local_rank, kernel=args.kernel)
    if args.refill_threshold is not None:
        ens.set("refill_threshold", args.refill_threshold)
    if args.waves_per_simd is not None:
        ens.set("waves_per_simd", args.waves_per_simd)
    if args.block is not None:
        ens.set("block", args.block)
    if args.lpt_lane is not None:
        ens.set("lpt_lane", args.lpt_lane)
    if args.tile_rows is not None:
        ens.set("tile_rows", args.tile_rows)
    m, x, d, pf, cfg = workload(G, args.size, ens)
    plan = G.shard_plan(args.size, args.size, world, rank, args.block_cols)
    if args.emulate_shard:
        ew, er = (int(t) for t in args.emulate_shard.split(":"))
        plan = G.shard_plan(args.size, args.size, ew, er, args.block_cols)
    rg = plan.ray_range()
    # Double-buffered slabs: the gather of render i (RCCL, its own stream) overlaps the kernel of
    # render i+1; a slab is only traced into again after its previous gather has completed.
    locals_ = [torch.empty(plan.count, dtype=torch.float64, device=dev) for _ in range(2)]
    forced = os.environ.get("GRADUS_FORCE_COLLECTIVE") == "1"      # one rank through RCCL as well (diagnostic)
    recv = [G.gather_buffers(plan, locals_[0]) if (rank == 0 and (world > 1 or forced)) else None for _ in range(2)]
    pending = [None, None]
    stats = gdev.new_stats(dev)
    last_image = [None]

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]

    if args.streams == 0:
        args.streams = 2 if (world > 1 or args.emulate_shard) else 1
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)] if args.streams > 1 else None

    def step(i=None, slot=0):
        if streams is not None:
            with torch.cuda.stream(streams[slot]):
                _step(i, slot)
        else:
            _step(i, slot)

    def _step(i, slot):
        if pending[slot] is not None:
            img = pending[slot].result()          # previous use of this slab: wait + assemble on rank 0
            if img is not None:
                last_image[0] = img
            pending[slot] = None
        if i is not None:
            ev[i][0].record()
        gdev.render_device(cfg, pf, locals_[slot], rg, stats if i is not None else None)
        if i is not None:
            ev[i][1].record()
        if args.emulate_shard:
            return
        pending[slot] = G.gather_image_async(locals_[slot], plan, recv_bufs=recv[slot])

    def drain(first=0):
        # the older render first: last_image ends as the image of the latest one
        for slot in (first, 1 - first):
            if pending[slot] is not None:
                img = pending[slot].result()
                if img is not None:
                    last_image[0] = img
                pending[slot] = None

    def fence():
        torch.cuda.synchronize()
        if dist.is_initialized():
            dist.barrier()
            torch.cuda.synchronize()

    for w in range(args.warmup):
        step(None, w % 2)
    drain()
    fence()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i, i % 2)
    drain(args.steps % 2)     # every render of the timed region is gathered and assembled inside it
    fence()
    elapsed = time.perf_counter() - t0
    image = last_image[0]
    if dist.is_initialized():
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    image_host = image.cpu().numpy() if image is not None else None
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, image_host)

    # ---- second leg (N = 1): the blocking host entry point, image copied D2H into a host buffer every step
    #      ("wall time of the blocking ABI call, H2D/D2H included, ctx creation excluded") ----
    host_call = None
    if args.full and world == 1 and not args.no_host_call and not args.emulate_shard:
        import ctypes as C

        from gradus_jl_amd import _lib
        from gradus_jl_amd.rendering import abi_pointfunction

        acfg, apl = cfg.abi_config(), cfg.abi_plane()
        apf, keep_pf = abi_pointfunction(pf)
        n_all = args.size * args.size
        arg_rg = _lib.gr_range(0, n_all, n_all, 1)
        host_img = np.empty(n_all, dtype=np.float64)        # a plain (pageable) array, like Julia's `zeros(T, (H, W))`
        hst = _lib.gr_stats()
        L = _lib.load()

        def host_step():
            _lib.check(L.gr_render(ens.ctx.handle, C.byref(acfg), C.byref(apl), C.byref(apf), C.byref(arg_rg),
                                   host_img.ctypes.data, C.byref(hst)))

        for _ in range(max(args.warmup, 1)):
            host_step()
        torch.cuda.synchronize()
        th0 = time.perf_counter()
        for _ in range(args.steps):
            host_step()
        th = time.perf_counter() - th0
        host_call = {"value": n_all * args.steps / th, "unit": "geodesics/s", "ms_per_step": th / args.steps * 1e3,
                     "steps": args.steps, "entry": "gr_render (blocking; kernel + 32 MiB D2H into a pageable host array)",
                     "definition": "SURVEY §8(d): rays completed / wall time of the blocking ABI call, H2D/D2H included, "
                                   "ctx creation excluded",
                     "kernel_ms_last": hst.kernel_ms, "kernel_plus_copy_ms_last": hst.call_ms}
        # the same call into an image the library pinned (gr_host_alloc): the kernel stores across the link itself
        blk = _lib.PinnedBlock(ens.ctx, 8 * n_all)
        pin_img = blk.array(np.float64, n_all)

        def pinned_step():
            _lib.check(L.gr_render(ens.ctx.handle, C.byref(acfg), C.byref(apl), C.byref(apf), C.byref(arg_rg),
                                   pin_img.ctypes.data, C.byref(hst)))

        pinned_step()
        assert pin_img.tobytes() == host_img.tobytes()
        psteps = max(args.steps // 5, 1)
        tp0 = time.perf_counter()
        for _ in range(psteps):
            pinned_step()
        tp = time.perf_counter() - tp0
        host_call["into_pinned_image"] = {"value": n_all * psteps / tp, "ms_per_step": tp / psteps * 1e3, "steps": psteps,
                                          "entry": "gr_render into a gr_host_alloc block: no staging image, no copy",
                                          "kernel_ms_last": hst.kernel_ms, "call_ms_last": hst.call_ms}
        del pin_img, blk

    launch_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))      # start -> end of one launch on its own stream
    # with two renders in flight consecutive launches overlap pairwise: the duration that prices a launch is then
    # the busy span of the device divided by the launches
    kernel_ms = launch_ms if streams is None else float(ev[0][0].elapsed_time(ev[-1][1])) / args.steps
    st = gdev.stats_dict(stats)
    total_rays = args.size * args.size
    rays_per_s = total_rays * args.steps / elapsed

    if args.emulate_shard:
        print(json.dumps({"emulated_shard": args.emulate_shard, "rays": plan.count, "ms_per_step": elapsed / args.steps * 1e3,
                          "kernel_ms": kernel_ms, "launch_ms": launch_ms, "renders_in_flight": args.streams, "rays_per_s_this_rank": plan.count * args.steps / elapsed}))
        return
    if rank == 0:
        # sanity: the image is a real render (hits exist, values finite and O(1))
        img = image_host
        hits = np.isfinite(img)
        assert hits.sum() > 0.05 * total_rays and 0.0 < np.nanmin(img) and np.nanmax(img) < 2.0

        rays_launch = st["rays"] / args.steps
        steps_launch = (st["accepted_steps"] + st["rejected_steps"]) / args.steps
        bytes_launch = rays_launch * 8.0   # fused render: 8 B written per ray, 0 B read
        achieved_gbs = bytes_launch / (kernel_ms * 1e-3) / 1e9
        # ---- hardware fraction: FP64 flops the kernel EXECUTED (rocprofv3 counters of this very build, per ray)
        #      x the rays this run launched / the launch duration measured live with HIP events ----
        summ, src = profile_evidence(args.size, world)
        if summ is not None:
            ex_per_ray = summ["executed_fp64_flops_per_launch"] / summ["rays_per_launch"]
            ex_tflops = rays_launch * ex_per_ray / (kernel_ms * 1e-3) / 1e12
            traffic = summ.get("hbm_read_bytes_per_launch", 0.0) + summ.get("hbm_write_bytes_per_launch", 0.0)
            executed = {"achieved": ex_tflops, "frac": ex_tflops / PEAK_FP64_VALU_TFLOPS, "flops_per_ray_executed": ex_per_ray,
                        "valu_issue_per_4clk": summ["valu_issue_per_4clk"], "fp64_pipe_busy_nominal": summ.get("fp64_pipe_busy_nominal"),
                        "clock_ghz_during_profile": summ.get("clock_ghz"), "valu_insts_per_wave": summ.get("valu_insts_per_wave"),
                        "profile": src, "profile_kernel": summ["kernel"], "profile_source_sha16": summ["source_sha16"],
                        "profile_avg_ms": summ["avg_ms"], "profile_timed_calls": summ.get("timed_calls"),
                        "traffic": traffic or None}
            # the FP64 pipe's own currency: FP64 wave-instructions issued per second against the bare pure-FMA stream of the
            # calibration (the resource that saturates here; a flop-based fraction falls when executed flops are REMOVED)
            cnt = summ.get("counters", {})
            n64 = sum(cnt.get(k, 0.0) for k in ("SQ_INSTS_VALU_FMA_F64", "SQ_INSTS_VALU_MUL_F64", "SQ_INSTS_VALU_ADD_F64",
                                                "SQ_INSTS_VALU_TRANS_F64"))
            if n64:
                per_ray64 = n64 / summ["rays_per_launch"]
                executed["fp64_wave_insts_per_s"] = rays_launch * per_ray64 / (kernel_ms * 1e-3)
        else:
            sys.stderr.write(f"bench.py: roofline.frac withheld: {src}\n")
            executed = {"achieved": None, "frac": None, "traffic": None, "profile": None, "profile_error": src}
        fm = flop_model()
        alg = None
        if fm:
            flops_launch = rays_launch * fm["flops_per_ray_fixed"] + steps_launch * fm["flops_per_step"]
            alg_tflops = flops_launch / (kernel_ms * 1e-3) / 1e12
            alg = {"flops_per_ray": flops_launch / rays_launch, "achieved": alg_tflops, "unit": "TFLOP/s-equivalent",
                   "ratio_to_peak": alg_tflops / PEAK_FP64_VALU_TFLOPS,
                   "note": "the launch priced at the flops of the REFERENCE formulation (oracle compiled on a counting "
                           "scalar, oracle/flopcount.json): a throughput-equivalent figure, not a hardware fraction -- "
                           "the kernel reaches the same results with about half of these flops"}
        # what the part SUSTAINS on a pure stream of independent v_fma_f64 (3 waves per SIMD, 25 ms launches, counters in a
        # separate pass: scripts/microbench/valu_calib.hip -> profiles/r3_valu_calib.json): the nominal 78.6 TFLOP/s assumes one
        # FP64 wave-instruction per 4 clocks at 2.4 GHz; the stream runs at 4.6-5.2 clocks per instruction and ~2.1 GHz
        sustained = None
        try:
            with open(os.path.join(ROOT, "profiles", "r3_valu_calib.json")) as f:
                cal = json.load(f)["calib_fma_f64"]
            sustained = {"tflops": cal["bare_wave_inst_per_s"] * 128.0 / 1e12, "bare_wave_insts_per_s": cal["bare_wave_inst_per_s"],
                         "clock_ghz_under_counters": cal["clock_ghz"],
                         "simd_cycles_per_inst_under_counters": cal["simd_cycles_per_valu_inst"],
                         "source": "profiles/r3_valu_calib.json (calib_fma_f64)"}
        except Exception:      # noqa: BLE001
            pass
        line = {
            "metric": "geodesics/sec, 2048^2 Kerr image plane (fp64 null geodesics, redshift image)",
            "value": rays_per_s,
            "unit": "geodesics/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "value_definition": "rays traced / wall time of the timed region with everything resident in HBM (N > 1: gathered "
                                "onto rank 0 over RCCL inside the region) -- the definition this build's measurement contract "
                                "fixes for `value` (a PCIe-inclusive rate is never `value`).  SURVEY §8(d) defines the metric as "
                                "the wall time of the blocking ABI call with the D2H copy: that rate, measured in this same run, "
                                "is `value_host_call` (details under `host_call`); VERDICT r2 item 5 asked for the two to be "
                                "told apart explicitly -- both are reported, neither is derived from the other",
            "value_host_call": (host_call or {}).get("value"),
            "config": {
                "workload": f"KerrMetric(a=0.998) {args.size}x{args.size} image plane, r_obs=1000, theta=75deg, "
                            "ThinDisc(r_isco,50), redshift∘filter_intersected, Tsit5 tol 1e-9, lambda_max=2000",
                "sharding": f"{world} rank(s), block-cyclic by {plan.block_cols} columns, one RCCL gather per render "
                            "(overlapped with the next render's kernel, double-buffered slabs)",
                "kernel": {0: "one-ray-per-lane", 1: "persistent+wave-ballot-refill",
                           2: "auto: one ray per lane, 8x8 pixel tiles, one-wave workgroups (image planes)"}[args.kernel],
                "renders_in_flight": args.streams,
                "rays_per_gpu": plan.count,
                "steps_per_ray": steps_launch / rays_launch,
                "rejected_steps_per_ray": st["rejected_steps"] / max(st["rays"], 1),
                "status_count_rank0": st["status_count"],
                "rccl_ranks": (dist.get_world_size() if dist.is_initialized() else 1),
            },
            "roofline": {
                "bound": "fp64-valu",
                "note": "neither HBM nor MFMA binds this path (SURVEY §8d): the ODE state lives in registers; peak = FP64 "
                        "vector ALU.  achieved = FP64 flops the kernel EXECUTED per ray (rocprofv3 SQ_INSTS_VALU_{FMA,MUL,"
                        "ADD,TRANS}_F64 x 64 lanes x active-lane fraction, from the committed summary of this build) x "
                        "rays per launch / launch duration measured here with HIP events.",
                "achieved": executed["achieved"],
                "peak": PEAK_FP64_VALU_TFLOPS,
                "unit": "TFLOP/s",
                "frac": executed["frac"],
                "sustained_fma_stream": sustained,
                "fp64_issue": ({"achieved": executed.get("fp64_wave_insts_per_s"), "sustained_pure_fma_stream": sustained.get("bare_wave_insts_per_s"),
                                "frac": executed["fp64_wave_insts_per_s"] / sustained["bare_wave_insts_per_s"],
                                "unit": "FP64 wave-instructions/s",
                                "note": "how busy the FP64 pipe is in its own currency: instructions, not flops (49 % of the kernel's FP64 "
                                        "instructions are multiplies / adds / reciprocals worth one flop)"}
                               if (sustained and sustained.get("bare_wave_insts_per_s") and executed.get("fp64_wave_insts_per_s")) else None),
                "frac_of_sustained_fma_stream": (executed["achieved"] / sustained["tflops"]) if (sustained and executed["achieved"]) else None,
                "kernel_ms": kernel_ms,
                "launch_ms": launch_ms,
                "traffic": executed["traffic"],
                "traffic_note": "HBM bytes per launch (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE, separate --pmc passes); "
                                "algorithmic: 8 B x rays",
                "algorithmic_bytes": bytes_launch,
                "executed": executed,
                "algorithmic_equivalent": alg,
                "hbm": {"achieved": achieved_gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                        "frac": achieved_gbs / PEAK_HBM_GBS, "bytes_per_ray": 8},
            },
        }
        if host_call is not None:
            line["host_call"] = host_call
            line["value_blocking_call_with_d2h"] = host_call["value"]      # SURVEY §8(d)'s definition, named as such
        line["value_device_resident"] = rays_per_s                         # == value (the contract's definition), named as such
        if args.full and world == 1 and not args.no_configs:
            try:
                line["configs"] = baseline_configs(G, ens)
            except Exception as e:      # noqa: BLE001 -- a sibling failing must not lose the measured headline
                line["configs"] = {"error": f"{type(e).__name__}: {e}"}
        if args.full and world == 1 and not args.no_cpu_baseline:
            try:
                line["cpu_baseline"] = cpu_baseline(args.size, args.cpu_seconds)
            except Exception as e:      # noqa: BLE001 -- the checker failing must not lose the measured line
                line["cpu_baseline"] = {"value": None, "unit": "geodesics/s", "cores": 0, "kind": "port",
                                        "sample": f"oracle unavailable: {type(e).__name__}: {e}"}
        if isinstance(line.get("configs"), dict) and "error" not in line["configs"]:
            # the LAST key of the line, ~300 characters: the driver keeps the tail of stdout, and `configs` above is longer than that
            # tail -- {name: [ms per launch, fraction of the vector-ALU peak]} of every BASELINE configuration
            line["configs_brief"] = {k: [round(v["ms"], 3), None if v["roofline"].get("frac") is None else round(v["roofline"]["frac"], 4)]
                                     for k, v in line["configs"].items()}
        print(json.dumps(line))
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
