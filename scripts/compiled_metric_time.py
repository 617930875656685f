"""Time a user's metric three ways on one MI355X: compiled into kernels of its own (metrics.CompiledMetric), through the table
(metrics.TabulatedMetric) and through the metric's fused catalogue kernel.

    python scripts/compiled_metric_time.py [--size 1024] [--reps 10] [--warmup 3] [--cache DIR] [--out FILE.json]
    python scripts/compiled_metric_time.py --build-only [--cache DIR]        (compile the two modules, no device needed)

Rows: Kerr a = 0.998 on C2 (1024², ThinDisc(isco, 50), redshift ∘ filter), Johannsen on C4 (the same plane), and the tangent
launch (gr_ray_tangent_device, one lane per ray) on the rays of the C2 plane against DatumPlane(0).  Every launch is device
resident (gr_render_device / gr_ray_tangent_device into device memory) and timed by a pair of events on its stream; the three
routes of a row alternate rep by rep in one process, after `warmup` untimed launches of each.  The registers and scratch of the
compiled kernels (gr_metric_module_resources) are recorded next to the times."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

JOH = (1.0, 0.7, 2.0, 0.0, 0.0, 1.0)
X_FAR = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
ALIMS, BLIMS = (-60.0, 60.0), (-35.0, 35.0)


def kerr_callable(r, th, p=(1.0, 0.998)):
    """kerr-metric.jl:11-28 as a numpy callable"""
    M, a = p
    R = 2.0 * M
    s2 = np.sin(th) ** 2
    Sig = r ** 2 + a ** 2 * (1.0 - s2)
    gam = s2 * R * r * a
    return (-(1.0 - (R * r) / Sig), Sig / (r ** 2 + a ** 2 - R * r), Sig, s2 * (r ** 2 + a ** 2 + (gam * a) / Sig), -gam / Sig)


def johannsen_callable(r, th, p=JOH):
    """johannsen-ad.jl:12-34 as a numpy callable"""
    M, a, a13, a22, a52, e3 = p
    s2, c2 = np.sin(th) ** 2, np.cos(th) ** 2
    Mr = M / r
    A1, A2, A5 = 1.0 + a13 * Mr ** 3, 1.0 + a22 * Mr ** 2, 1.0 + a52 * Mr ** 2
    Sig = r * r + a * a * c2 + e3 * M ** 3 / r
    Del = r * r - 2.0 * M * r + a * a
    r2a2 = r * r + a * a
    den = (r2a2 * A1 - a * a * A2 * s2) ** 2
    tt = -Sig * (Del - a * a * A2 * A2 * s2) / den
    pp = Sig * s2 * (r2a2 * r2a2 * A1 * A1 - a * a * Del * s2) / den
    tp = -a * (r2a2 * A1 * A2 - Del) * Sig * s2 / den
    return (tt, Sig / (Del * A5), Sig, pp, tp)


def metrics(G, cache):
    kerr, joh = G.KerrMetric(1.0, 0.998), G.JohannsenMetric(*JOH)
    return {"kerr": {"fused": kerr, "compiled": G.CompiledMetric(kerr_callable, inner_radius=kerr.inner_radius(), isco=kerr.isco(), cache_dir=cache)},
            "johannsen": {"fused": joh, "compiled": G.CompiledMetric(johannsen_callable, inner_radius=joh.inner_radius(), isco=joh.isco(), cache_dir=cache)}}


def summary(ms):
    return {"min_ms": float(np.min(ms)), "median_ms": float(np.median(ms)), "max_ms": float(np.max(ms)), "all_ms": [float(t) for t in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--build-only", action="store_true")
    args = ap.parse_args()
    if args.build_only:
        import gradus_jl_amd as G

        for name, ms in metrics(G, args.cache).items():
            print(name, ms["compiled"].compile(), flush=True)
        return
    import torch  # (one HIP runtime per process: torch first, as in tests/conftest.py)

    import gradus_jl_amd as G
    from gradus_jl_amd import _lib
    from gradus_jl_amd import device as gdev
    from gradus_jl_amd.rendering import abi_pointfunction
    from gradus_jl_amd.tracing import lnr_momentum_to_global_velocity_matrix, tracing_configuration

    if not torch.cuda.is_available():
        raise SystemExit("compiled_metric_time.py measures on the GPU and found none")
    dev = torch.device("cuda", 0)
    ens = G.EnsembleMI355X(0)
    L = _lib.load()
    S = args.size
    ms_all = metrics(G, args.cache)
    for name in ms_all:
        ms_all[name]["tabulated"] = G.TabulatedMetric(ms_all[name]["fused"])
    rows = []

    def alternate(launchers):
        """{route: launch()} -> {route: [ms]}: warm-up launches of each, then the routes in turn, rep by rep"""
        for _ in range(args.warmup):
            for fn in launchers.values():
                fn()
        torch.cuda.synchronize()
        out = {k: [] for k in launchers}
        for _ in range(args.reps):
            for k, fn in launchers.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out[k].append(e0.elapsed_time(e1))
        return out

    # ---- fused renders: C2 (Kerr) and C4 (Johannsen) ----
    for name, label in (("kerr", "C2 Kerr a=0.998"), ("johannsen", "C4 Johannsen")):
        base = ms_all[name]["fused"]
        d = G.ThinDisc(base.isco(), 50.0)
        launchers, images = {}, {}
        for route in ("fused", "compiled", "tabulated"):
            m = ms_all[name][route]
            pf = G.ConstPointFunctions.redshift(m, X_FAR, **({"ensemble": ens} if m.metric_id != 0 else {})) @ G.ConstPointFunctions.filter_intersected()
            cfg = G.render_configuration(m, X_FAR, d, 2000.0, image_width=S, image_height=S, alpha_lims=ALIMS, beta_lims=BLIMS, ensemble=ens)
            images[route] = torch.empty(S * S, dtype=torch.float64, device=dev)
            launchers[route] = (lambda cfg=cfg, pf=pf, img=images[route]: gdev.render_device(cfg, pf, img))
        times = alternate(launchers)
        ref = images["fused"].cpu().numpy()
        for route in launchers:
            img = images[route].cpu().numpy()
            both = ~np.isnan(img) & ~np.isnan(ref)
            row = {"row": label, "size": S, "route": route, **summary(times[route]),
                   "flips_vs_fused": int(np.sum(np.isnan(img) != np.isnan(ref))),
                   "rel_q999_vs_fused": float(np.quantile(np.abs(img[both] / ref[both] - 1.0), 0.999))}
            if route == "compiled":
                row["resources"] = ms_all[name]["compiled"].resources
                row["build_id"] = ms_all[name]["compiled"].build_id
            rows.append(row)
            print(json.dumps(row), flush=True)

    # ---- the tangent launch: the rays of the C2 plane, value + ∂/∂α + ∂/∂β, one lane per ray ----
    ens.set("tangent_pairs", 0)
    al = torch.linspace(ALIMS[0], ALIMS[1], S, dtype=torch.float64, device=dev).repeat_interleave(S).contiguous()
    be = torch.linspace(BLIMS[0], BLIMS[1], S, dtype=torch.float64, device=dev).repeat(S).contiguous()
    launchers, outs, keep = {}, {}, []
    for route in ("fused", "compiled", "tabulated"):
        m = ms_all["kerr"][route]
        config = tracing_configuration(m, X_FAR, np.zeros((1, 4)), G.DatumPlane(0.0), 2000.0, chart=G.chart_for_metric(m, 2000.0), ensemble=ens)
        cfg = config.abi_config()
        pf, keep_pf = abi_pointfunction(G.ConstPointFunctions.redshift(m, X_FAR, **({"ensemble": ens} if m.metric_id != 0 else {})))
        Mx = lnr_momentum_to_global_velocity_matrix(m, config.position)
        rs = _lib.gr_rayset()
        for i in range(4):
            rs.x_obs[i] = float(config.position[i])
            for k in range(4):
                rs.Mx[4 * i + k] = float(Mx[i, k])
        rs.alpha, rs.beta, rs.area, rs.n = al.data_ptr(), be.data_ptr(), None, S * S
        outs[route] = torch.empty(S * S * 8, dtype=torch.float64, device=dev)
        keep.append((cfg, pf, keep_pf, rs, config))

        def launch(cfg=cfg, rs=rs, pf=pf, out=outs[route]):
            _lib.check(L.gr_ray_tangent_device(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), C.c_void_p(out.data_ptr()), None,
                                               gdev._stream_handle()))

        launchers[route] = launch
    times = alternate(launchers)
    ref = outs["fused"].cpu().numpy().reshape(-1, 8)
    for route in launchers:
        o = outs[route].cpu().numpy().reshape(-1, 8)
        hit = (o[:, 7] == 2) & (ref[:, 7] == 2)
        row = {"row": "tangent launch, Kerr a=0.998", "size": S, "route": route, **summary(times[route]), "hits": int(hit.sum()),
               "status_flips_vs_fused": int(np.sum(o[:, 7] != ref[:, 7])),
               "rel_q999_radius_vs_fused": float(np.quantile(np.abs(o[hit, 1] / ref[hit, 1] - 1.0), 0.999))}
        if route == "compiled":
            row["resources"] = ms_all["kerr"]["compiled"].resources
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
