"""ctypes binding of tests/host_harness_offsetsolve.cpp: csrc/gr_offsetsolve.hpp (the offset solve and the extremum search as state
machines) driven by the host build of the tangent integrator -- a tracer with `.tangent`, `.solve` and `.search`, as
transfer_functions.device_tracer's, without a GPU."""
import ctypes as C
import math

import numpy as np

import hostbuild


def lib():
    L = hostbuild.load("host_harness_offsetsolve.cpp")
    L.hho_rays_traced.restype = C.c_int64
    return L


def rays_traced():
    """every ray the harness has traced for a `.solve` or a `.search` so far"""
    return int(lib().hho_rays_traced())


def tracer(G, m, x, max_time, plane=None):
    """`(α, β) -> (points, g)` with `.tangent(α, β[, heights])`, `.solve(...)` and `.search(...)` against `plane` (default
    DatumPlane(0)); the configuration is harness.tangent_tracer's."""
    from gradus_jl_amd.rendering import abi_pointfunction
    from gradus_jl_amd.tracing import lnr_momentum_to_global_velocity_matrix
    from gradus_jl_amd.transfer_functions import SEARCH_RECORD, SOLVE_ROW, SUMMARY_DTYPE, unpack_search, unpack_solve

    L, A = lib(), G._lib
    x = np.asarray(x, dtype=np.float64)
    config = G.tracing_configuration(m, x, np.zeros((1, 4)), G.DatumPlane(0.0) if plane is None else plane, max_time,
                                     chart=G.chart_for_metric(m, 2 * x[1], closest_approach=1.005))
    cfg = config.abi_config()
    pf, keep_pf = abi_pointfunction(G.ConstPointFunctions.redshift(m, x))
    Mx = lnr_momentum_to_global_velocity_matrix(m, config.position)

    def rayset():
        rs = A.gr_rayset()
        for i in range(4):
            rs.x_obs[i] = float(config.position[i])
            for k in range(4):
                rs.Mx[4 * i + k] = float(Mx[i, k])
        return rs

    def ptr(a):
        return C.c_void_p(a.ctypes.data)

    def f64(a, n=None):
        a = np.asarray(a, dtype=np.float64)
        return np.ascontiguousarray(a if n is None else np.broadcast_to(a, (n,)))

    def setup_of(r_min, α0=0.0, β0=0.0, zero_atol=1e-7, max_iter=50, contrapoint_bias=2.0, per_wave=0):
        return f64([α0, β0, zero_atol, r_min, contrapoint_bias]), int(max_iter)

    def tangent(α, β, heights=None):
        α, β = f64(α), f64(β)
        rs = rayset()
        rs.alpha, rs.beta, rs.area, rs.n = α.ctypes.data, β.ctypes.data, None, α.size
        if heights is not None:
            h = f64(heights, α.size)
            rs.height = h.ctypes.data
        out = np.zeros((α.size, 8))
        rc = L.hht_ray_tangent(C.byref(cfg), C.byref(rs), C.byref(pf), ptr(out))
        assert rc == 0, rc
        return out

    def trace(α, β):
        out = tangent(α, β)
        pts = np.zeros(out.shape[0], dtype=SUMMARY_DTYPE)
        pts["status"] = out[:, 7].astype(np.int32)
        pts["x"][:, 0], pts["x"][:, 1], pts["x"][:, 2] = out[:, 6], out[:, 1], math.pi / 2
        return pts, out[:, 0].copy()

    def solve(r_target, θ, heights=None, **setup):
        r_target, θ = f64(r_target), f64(θ)
        n = r_target.size
        cθ, sθ = f64(np.cos(θ)), f64(np.sin(θ))
        h = None if heights is None else f64(heights, n)
        s, max_iter = setup_of(**setup)
        out = np.full((n, SOLVE_ROW), np.nan)
        rs = rayset()
        rc = L.hho_solve(C.byref(cfg), C.byref(rs), C.byref(pf), C.c_int64(n), ptr(r_target), ptr(cθ), ptr(sθ),
                         None if h is None else ptr(h), ptr(s), C.c_int32(max_iter), ptr(out))
        assert rc == 0, rc
        return unpack_solve(out)

    def search(r_target, lower, upper, sign, iterations, heights=None, **setup):
        r_target = f64(r_target)
        n = r_target.size
        lower, upper, sign = f64(lower, n), f64(upper, n), f64(sign, n)
        h = None if heights is None else f64(heights, n)
        s, max_iter = setup_of(**setup)
        out = np.full((n, SEARCH_RECORD * (int(iterations) + 1) + 1), np.nan)
        rs = rayset()
        rc = L.hho_search(C.byref(cfg), C.byref(rs), C.byref(pf), C.c_int64(n), ptr(r_target), ptr(lower), ptr(upper), ptr(sign),
                          None if h is None else ptr(h), ptr(s), C.c_int32(max_iter), C.c_int32(int(iterations)), ptr(out))
        assert rc == 0, rc
        return unpack_search(out, int(iterations))

    trace._keep = (keep_pf, config, cfg)
    trace.tangent, trace.solve, trace.search = tangent, solve, search
    return trace
