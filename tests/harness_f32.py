"""ctypes binding of tests/host_harness_f32.cpp: the SINGLE-PRECISION text of the HIP integrator compiled for the host, with
the clang++ that belongs to hipcc and the flags of the library's kernels32_m*.o objects."""
import ctypes as C
import functools
import os

import numpy as np

import hostbuild

# the single-precision flags of __graft_entry__.hip_units / HIP_FLAGS
F32_FLAGS = ["-DGR_REAL_IS_FLOAT", "-Xclang", "-cl-single-precision-constant", "-ffp-contract=on"]
LOG_COLS = ("t", "r", "theta", "h", "dt", "e2", "flags")      # host_harness_f32.cpp: HF_LOG_COLS


@functools.cache
def clangxx():
    """The clang++ of the ROCm installation whose hipcc builds the library (g++ ignores ext_vector_type)."""
    import __graft_entry__ as g

    bindir = os.path.dirname(os.path.realpath(g._hipcc()))
    for cand in (os.path.join(bindir, "amdclang++"), os.path.join(bindir, "..", "lib", "llvm", "bin", "clang++"),
                 os.path.join(bindir, "..", "llvm", "bin", "clang++"), os.path.join(bindir, "clang++")):
        if os.path.exists(cand):
            return cand
    raise RuntimeError("no clang++ next to " + g._hipcc())


def lib():
    L = hostbuild.load("host_harness_f32.cpp", flags=F32_FLAGS, compiler=clangxx())
    L.hf_step_log.restype = C.c_int64
    return L


def render_endpoints(G, config):
    """gr_point records of the plane's rays in ray order (column-major pixels), as tests/harness.py render_endpoints."""
    L = G._lib
    cfg, pl = config.abi_config(), config.abi_plane()
    n = pl.width * pl.height
    rg = L.gr_range(0, n, max(n, 1), 1)
    out = np.zeros(n, dtype=L.POINT_DTYPE)
    rc = lib().hf_render_endpoints(C.byref(cfg), C.byref(pl), C.byref(rg), C.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    return out


def render(G, config, pf):
    from gradus_jl_amd.rendering import abi_pointfunction

    L = G._lib
    cfg, pl = config.abi_config(), config.abi_plane()
    n = pl.width * pl.height
    rg = L.gr_range(0, n, max(n, 1), 1)
    s, keep = abi_pointfunction(pf)
    img = np.zeros(n)
    rc = lib().hf_render(C.byref(cfg), C.byref(pl), C.byref(rg), C.byref(s), C.c_void_p(img.ctypes.data))
    assert rc == 0, rc
    return img.reshape(pl.width, pl.height).T


def step_log(G, config, i, cap=100000):
    """(end point record, log) of ray `i`: one row of LOG_COLS per attempted step, row 0 the state after init."""
    L = G._lib
    cfg, pl = config.abi_config(), config.abi_plane()
    out = np.zeros(1, dtype=L.POINT_DTYPE)
    log = np.zeros((cap, len(LOG_COLS)))
    n = lib().hf_step_log(C.byref(cfg), C.byref(pl), C.c_int64(i), C.c_void_p(out.ctypes.data),
                          C.c_void_p(log.ctypes.data), C.c_int64(cap))
    assert n >= 0, n
    return out[0], log[:n]
