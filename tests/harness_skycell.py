"""ctypes front of tests/host_harness_skycell.cpp: the tangent flavour of the device integrator on the host, for the cells
of a source's sky -- seeded (x, v, ∂v/∂θ, ∂v/∂ϕ) -> (t, r, ϕ, g, J, status) rows.  The seed is formed here in numpy from the
closed form the device kernel uses (k_skycell_velocities), so the harness checks Ray::initial_conditions, the integrator
and Ray::finalize; the seeding kernel itself is checked against this on the GPU."""
import ctypes as C

import numpy as np

import hostbuild


def lib():
    L = hostbuild.load("host_harness_skycell.cpp")
    assert L.hhs_row_doubles() == 6 and L.hhs_seed_doubles() == 9
    return L


def seeds(Mx, cosθ, ϕ):
    """v = Mx (1, -k̂) and the seed rows (∂v/∂θ[4], ∂v/∂ϕ[4], sin θ) of the cells: samplers.jl:75-97 and its derivatives"""
    cosθ, ϕ = np.asarray(cosθ, dtype=np.float64), np.asarray(ϕ, dtype=np.float64)
    θ = np.arccos(cosθ)
    st, sp, cp = np.sin(θ), np.sin(ϕ), np.cos(ϕ)
    zero = np.zeros_like(θ)
    k = np.stack([st * cp, st * sp, cosθ], axis=-1)
    kθ = np.stack([cosθ * cp, cosθ * sp, -st], axis=-1)
    kϕ = np.stack([-st * sp, st * cp, zero], axis=-1)
    S = np.asarray(Mx)[:, 1:]
    v = np.asarray(Mx)[:, 0][None, :] - k @ S.T
    seed = np.concatenate([-(kθ @ S.T), -(kϕ @ S.T), st[:, None]], axis=1)
    return np.ascontiguousarray(v), np.ascontiguousarray(seed)


def sky_cells(su, cosθ, ϕ, tangent_norm=1):
    """(n, 6) rows of the host build for the cells (cos θ, ϕ) of the source of `su` (tests/skycell_scene.py: setup)"""
    v, seed = seeds(su["Mx"], cosθ, ϕ)
    x = np.ascontiguousarray(su["x_src"], dtype=np.float64)
    out = np.full((v.shape[0], 6), -777.0)
    rc = lib().hhs_sky_cells(C.byref(su["cfg"]), C.byref(su["pf"]), C.c_void_p(x.ctypes.data), C.c_void_p(v.ctypes.data),
                             C.c_void_p(seed.ctypes.data), C.c_int64(v.shape[0]), C.c_int(tangent_norm), C.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    return out
