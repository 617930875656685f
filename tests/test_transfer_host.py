"""TraceRadiativeTransfer on the CPU: the radiative-transfer flavour of the device integrator (gr_device.hpp under GR_RADTRANS, what
kernels_tu.hip -DGR_TU_RT compiles for the GPU) built for the host (tests/host_harness_transfer.cpp) and held, ray by ray, to

  1. an independent integration (tests/independent/transfer_dop853.py: DOP853 at 1e-12 in Hamiltonian form, exact crossings,
     I integrated piecewise) -- every fixture ray, every medium, both scenes;
  2. statements that hold exactly: no crossing or no medium leaves I0 untouched bit for bit, absorption of nothing is nothing,
     emission never lowers I;
  3. the equilibrium of a medium with sj = sa - 3, pj = pa (dI/dλ = s a_ν (S - I)), and its superposition law off equilibrium;
  4. termination: a ray tangent to the torus ends within maxiters passes through the step loop, by fewer than 64 crossings or flagged;
  5. a run of the same source under AddressSanitizer and UBSan, as a stand-alone program.

Scenes, rays, media and every bound: tests/transfer_scene.py (the measured figures behind the bounds: DESIGN_measurements.md §M40).
Nothing here launches a kernel; tests/test_gpu_transfer.py asks the device the same questions.
"""
import os
import subprocess

import numpy as np
import pytest

import harness
import transfer_scene as S

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = ("A", "B")


@pytest.mark.parametrize("medium", ["emission", "absorption", "both", "equilibrium"])
@pytest.mark.parametrize("scene", SCENES)
def test_host_build_against_the_independent_integration(G, scene, medium):
    md = S.golden()["media"][medium]
    pts, I, iters, ncross = S.host_scene(G, scene, md)
    ref = S.golden_intensity(scene, medium)
    want = np.array([len(r["crossings"]) for r in S.rays(scene)[2]])
    dev = S.deviation(I, ref)
    print(f"scene {scene} {medium}: {I.size} rays ({int((want > 0).sum())} crossing), max deviation {dev.max():.3e} (bound {S.GOLDEN_BOUND:.1e})")
    assert np.array_equal(ncross, want), "the host build and the independent integration count different crossings"
    assert not np.any(pts["flags"] & 0xFFFF)
    assert dev.max() <= S.GOLDEN_BOUND


@pytest.mark.parametrize("scene", SCENES)
def test_a_ray_that_never_crosses_keeps_I0_and_the_plain_traces_status(G, scene):
    md = S.golden()["media"]["both"]
    pts, I, _, ncross = S.host_scene(G, scene, md)
    never = ncross == 0
    assert never.sum() >= 8
    assert np.all(I[never] == md["I0"])
    al, be, _ = S.rays(scene)
    plain = harness.trace_endpoints(G, S.configuration(G, scene, None, al, be))
    # the plain trace ends a crossing ray on the surface; one that never meets it ends where this trace ends it
    assert np.array_equal(pts["status"][never], plain["status"][never])
    assert not np.any(plain["status"][never] == int(G.StatusCodes.IntersectedWithGeometry))
    assert np.all(plain["status"][~never] == int(G.StatusCodes.IntersectedWithGeometry))


@pytest.mark.parametrize("scene", SCENES)
def test_exact_statements(G, scene):
    zero = dict(nu0=1.0, I0=0.7, a0=0.0, j0=0.0, pa=0.0, pj=0.0, sa=0.0, sj=0.0)
    _, I, _, ncross = S.host_scene(G, scene, zero)
    assert (ncross > 0).sum() >= 30
    assert np.all(I == 0.7), "zero coefficients must leave I0 untouched bit for bit"
    # ... and so must the reference's default medium (None)
    al, be, _ = S.rays(scene)
    _, I, _, _ = S.host_endpoints(G, S.configuration(G, scene, G.TraceRadiativeTransfer(), al, be))
    assert np.all(I == 1.0)
    dark = dict(S.golden()["media"]["absorption"], I0=0.0)
    _, I, _, _ = S.host_scene(G, scene, dark)
    assert np.all(I == 0.0), "absorption only with I0 = 0 gives exactly 0"
    em = dict(S.golden()["media"]["emission"], I0=0.25)
    _, I, _, ncross = S.host_scene(G, scene, em)
    assert np.all(I >= 0.25) and np.all(I[ncross > 0] > 0.25) and np.all(I[ncross == 0] == 0.25)


@pytest.mark.parametrize("scene", SCENES)
def test_equilibrium_and_superposition(G, scene):
    eq, ab, Sv = S.superposition_media()
    _, I_at, _, _ = S.host_scene(G, scene, dict(eq, I0=Sv))
    print(f"scene {scene}: I0 = S ends within {np.abs(I_at / Sv - 1).max():.2e} of S")
    assert np.abs(I_at / Sv - 1).max() <= S.EQUILIBRIUM_BOUND
    _, I_eq, _, ncross = S.host_scene(G, scene, eq)
    _, I_ab, _, _ = S.host_scene(G, scene, ab)
    d = np.abs(I_eq - (Sv + (eq["I0"] - Sv) * I_ab / ab["I0"])) / Sv
    print(f"scene {scene}: superposition holds to {d.max():.2e} (bound {S.SUPERPOSITION_BOUND:.1e})")
    assert d.max() <= S.SUPERPOSITION_BOUND
    assert np.abs(I_eq[ncross > 0] - eq["I0"]).min() > 1e-3      # (the medium did something on every crossing ray)


def test_a_grazing_ray_terminates(G):
    lo, hi = S.grazing_beta(G)
    assert 0.0 < hi - lo <= 4 * np.spacing(hi)
    al, be = S.grazing_rays(G)
    maxiters = 2000
    trace = G.TraceRadiativeTransfer(I0=1.0, medium=G.PowerLawMedium(a0=0.3, j0=0.1))
    pts, I, iters, ncross = S.host_endpoints(G, S.configuration(G, "A", trace, al, be, maxiters=maxiters))
    flagged = (pts["flags"] & S.GR_FLAG_MAXITERS) != 0
    print(f"tangent β in [{lo!r}, {hi!r}]: passes {iters.min()}..{iters.max()}, crossings {sorted(set(ncross.tolist()))}, flagged {int(flagged.sum())}")
    # every pass through the step loop but the last counts one attempted step, and the loop's first test ends it at maxiters
    assert np.all(iters <= maxiters + 1)
    assert np.all((ncross < S.MAX_CROSSINGS) | flagged)
    assert np.all(np.isfinite(I))
    assert set(ncross.tolist()) >= {0, 2}      # the fan really straddles the tangent ray
    # ... and the cap itself: with maxiters too small for the ray, the ray ends flagged after exactly that many steps
    pts, _, iters, _ = S.host_endpoints(G, S.configuration(G, "A", trace, al[:4], be[:4], maxiters=50))
    assert np.all((pts["flags"] & S.GR_FLAG_MAXITERS) != 0) and np.all(iters == 51)


def test_fluid_velocity_is_the_references(G):
    """fluid_velocity as circular-orbits.jl has it: outside the ISCO the circular orbit (normalised, v^r = 0); inside, the SAME
    v^t and v^ϕ with v^r = -sqrt|nom / (-g_rr)| -- nom = u.u + 1, zero to rounding where the orbit is timelike, 2 inside the photon
    orbit where it is not (so v^r = -sqrt(2 / g_rr) there: real, and not the interpolated plunge of the redshift)."""
    import ctypes as C

    m = G.KerrMetric(1.0, 0.9)
    cfg = G.tracing_configuration(m, np.array([0.0, 100.0, 1.3, 0.0]), np.zeros((1, 4)), None, 10.0).abi_config()
    isco = m.isco()
    out = (C.c_double * 3)()

    def u(rho):
        S.lib().hhr_fluid_velocity(C.byref(cfg), C.c_double(rho), C.c_double(isco), out)
        return np.array([out[0], out[1], out[2]])

    def norm(rho, v):
        g = m.metric(np.array([0.0, rho, np.pi / 2, 0.0]))
        return g[0, 0] * v[0] ** 2 + 2 * g[0, 3] * v[0] * v[2] + g[3, 3] * v[2] ** 2 + g[1, 1] * v[1] ** 2

    for rho in (isco * 1.0001, 4.0, 10.0, 30.0):
        v = u(rho)
        assert v[1] == 0.0 and v[0] > 0 and abs(norm(rho, v) + 1.0) < 1e-12
        Om = 1.0 / (rho ** 1.5 + 0.9)
        assert v[2] / v[0] == pytest.approx(Om, rel=1e-12)
    v_in, v_out = u(isco * 0.999), u(isco * 1.001)
    assert v_in[1] <= 0.0 and abs(v_in[1]) < 1e-6 and v_in[0] == pytest.approx(v_out[0], rel=1e-2)
    r_ph = 2.0 * (1.0 + np.cos(2.0 / 3.0 * np.arccos(-0.9)))      # Kerr's prograde photon orbit
    v = u(0.98 * r_ph)
    g_rr = m.metric(np.array([0.0, 0.98 * r_ph, np.pi / 2, 0.0]))[1, 1]
    assert v[1] == pytest.approx(-np.sqrt(2.0 / g_rr), rel=1e-9)


def test_sanitizer_run_of_the_harness_source():
    """The same source as a stand-alone program (-DHHR_MAIN: own main, scene A by hand, every medium kind) under AddressSanitizer
    and UBSan, once.  It needs no preloaded runtime: the program is linked against the sanitizers itself."""
    exe = os.path.join(HERE, "host_harness_transfer_asan")
    src = os.path.join(HERE, "host_harness_transfer.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-DHHR_MAIN", "-o", exe, src])
    try:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    finally:
        os.remove(exe)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.stdout.count("rays changed I") == 4
