"""The closed forms of the pass cull (KerrFamily::pass_cull_bounds) against independent numerics, ray by ray, on
the kernel logic compiled for the host (tests/host_harness_culls.cpp): the bracket of the radial turning point against the
quartic's root from numpy, the two Mino-time bounds against quadrature of du / sqrt(U), the phase-rate bounds against dψ/dτ on a
grid, and every decided ray against the full host trace (a decided ray must be a miss).  CPU only.

Tolerances.  The bracket is 2e-6 wide and numpy's root is refined by Newton to a few ulp: the enclosure is asserted as it
stands.  The quadrature (Gauss-Legendre, 96 nodes, smooth integrands after u = u_t - s²) is good to ~1e-13 relative; the time
bounds come out 0.4-0.6 % loose on these scenes (printed) and are asserted with 1e-9 of slack.  The rates are quotients of two polynomials that both vanish at
μ = +-μ+: the grid stops at 0.999 μ+ and the enclosure carries 1e-9 for that cancellation."""
import math

import numpy as np
import pytest

import harness_culls as H
from cull_scenes import SCENES, bench_variant as scene

GL_X, GL_W = np.polynomial.legendre.leggauss(96)


def tile_rays(tiles, H):
    """plane indices of the tiles' rays, (len(tiles), 64), lanes as host_harness_culls.cpp lays them out"""
    tiles = np.asarray(tiles, dtype=np.int64)
    tx, ty = tiles // (H // 8), tiles % (H // 8)
    lane = np.arange(64)
    return ((tx[:, None] << 3) + (lane >> 3)) * H + (ty[:, None] << 3) + (lane & 7)


def _coeffs(b, i, a):
    E, L, Q = b["E"][i], b["L"][i], b["Q"][i]
    w2 = L * L + Q - a * a * E * E
    c1 = 2.0 * (Q + (L - a * E) ** 2)       # M = 1
    return E, Q, w2, c1, a * a * Q


def _turning_point(E, w2, c1, q4, uc):
    """the first root of U(u) = E² - ω² u² + c1 u³ - a²Q u⁴ beyond uc, refined by Newton"""
    roots = np.roots([-q4, c1, -w2, 0.0, E * E]) if q4 != 0.0 else np.roots([c1, -w2, 0.0, E * E])
    real = roots[np.abs(roots.imag) < 1e-9 * np.abs(roots.real)].real
    ut = float(np.min(real[real > uc]))
    for _ in range(3):
        U = E * E - ut * ut * (w2 - c1 * ut + q4 * ut * ut)
        dU = -ut * (2.0 * w2 - 3.0 * c1 * ut + 4.0 * q4 * ut * ut)
        ut -= U / dU
    return ut


def _mino_time(poly_p, ut, u1):
    """∫ du / sqrt(U) from u1 to u_t with U(u) = (u_t - u) P(u): u = u_t - s² leaves 2 ds / sqrt(P(u_t - s²))"""
    smax = math.sqrt(ut - u1)
    s = 0.5 * smax * (GL_X + 1.0)
    return float(np.sum(GL_W * 2.0 / np.sqrt(np.polyval(poly_p, ut - s * s))) * 0.5 * smax)


def _check_scene(G, cfg, pf, a, rays):
    b = H.pass_bounds(cfg, rays.ravel())
    gtol = cfg.abi_config().gtol
    formed = np.flatnonzero(b["Tb_hi"] > 0.0)          # rays whose radial side went through
    polar = np.flatnonzero(b["Om_hi"] > 0.0)           # ... and the polar side
    loose_a, loose_b = [], []
    for i in formed[:: max(1, formed.size // 500)]:
        E, Q, w2, c1, q4 = _coeffs(b, i, a)
        ut = _turning_point(E, w2, c1, q4, b["uc"][i])
        assert b["u_lo"][i] <= ut <= b["u_hi"][i], (i, b["u_lo"][i], ut, b["u_hi"][i])
        assert (b["u_hi"][i] - b["u_lo"][i]) < 2.1e-6 * ut
        # U = (u_t - u) P(u): deflate the quartic by its root
        quot, _ = np.polydiv(np.array([-q4, c1, -w2, 0.0, E * E]), np.array([1.0, -ut]))
        P = -quot
        t0, tc = _mino_time(P, ut, b["u0"][i]), _mino_time(P, ut, b["uc"][i])
        Ta, Tb = t0 - tc, t0 + tc
        assert b["Ta_lo"][i] <= Ta * (1.0 + 1e-9), (i, b["Ta_lo"][i], Ta)
        assert b["Tb_hi"][i] >= Tb * (1.0 - 1e-9), (i, b["Tb_hi"][i], Tb)
        loose_a.append(1.0 - b["Ta_lo"][i] / Ta)
        loose_b.append(b["Tb_hi"][i] / Tb - 1.0)
    for i in polar[:: max(1, polar.size // 500)]:
        E, Q, w2, c1, q4 = _coeffs(b, i, a)
        A = a * a * E * E
        # μ+²: the positive root of a²E² y² + ω² y - Q (Θ as a polynomial in y = μ²); a = 0 leaves ω² y = Q
        mp2 = Q / w2 if A == 0.0 else float(np.max(np.roots([A, w2, -Q]).real))
        mu = math.sqrt(mp2) * np.linspace(-0.999, 0.999, 201)
        theta_pot = Q - w2 * mu ** 2 - A * mu ** 4
        rate = np.sqrt(theta_pot / (mp2 - mu ** 2))
        assert b["Om_lo"][i] * (1.0 - 1e-9) <= rate.min() and rate.max() <= b["Om_hi"][i] * (1.0 + 1e-9), (i, rate.min(), rate.max())
        # the phase: μ0 = μ+ sin ψ0, rising where dμ/dτ >= 0
        assert math.isclose(math.sqrt(mp2) * math.sin(b["psi0"][i]), b["mu0"][i], rel_tol=1e-9, abs_tol=1e-12)
        assert (math.cos(b["psi0"][i]) >= 0.0) == (b["mu_rising"][i] == 1.0)
        assert abs(b["mu0"][i]) > gtol
    decided = b["decided"] == 1.0
    if loose_a:
        print(f"rays {rays.size}, radial side formed {formed.size}, decided {int(decided.sum())}; looseness of T_a^lo "
              f"{np.min(loose_a):.4f}..{np.max(loose_a):.4f}, of T_b^hi {np.min(loose_b):.4f}..{np.max(loose_b):.4f}")
    return b, decided


def _full_trace_hits(G, cfg, pf, tiles):
    off = H.render_tiles(G, cfg, pf, tiles, step=0, start=0, zeta=0.0)
    assert np.all(off["at_start"] == 0)
    return off["status"].ravel() == int(G.StatusCodes.IntersectedWithGeometry)


def test_bench_plane_bounds_enclose_and_decided_rays_miss(G):
    """8 tiles of the 2048² bench plane on the image's diagonal through the annulus the pass cull decides (512 rays)."""
    cfg, pf, a = scene(G, size=2048)
    nt = 2048 // 8
    tiles = np.array([k * nt + k for k in (8, 24, 40, 56, 72, 88, 104, 120)])
    rays = tile_rays(tiles, 2048)
    b, decided = _check_scene(G, cfg, pf, a, rays)
    assert decided.sum() > 0
    hit = _full_trace_hits(G, cfg, pf, tiles)
    assert not np.any(decided & hit)


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_bounds_enclose_and_decided_rays_miss(G, name):
    """Every ray of the scene at 64² for the decision, about 500 of them for the numerics."""
    cfg, pf, a = scene(G, **SCENES[name])
    tiles = np.arange(64)
    rays = tile_rays(tiles, 64)
    b, decided = _check_scene(G, cfg, pf, a, rays)
    assert decided.sum() > 0, name
    assert np.all(b["vr"] < 0.0)
    hit = _full_trace_hits(G, cfg, pf, tiles)
    assert not np.any(decided & hit), name
