"""The sky-cell rows (t, r, ϕ, g, J, status) of the tangent kernels, on their HOST build (tests/host_harness_skycell.cpp):
the (θ, ϕ) seed on a source's sky, dual numbers through the integrator and the event, J = |∂(r, ϕ)/∂(θ, ϕ_sky)| / sin θ.

  flat space   against the closed form (a straight line to the thin disc's wedge) and its complex-step Jacobian;
  Kerr a = 0.998 and a Johannsen metric, RingCorona r = 10, h = 4: t, r, ϕ, g, status against `oracle.trace` of
               `corona.sky_angles_to_velocity` rays, J against Richardson-extrapolated central differences of the oracle.

Scenes, references and bars: tests/skycell_scene.py (shared with tests/test_gpu_skycell.py).  Measured on the host build when
this was written: flat space t 9.0e-10, r 6.0e-10, ϕ 3.3e-10, J 1.4e-7; Kerr t, r 1.6e-7, ϕ 3.5e-8, g 2.1e-9, J 1.4e-6 on 406
of 420 hit cells, no status mismatch; Johannsen t, r 1.2e-8, g 1.5e-9, J 7.8e-6 on 47 of 49."""
import numpy as np
import pytest

import harness_skycell as H
import skycell_scene as S
from skycell_scene import check_against_flat_space, check_against_oracle, reference


def test_seed_is_the_derivative_of_the_velocity(G, oracle):
    """the closed-form seed against central differences of sky_angles_to_velocity (step 1e-6: truncation and rounding < 1e-9)"""
    su = S.setup(G, S.KERR, oracle)
    cosθ, ϕ = S.FLAT.cells(G)
    v, seed = H.seeds(su["Mx"], cosθ, ϕ)
    np.testing.assert_allclose(v, G.sky_angles_to_velocity(su["m"], su["x_src"], su["v_src"], np.arccos(cosθ), ϕ), rtol=1e-13, atol=1e-15)
    h = 1e-6
    θ = np.arccos(cosθ)
    for col, (dθ, dϕ) in ((0, (h, 0.0)), (4, (0.0, h))):
        hi = G.sky_angles_to_velocity(su["m"], su["x_src"], su["v_src"], θ + dθ, ϕ + dϕ)
        lo = G.sky_angles_to_velocity(su["m"], su["x_src"], su["v_src"], θ - dθ, ϕ - dϕ)
        np.testing.assert_allclose(seed[:, col:col + 4], (hi - lo) / (2 * h), rtol=0, atol=1e-9)
    np.testing.assert_allclose(seed[:, 8], np.sin(θ), rtol=1e-15)


def test_flat_space_rows_equal_the_closed_form(G, oracle):
    su = S.setup(G, S.FLAT, oracle)
    cosθ, ϕ = S.FLAT.cells(G)
    assert cosθ.size == 50 and cosθ.min() == 0.2 and abs(cosθ.max() - 0.95) < 1e-15
    rows = H.sky_cells(su, cosθ, ϕ)
    check_against_flat_space(rows, su, cosθ, ϕ, "host")
    np.testing.assert_allclose(rows[:, 3], 1.0, rtol=1e-12)        # a stationary source over a static disc in flat space


@pytest.mark.parametrize("scene", [S.KERR, S.JOHANNSEN], ids=lambda s: s.name)
def test_rows_equal_the_oracle_and_J_its_richardson_differences(G, oracle, scene):
    su, cosθ, ϕ, ref = reference(oracle, G, scene)
    assert cosθ.size == 9 ** scene.level
    rows = H.sky_cells(su, cosθ, ϕ)
    check_against_oracle(rows, ref, scene.name)


def test_values_do_not_depend_on_the_tangents_unless_the_norm_reads_them(G, oracle):
    """with tangent_norm 0 the controller sees values only: the rows' values are those of the same rays without a seed"""
    su, cosθ, ϕ, ref = reference(oracle, G, S.JOHANNSEN)
    a = H.sky_cells(su, cosθ, ϕ, tangent_norm=0)
    b = H.sky_cells(su, cosθ, ϕ, tangent_norm=1)
    assert np.array_equal(a[:, 5], b[:, 5])
    hit = a[:, 5] == 1.0
    np.testing.assert_allclose(a[hit][:, :4], b[hit][:, :4], rtol=1e-6)
    check_against_oracle(a, ref, "values-only norm")
