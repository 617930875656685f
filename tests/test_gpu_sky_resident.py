"""`AdaptiveSky(m, corona, d, resident=True)` on the MI355X: the tree and the rows stay on the device (gr_sky_*), the pair
search, the refinement and the census of the (r, ϕ) bins are kernels, and a step's new cells go to one gr_sky_cells_device
launch.  Everything is pinned to the host route (gradus.jl_amd/adaptive.py over grids.py and gr_sky_cells) on the same
ensemble, bit for bit.  The scene of tests/test_gpu_adaptive_sky.py: RingCorona r = 10, h = 4 over a Kerr hole with a = 0.998
and ThinDisc(0, ∞); one tangent-kernel shape per test, as there (the two shapes agree to 1e-11, not bit for bit)."""
import copy
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("pos", "level", "children", "neighbours", "parent", "location")


def scene(G):
    return G.KerrMetric(1.0, 0.998), G.RingCorona(r=10.0, h=4.0), G.ThinDisc(0.0, math.inf)


def new_sky(G, ens, resident, steps=2):
    sky = G.AdaptiveSky(*scene(G), ensemble=ens, resident=resident)
    if steps is not None:
        G.trace_initial(sky)
        for _ in range(steps):
            G.trace_step(sky)
    return sky


def launches(sky, since=0):
    return [n for n, _ in sky.tracer["launches"][since:]]


def state(sky):
    g = sky.grid
    out = {f: getattr(g, f)[:g.n + 1].tobytes() for f in FIELDS}
    out["values"] = sky.values.tobytes()
    out["n"] = (g.n, sky.n_values)
    return out


def assert_same(a, b):
    sa, sb = state(a), state(b)
    for key in sa:
        assert sa[key] == sb[key], key


def clone_host(sky):
    """a host-route sky that continues where `sky` is (its tracer, and so its launch log, is shared)"""
    twin = copy.copy(sky)
    twin._grid = copy.deepcopy(sky._grid)
    twin._values = sky._values.copy()
    return twin


def menu(G):
    return {
        "default-2": G.check_refine,
        "default-10": lambda s, a, b: G.check_refine(s, a, b, percentage=10),        # a plain callable: the gr_sky_pairs route
        "function-box": G.refine_function(G.RadialBox(15.0, 40.0)),
        "fine-open-r": G.fine_refine_function(G.RadialBox(800.0, math.inf, open=(True, False)), percentage=10),
        "fine-inner": G.fine_refine_function(G.RadialBox(1.2369706551751847, 2.0), percentage=20),
        "closed-wrapped-phi": G.fine_refine_function([G.RadialBox(5.0, 30.0, ϕ=[(0.0, 0.7), (5.6, 2 * math.pi)], open=False),
                                                      G.RadialBox(2.0, 4.0, ϕ=(1.0, 2.5), open=False)], percentage=10),
        "level-4": G.refine_to_level(4),
    }


@pytest.fixture(scope="module")
def host_base(G, _ens_session):
    """the host-route sky after trace_initial and two trace_steps (pairs of lanes), computed once and only ever cloned"""
    _ens_session.set("tangent_pairs", 1)
    sky = new_sky(G, _ens_session, resident=False)
    _ens_session.set("tangent_pairs", 2)
    return sky


@pytest.mark.parametrize("shape", [0, 1], ids=["lane", "pair"])
def test_the_resident_sky_equals_the_host_route(G, ens, shape):
    ens.set("tangent_pairs", shape)
    host, dev = new_sky(G, ens, False, steps=None), new_sky(G, ens, True, steps=None)
    assert dev.resident and not host.resident
    G.trace_initial(host)
    G.trace_initial(dev)
    assert launches(dev) == launches(host) == [9, 72, 648] and len(dev.grid) == 819
    assert_same(host, dev)
    for _ in range(2):
        need = G.find_need_refine(host)
        np.testing.assert_array_equal(G.find_need_refine(dev), need)
        before = len(launches(dev))
        G.trace_step(host)
        G.trace_step(dev)
        assert launches(dev, before) == [8 * need.size] and launches(dev) == launches(host)
        assert_same(host, dev)
    assert len(dev.grid) == 40995 and dev.n_values == 40995
    # what is built on the mirror reads the same
    for a, b in zip(G.unpack_sky(host), G.unpack_sky(dev)):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["default-2", "default-10", "function-box", "fine-open-r", "fine-inner", "closed-wrapped-phi", "level-4"])
def test_one_more_step_under_each_criterion(G, ens, host_base, name):
    ens.set("tangent_pairs", 1)
    criterion = menu(G)[name]
    host, dev = clone_host(host_base), new_sky(G, ens, True)
    assert_same(host, dev)
    need = G.find_need_refine(host, criterion)
    np.testing.assert_array_equal(G.find_need_refine(dev, criterion), need)
    at_host, at_dev = len(launches(host)), len(launches(dev))
    G.trace_step(host, criterion)
    G.trace_step(dev, criterion)
    assert launches(dev, at_dev) == launches(host, at_host) == ([8 * need.size] if need.size else [])
    assert len(dev.grid) == 40995 + 9 * need.size
    assert_same(host, dev)
    print(f"{name}: {need.size} cells refined")


def test_refine_and_trace_with_a_host_list(G, ens, host_base):
    ens.set("tangent_pairs", 1)
    host, dev = clone_host(host_base), new_sky(G, ens, True)
    leaves = host.grid.leaves()
    ids = leaves[[5, 1, 700, 333, leaves.size - 1, 12345]]          # (in no order, as refine_many takes them)
    G.refine_and_trace(host, ids)
    G.refine_and_trace(dev, ids)
    assert launches(dev)[-1] == 48 and len(dev.grid) == 40995 + 54
    assert_same(host, dev)
    np.testing.assert_array_equal(dev.grid.children[ids], 40996 + 9 * np.arange(6)[:, None] + np.arange(9)[None, :])


def test_the_pair_list_of_the_device_is_bordering_pairs(G, ens):
    ens.set("tangent_pairs", 1)
    dev = new_sky(G, ens, True)
    i1, i2 = dev.device_pairs()
    a, b = dev.grid.bordering_pairs()
    assert i1.size == a.size > 100_000
    np.testing.assert_array_equal(i1, a)
    np.testing.assert_array_equal(i2, b)


def test_the_census_of_the_bins_is_where_the_emissivity_map_is_lit(G, ens):
    ens.set("tangent_pairs", 1)
    m, _, d = scene(G)
    dev = new_sky(G, ens, True)
    r_bins, ϕ_bins = np.geomspace(m.isco(), 1000.0, 100), np.linspace(0.0, 2 * math.pi, 100)
    counts = dev.device_occupancy(r_bins, ϕ_bins)
    lit = G.bin_emissivity_grid(m, d, r_bins, ϕ_bins, dev) != 0
    np.testing.assert_array_equal(counts != 0, lit)
    assert 0 < lit.sum() < lit.size
    v, _, r_i, ϕ_i = G.adaptive._binned_cells(dev, r_bins, ϕ_bins)
    ref = np.zeros_like(counts)
    np.add.at(ref, (r_i, ϕ_i), 1)
    np.testing.assert_array_equal(counts, ref)            # (no row of this sky has J g² = ±0: every leaf in a bin counts)
    np.testing.assert_array_equal(dev.device_occupancy(r_bins, ϕ_bins), counts)
    np.testing.assert_array_equal(dev.device_occupancy(r_bins, ϕ_bins, Γ=None), ref)
    assert G.empty_fraction(None, None, counts) == np.count_nonzero(lit) / lit.size


def test_step_block_on_both_skies(G, ens, host_base):
    ens.set("tangent_pairs", 1)
    m, _, d = scene(G)
    host, dev = clone_host(host_base), new_sky(G, ens, True)
    codes = [G.step_block(m, d, s, N=100, split=5, top=4) for s in (host, dev)]
    assert codes[0] is codes[1] and codes[0] in (G.StepBlockCodes.not_converged, G.StepBlockCodes.converged)
    assert_same(host, dev)
    # too many cells for the limit: the code says so and nothing is refined
    n = len(dev.grid)
    if codes[0] is G.StepBlockCodes.not_converged:
        assert n > 40995
        again = [G.step_block(m, d, s, N=100, split=5, top=4, limit=0) for s in (host, dev)]
        assert again[0] is again[1] and again[0] in (G.StepBlockCodes.limit_exceeded, G.StepBlockCodes.converged)
        assert len(dev.grid) == n
        assert_same(host, dev)
    # a metric of the caller's own reads the map of the mirror
    custom = [G.step_block(m, d, s, N=100, split=5, top=4, metric=lambda r, ϕ, block: float(np.mean(block != 0))) for s in (host, dev)]
    assert custom[0] is custom[1]
    assert_same(host, dev)


def test_adaptive_solve_on_both_skies(G, ens):
    ens.set("tangent_pairs", 1)
    m, _, d = scene(G)
    host, dev = new_sky(G, ens, False, steps=None), new_sky(G, ens, True, steps=None)
    n_host = G.adaptive_solve(m, d, host, trace_calls=1, limit=8, N=100, verbose=False)
    n_dev = G.adaptive_solve(m, d, dev, trace_calls=1, limit=8, N=100, verbose=False)
    assert n_dev == n_host and 7 <= n_dev <= 10
    assert launches(dev) == launches(host)
    assert_same(host, dev)
    print(f"adaptive_solve: {n_dev} iterations, {len(dev.grid)} cells")


def download_again(sky):
    """drop the mirrors: the next read fetches every cell from the device"""
    sky._n_values, sky._stale = 0, True


def test_refusals_leave_the_sky_as_it_was(G, ens):
    ens.set("tangent_pairs", 1)
    dev = new_sky(G, ens, True, steps=0)
    before, n_launches = state(dev), len(launches(dev))
    for ids in ([1], [0], [820], [100, 100], [100, 1], [-3]):       # refined already, out of range, named twice
        with pytest.raises(ValueError):
            G.refine_and_trace(dev, ids)
        download_again(dev)
        assert state(dev) == before and len(launches(dev)) == n_launches
    host = new_sky(G, ens, False, steps=0)
    G.refine_and_trace(host, [100])
    G.refine_and_trace(dev, [100])                                       # ... and the sky still works
    assert len(dev.grid) == 828 and launches(dev)[-1] == 8
    assert_same(host, dev)
    download_again(dev)                                                  # (the incremental mirror is the device's state)
    assert_same(host, dev)
    with pytest.raises(ValueError, match="ONE context"):
        G.AdaptiveSky(*scene(G), ensemble=G.EnsembleMI355X(devices=[0, 0]), resident=True)
    with pytest.raises(ValueError, match="traced already"):
        G.trace_initial(dev)
