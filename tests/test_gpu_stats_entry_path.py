"""The statistics of a launch and the path of a wave outside its step loop (LaneStats::flush, gr_stats_fold.hpp, k_stats_fold;
Ray::finalize's early exit for rays decided at the start).  The nine counters of a launch against what the same rays give one
by one -- a launch of ONE ray has nothing to reduce: its wave holds one ray's counts and 63 zeros -- and against the per-ray
summaries (out_mode 4) of the launch that produced them; partial last waves, accumulation over launches, launches without
statistics, a scene whose rays are all decided before their first step, a non-Kerr metric and the fp32 kernels.  A per-ray summary
holds (g, ρ, t, status) and no step counts: rays and the status counts are checked against the summaries, the step counts against
the same rays in launches of their own.  Needs an MI355X."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALIMS, BLIMS = (-60.0, 60.0), (-35.0, 35.0)
KEYS = ("rays", "accepted_steps", "rejected_steps", "rhs_evals", "flagged_rays")


def _nine(st):
    return [int(st[k]) for k in KEYS] + [int(v) for v in st["status_count"]]


def _kerr(G):
    m = G.KerrMetric(1.0, 0.998)
    return m, np.array([0.0, 1000.0, math.radians(75.0), 0.0]), G.ThinDisc(m.isco(), 50.0)


def _config(G, ens, m, x, d, W, H, alims=ALIMS, blims=BLIMS):
    return G.render_configuration(m, x, d, 2000.0, image_width=W, image_height=H, alpha_lims=alims, beta_lims=blims, ensemble=ens)


def _launch(cfg, pf, n, rg=None, stats="new", img=None):
    """One gr_render_device launch -> (image bytes as a numpy array, stats tensor or None)"""
    import torch

    from gradus_jl_amd import device as gdev

    dev = torch.device("cuda", 0)
    if img is None:
        img = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    st = gdev.new_stats(dev) if isinstance(stats, str) else stats
    gdev.render_device(cfg, pf, img, rg, st)
    torch.cuda.synchronize()
    return img.cpu().numpy(), st


def _ray_by_ray(cfg, pf, n):
    """Every ray of the plane in a launch of its own (kernel and precision as the ensemble has them): the image and the nine sums
    formed on the host from the n single-ray counter sets."""
    import torch

    from gradus_jl_amd import _lib
    from gradus_jl_amd import device as gdev

    dev = torch.device("cuda", 0)
    px = torch.empty(1, dtype=torch.float64, device=dev)
    img = torch.empty(n, dtype=torch.float64, device=dev)
    per_ray = torch.zeros((n, 11), dtype=torch.int64, device=dev)
    for i in range(n):
        gdev.render_device(cfg, pf, px, _lib.gr_range(i, 1, 1, 1), per_ray[i])
        img[i] = px[0]
    torch.cuda.synchronize()
    h = per_ray.cpu().numpy()
    assert (h[:, 0] == 1).all()          # every launch counted its one ray
    return img.cpu().numpy(), [int(v) for v in h[:, :9].sum(axis=0)]


_REF = {}


def _kerr_reference(G, ens, W, H):
    """(image, nine sums) of the W x H Kerr render ray by ray, on the one-ray-per-lane kernel: computed once, shared, left unchanged"""
    if (W, H) not in _REF:
        ens.set("kernel", 0).set("precision", 64)
        m, x, d = _kerr(G)
        pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
        _REF[(W, H)] = _ray_by_ray(_config(G, ens, m, x, d, W, H), pf, W * H)
    return _REF[(W, H)]


def _check_identities(nine, n):
    rays, acc, rej, rhs, flagged = nine[:5]
    assert rays == n
    assert rhs == 2 * rays + 6 * (acc + rej)
    assert sum(nine[5:]) == rays          # every ray has one status (a flagged ray counts as NoStatus)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("shape", [(24, 24), (20, 12)])
def test_render_counters_equal_the_per_ray_sums(G, ens, shape, kernel):
    """24 x 24: nine whole 8 x 8 tiles; 20 x 12: no whole tiles, the last wave of the launch has 48 rays."""
    from gradus_jl_amd import device as gdev

    W, H = shape
    ref_img, ref_nine = _kerr_reference(G, ens, W, H)
    ens.set("kernel", kernel).set("precision", 64)
    m, x, d = _kerr(G)
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    img, st = _launch(_config(G, ens, m, x, d, W, H), pf, W * H)
    nine = _nine(gdev.stats_dict(st))
    print(f"{W}x{H} kernel {kernel}: launch {nine}  ray by ray {ref_nine}")
    _check_identities(nine, W * H)
    assert nine == ref_nine
    assert img.tobytes() == ref_img.tobytes()


def _summary_launch(G, ens, alpha, beta):
    """gr_ray_summary (out_mode 4) of a ray set: (rows (g, ρ, t, status), nine counters of that launch)"""
    from gradus_jl_amd import _lib
    from gradus_jl_amd.rendering import abi_pointfunction
    from gradus_jl_amd.tracing import lnr_momentum_to_global_velocity_matrix

    m, x, d = _kerr(G)
    config = G.tracing_configuration(m, x, np.zeros((1, 4)), d, 2000.0, ensemble=ens)
    cfg = config.abi_config()
    pf, keep = abi_pointfunction(G.ConstPointFunctions.redshift(m, x))
    Mx = lnr_momentum_to_global_velocity_matrix(m, config.position)
    alpha, beta = np.ascontiguousarray(alpha, dtype=np.float64), np.ascontiguousarray(beta, dtype=np.float64)
    rs = _lib.gr_rayset()
    for i in range(4):
        rs.x_obs[i] = float(config.position[i])
        for k in range(4):
            rs.Mx[4 * i + k] = float(Mx[i, k])
    rs.alpha, rs.beta, rs.area, rs.n = alpha.ctypes.data, beta.ctypes.data, None, alpha.size
    out = np.zeros((alpha.size, 4))
    st = _lib.gr_stats()
    _lib.check(_lib.load().gr_ray_summary(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), out.ctypes.data, C.byref(st)))
    return out, _nine(st.asdict())


def _status_histogram(rows):
    s = rows[:, 3].astype(np.int64)
    return [int((s == k).sum()) for k in range(4)]


@pytest.mark.parametrize("kernel", [0, 1])
def test_ray_sets_of_5000_rays_and_of_one(G, ens, kernel):
    """5000 = 78 waves of 64 and one of 8.  The counters of the launch against its own per-ray summaries (rays, status counts),
    and against the same rays launched in five pieces whose waves are made up differently (1 + 7 + 64 + 129 + 4799)."""
    ens.set("kernel", kernel).set("precision", 64)
    rng = np.random.default_rng(26)
    alpha, beta = rng.uniform(-60.0, 60.0, 5000), rng.uniform(-35.0, 35.0, 5000)
    rows, nine = _summary_launch(G, ens, alpha, beta)
    _check_identities(nine, 5000)
    assert nine[5:] == _status_histogram(rows)
    pieces, cut = [], np.cumsum([0, 1, 7, 64, 129, 4799])
    for a, b in zip(cut[:-1], cut[1:]):
        r, n9 = _summary_launch(G, ens, alpha[a:b], beta[a:b])
        assert r.tobytes() == rows[a:b].tobytes()
        _check_identities(n9, b - a)
        assert n9[5:] == _status_histogram(r)
        pieces.append(n9)
    print(f"kernel {kernel}: 5000 rays {nine}; first piece (one ray) {pieces[0]}")
    assert nine == [int(v) for v in np.sum(pieces, axis=0)]
    assert pieces[0][0] == 1


def test_both_kernels_count_a_ray_set_alike(G, ens):
    rng = np.random.default_rng(27)
    alpha, beta = rng.uniform(-60.0, 60.0, 5000), rng.uniform(-35.0, 35.0, 5000)
    got = []
    for kernel in (0, 1):
        ens.set("kernel", kernel).set("precision", 64)
        got.append(_summary_launch(G, ens, alpha, beta))
    assert got[0][0].tobytes() == got[1][0].tobytes()
    assert got[0][1] == got[1][1]


@pytest.mark.parametrize("kernel", [0, 1])
def test_two_launches_into_one_stats_tensor(G, ens, kernel):
    from gradus_jl_amd import device as gdev

    ens.set("kernel", kernel).set("precision", 64)
    m, x, d = _kerr(G)
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    ca, cb = _config(G, ens, m, x, d, 24, 24), _config(G, ens, m, x, d, 20, 12)
    _, sa = _launch(ca, pf, 576)
    _, sb = _launch(cb, pf, 240)
    _, both = _launch(ca, pf, 576)
    _launch(cb, pf, 240, stats=both)
    a, b, ab = (_nine(gdev.stats_dict(t)) for t in (sa, sb, both))
    assert ab == [p + q for p, q in zip(a, b)]
    assert ab[0] == 576 + 240


@pytest.mark.parametrize("kernel", [0, 1])
def test_a_launch_without_statistics_gives_the_same_image(G, ens, kernel):
    ens.set("kernel", kernel).set("precision", 64)
    m, x, d = _kerr(G)
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    cfg = _config(G, ens, m, x, d, 24, 24)
    with_stats, _ = _launch(cfg, pf, 576)
    without, none = _launch(cfg, pf, 576, stats=None)
    assert none is None
    assert with_stats.tobytes() == without.tobytes()
    assert np.isnan(without).any() and not np.isnan(without).all()          # misses and hits: the launch wrote every pixel


@pytest.mark.parametrize("kernel", [0, 1])
def test_rays_decided_at_the_start_against_the_start_cull_switched_off(G, ens, monkeypatch, kernel):
    """Observer at r = 1000, a disc that ends at r = 2, window ± 60: the start's tests decide the rays of whole waves, which go
    from Ray::init to their fill-value store.  With GRADUS_MI355X_START_CULL=0 the same rays are traced: the same image bytes
    and status counts, only the step counts differ."""
    from gradus_jl_amd import device as gdev

    ens.set("kernel", kernel).set("precision", 64)
    m = G.KerrMetric(1.0, 0.998)
    x = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
    d = G.ThinDisc(m.isco(), 2.0)
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    cfg = _config(G, ens, m, x, d, 24, 24, (-60.0, 60.0), (-60.0, 60.0))
    monkeypatch.delenv("GRADUS_MI355X_START_CULL", raising=False)
    img_on, st_on = _launch(cfg, pf, 576)
    monkeypatch.setenv("GRADUS_MI355X_START_CULL", "0")
    img_off, st_off = _launch(cfg, pf, 576)
    monkeypatch.delenv("GRADUS_MI355X_START_CULL", raising=False)
    on, off = _nine(gdev.stats_dict(st_on)), _nine(gdev.stats_dict(st_off))
    print(f"kernel {kernel}: start cull on {on}  off {off}")
    assert img_on.tobytes() == img_off.tobytes()
    assert not (img_on == -7.0).any()          # every pixel was written (the buffer starts at -7)
    _check_identities(on, 576)
    _check_identities(off, 576)
    assert on[0] == off[0] and on[4:] == off[4:]          # rays, flagged rays, status counts
    assert on[1] < off[1]          # the cull fired: fewer accepted steps with it


@pytest.mark.parametrize("case", ["johannsen", "fp32"])
def test_other_kernels_share_the_counters(G, ens, case):
    """LaneStats is one template for every metric and precision: a Johannsen launch and an fp32 Kerr launch, 16 x 16, against the
    same rays one by one."""
    from gradus_jl_amd import device as gdev

    if case == "johannsen":
        ens.set("kernel", 2).set("precision", 64)
        m = G.JohannsenMetric(1.0, 0.7, 2.0, 0.0, 0.0, 1.0)
        x = np.array([0.0, 1000.0, math.radians(70.0), 0.0])
        pf = G.ConstPointFunctions.shadow()          # (no plunging table needed)
    else:
        ens.set("kernel", 0).set("precision", 32)
        m = G.KerrMetric(1.0, 0.998)
        x = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
        pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    cfg = _config(G, ens, m, x, G.ThinDisc(m.isco(), 50.0), 16, 16)
    img, st = _launch(cfg, pf, 256)
    nine = _nine(gdev.stats_dict(st))
    ref_img, ref_nine = _ray_by_ray(cfg, pf, 256)
    print(f"{case}: launch {nine}  ray by ray {ref_nine}")
    _check_identities(nine, 256)
    assert nine == ref_nine
    assert img.tobytes() == ref_img.tobytes()
