"""The live-first tile order of an image launch (gr_tile_order.hpp, k_tile_classify, k_tile_partition; gr_ctx_set "live_first",
GRADUS_MI355X_LIVE_FIRST): the one-ray-per-lane kernel takes the tiles with a corner ray that is traced first and
the tiles whose four corner rays are decided at the start last.  Only the order of the work changes: on small windows of the
bench scene the image bytes (into a buffer that starts at -7: every pixel written) and the nine counters with "live_first" 2 equal those with 0,
two runs give the same bytes and the same permutation, and the permutation the device built is a bijection with the live class
first, each class ascending.  Windows with live and dead tiles, with no dead tile, with dead tiles only; both tile shapes; a
block-cyclic range; each cull switch off in turn; the launches that keep their order.  Needs an MI355X."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("rays", "accepted_steps", "rejected_steps", "rhs_evals", "flagged_rays")
SWITCHES = ("GRADUS_MI355X_ESCAPE_CULL", "GRADUS_MI355X_START_CULL", "GRADUS_MI355X_PASS_CULL", "GRADUS_MI355X_ENTRY_CULL",
            "GRADUS_MI355X_DEFER_CULL")
# name -> (width, height, α limits, β limits): the bench scene's metric, disc and observer
WINDOWS = {
    "mixed": (256, 128, (-60.0, 60.0), (-35.0, 35.0)),       # 512 tiles, the disc's image and the sky around it
    "all-live": (64, 32, (-20.0, 20.0), (-5.0, 5.0)),        # every ray turns deep inside R_cull: none is decided at the start
    "all-dead": (64, 32, (70.0, 90.0), (-35.0, 35.0)),       # every ray turns outside R_cull: all are decided at the start
    "deep": (512, 256, (-60.0, 60.0), (-35.0, 35.0)),        # 2048 tiles: eight per CU of the device's 256
}


@pytest.fixture
def lf(ens):
    """The session's ensemble on the one-ray-per-lane fp64 kernel; "live_first" and "tile_rows" back at their defaults afterwards
    (the shared fixture resets neither)."""
    ens.set("kernel", 0).set("precision", 64)
    yield ens
    ens.set("live_first", 1).set("tile_rows", 8)


def _scene(G, ens, name):
    W, H, alims, blims = WINDOWS[name]
    m = G.KerrMetric(1.0, 0.998)
    x = np.array([0.0, 1000.0, math.radians(75.0), 0.0])
    cfg = G.render_configuration(m, x, G.ThinDisc(m.isco(), 50.0), 2000.0, image_width=W, image_height=H, alpha_lims=alims,
                                 beta_lims=blims, ensemble=ens)
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    return cfg, pf, W, H


def _order(ens, cap):
    """(permutation, live tiles) of the context's last trace launch as the device built it, or (None, 0): not reordered"""
    from gradus_jl_amd import _lib

    L = _lib.load()
    L.gr_debug_tile_order.restype = C.c_int32
    L.gr_debug_tile_order.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    perm = np.full(cap, 0xFFFFFFFF, dtype=np.uint32)
    tiles, live = C.c_int64(-1), C.c_int64(-1)
    _lib.check(L.gr_debug_tile_order(ens.ctx.handle, perm.ctypes.data, cap, C.byref(tiles), C.byref(live)))
    if tiles.value == 0:
        return None, 0
    assert 0 < tiles.value <= cap
    return perm[:tiles.value], int(live.value)


def _launch(ens, cfg, pf, n, mode, rg=None):
    """One gr_render_device launch with "live_first" = mode -> (image, nine counters, permutation or None, live tiles)"""
    import torch

    from gradus_jl_amd import device as gdev

    ens.set("live_first", mode)
    dev = torch.device("cuda", 0)
    img = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    st = gdev.new_stats(dev)
    gdev.render_device(cfg, pf, img, rg, st)
    torch.cuda.synchronize()
    d = gdev.stats_dict(st)
    perm, live = _order(ens, max(n // 64, 1))
    return img.cpu().numpy(), [int(d[k]) for k in KEYS] + [int(v) for v in d["status_count"]], perm, live


def _check_order(perm, live, tiles):
    assert perm is not None and perm.size == tiles and 0 <= live <= tiles
    assert np.array_equal(np.sort(perm), np.arange(tiles, dtype=np.uint32))          # a bijection of [0, tiles)
    assert (np.diff(perm[:live].astype(np.int64)) > 0).all() and (np.diff(perm[live:].astype(np.int64)) > 0).all()


def _same(a, b, n):
    assert a[0].tobytes() == b[0].tobytes()          # NaN pattern included
    assert not (a[0] == -7.0).any() and not (b[0] == -7.0).any()          # every pixel was written
    assert a[1] == b[1]
    assert a[1][0] == n and a[1][4] == 0


_OFF = {}


def _off(G, ens, name, rows=8):
    """The window with the order off, the library's default tile shape or 16 x 4: computed once, shared, left unchanged"""
    if (name, rows) not in _OFF:
        ens.set("tile_rows", rows)
        cfg, pf, W, H = _scene(G, ens, name)
        r = _launch(ens, cfg, pf, W * H, 0)
        assert r[2] is None
        _OFF[(name, rows)] = r
    return _OFF[(name, rows)]


@pytest.mark.parametrize("rows", [8, 16])
@pytest.mark.parametrize("name", ["mixed", "all-live", "all-dead"])
def test_live_first_changes_no_byte_and_no_counter(G, lf, name, rows):
    off = _off(G, lf, name, rows)
    lf.set("tile_rows", rows)
    cfg, pf, W, H = _scene(G, lf, name)
    tiles = W * H // 64
    on = _launch(lf, cfg, pf, W * H, 2)
    again = _launch(lf, cfg, pf, W * H, 2)
    _same(on, off, W * H)
    _same(again, off, W * H)
    _check_order(on[2], on[3], tiles)
    assert np.array_equal(on[2], again[2]) and on[3] == again[3]          # the same order at every launch
    print(f"{name} {rows} rows: {on[3]} live of {tiles} tiles; counters {on[1]}")
    if name == "mixed":
        assert 0 < on[3] < tiles
        assert not np.array_equal(on[2], np.arange(tiles, dtype=np.uint32))
        # the flag against the pixels: a tile in the dead class holds no hit at any of its four corners
        img = on[0].reshape(W, H)
        tr = 3 if rows == 8 else 4
        for t in on[2][on[3]:]:
            tx, ty = divmod(int(t), H >> tr)
            for lane in (0, rows - 1, 64 - rows, 63):
                assert np.isnan(img[(tx << (6 - tr)) + (lane >> tr), (ty << tr) + (lane & (rows - 1))])
    elif name == "all-live":
        assert on[3] == tiles and np.array_equal(on[2], np.arange(tiles, dtype=np.uint32))
    else:
        assert on[3] == 0 and np.array_equal(on[2], np.arange(tiles, dtype=np.uint32))
        assert on[1][1] == 0 and np.isnan(on[0]).all()          # no step was taken


def test_block_cyclic_range_rank_1_of_2(G, lf):
    cfg, pf, W, H = _scene(G, lf, "mixed")
    plan = G.shard_plan(W, H, 2, 1)
    rg = plan.ray_range()
    off = _launch(lf, cfg, pf, plan.count, 0, rg)
    on = _launch(lf, cfg, pf, plan.count, 2, rg)
    _same(on, off, plan.count)
    _check_order(on[2], on[3], plan.count // 64)
    assert 0 < on[3] < plan.count // 64
    full = _off(G, lf, "mixed")[0].reshape(W, H)
    cols = np.concatenate([np.arange(b * plan.block // H, (b + 1) * plan.block // H) for b in range(1, 2 * plan.n_blocks, 2)])
    assert on[0].tobytes() == np.ascontiguousarray(full[cols]).tobytes()          # rank 1's columns of the whole image


@pytest.mark.parametrize("switch", SWITCHES)
def test_each_cull_switch_off(G, lf, monkeypatch, switch):
    cfg, pf, W, H = _scene(G, lf, "mixed")
    monkeypatch.setenv(switch, "0")
    off = _launch(lf, cfg, pf, W * H, 0)
    on = _launch(lf, cfg, pf, W * H, 2)
    monkeypatch.delenv(switch, raising=False)
    _same(on, off, W * H)
    assert on[0].tobytes() == _off(G, lf, "mixed")[0].tobytes()          # (a cull changes no pixel either)
    if switch == "GRADUS_MI355X_START_CULL":
        assert on[2] is None          # no ray is decided at the start: nothing to order by
    else:
        _check_order(on[2], on[3], W * H // 64)
        assert 0 < on[3] < W * H // 64


def test_the_switch_in_the_environment(G, lf, monkeypatch):
    """GRADUS_MI355X_LIVE_FIRST = 0, 1 or 2 takes the knob's place at every launch; anything else leaves the knob."""
    cfg, pf, W, H = _scene(G, lf, "mixed")
    off = _off(G, lf, "mixed")
    for env, knob, applied in (("0", 2, False), ("2", 0, True), ("1", 2, False), ("on", 2, True), ("on", 0, False)):
        monkeypatch.setenv("GRADUS_MI355X_LIVE_FIRST", env)
        r = _launch(lf, cfg, pf, W * H, knob)
        monkeypatch.delenv("GRADUS_MI355X_LIVE_FIRST", raising=False)
        assert (r[2] is not None) == applied, (env, knob)          # ("1": 512 tiles are fewer than the device holds waves)
        _same(r, off, W * H)


def test_launches_that_keep_their_order(G, lf):
    """The persistent kernel, the fp32 kernels, a window without tiles, a metric without the start cull, and -- under "live_first"
    1 -- a launch of fewer tiles than the device holds waves."""
    cfg, pf, W, H = _scene(G, lf, "mixed")
    off = _off(G, lf, "mixed")
    auto = _launch(lf, cfg, pf, W * H, 1)
    assert auto[2] is None          # 512 tiles: every wave is resident at once
    _same(auto, off, W * H)
    lf.set("kernel", 1)
    pers = _launch(lf, cfg, pf, W * H, 2)
    assert pers[2] is None
    _same(pers, off, W * H)
    lf.set("kernel", 0).set("swizzle", 0)
    flat = _launch(lf, cfg, pf, W * H, 2)
    assert flat[2] is None
    _same(flat, off, W * H)
    lf.set("swizzle", 1).set("precision", 32)
    assert _launch(lf, cfg, pf, W * H, 2)[2] is None
    lf.set("precision", 64)
    mj = G.JohannsenMetric(1.0, 0.7, 2.0, 0.0, 0.0, 1.0)
    x = np.array([0.0, 1000.0, math.radians(70.0), 0.0])
    cj = G.render_configuration(mj, x, G.ThinDisc(mj.isco(), 50.0), 2000.0, image_width=64, image_height=64, alpha_lims=(-60.0, 60.0),
                                beta_lims=(-35.0, 35.0), ensemble=lf)
    j_on = _launch(lf, cj, G.ConstPointFunctions.shadow(), 4096, 2)
    j_off = _launch(lf, cj, G.ConstPointFunctions.shadow(), 4096, 0)
    assert j_on[2] is None and j_on[0].tobytes() == j_off[0].tobytes() and j_on[1] == j_off[1]


def test_auto_orders_a_launch_deeper_than_the_device(G, lf):
    """512 x 256: 2048 tiles, the smallest launch "live_first" 1 reorders and the learned order (lpt_prepare) looks at."""
    cfg, pf, W, H = _scene(G, lf, "deep")
    off = _off(G, lf, "deep")
    auto = _launch(lf, cfg, pf, W * H, 1)
    _same(auto, off, W * H)
    _check_order(auto[2], auto[3], 2048)
    assert 0 < auto[3] < 2048


def test_a_learned_order_takes_precedence(G, lf):
    """ "lpt_lane" 1 with "lpt" 2: the first render of a plane records its tiles' costs, the next ones take them longest first;
    neither is reordered."""
    cfg, pf, W, H = _scene(G, lf, "deep")
    off = _off(G, lf, "deep")
    lf.set("lpt_lane", 1).set("lpt", 2)
    runs = [_launch(lf, cfg, pf, W * H, 2) for _ in range(3)]
    for r in runs:
        _same(r, off, W * H)
        assert r[2] is None
