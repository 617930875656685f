"""ctypes binding of tests/host_harness_culls.cpp: whole 8 x 8 tiles of an image plane traced by the HIP integrator compiled for
the host (g++) with the miss culls (Ray::start_decided, Ray::step) -- the step loop's culls, the decisions at the
start, the pass cull, the entry cull, the defer cull -- switched one by one; which of them ended each ray; the bounds the pass
cull and the entry cull decide by, ray by ray; and the census of each mechanism's arms."""
import ctypes as C

import numpy as np

import hostbuild

# struct hhc_out of the harness, in its order: what render_tiles returns per ray
OUT = (("image", np.float64), ("status", np.int32), ("nacc", np.int32), ("nrej", np.int32), ("at_start", np.int32),
       ("by_pass", np.int32), ("marked", np.int32), ("defer_end", np.int32), ("entry_step", np.int32), ("r_start", np.float64),
       ("vr_start", np.float64), ("r_last", np.float64), ("vr_last", np.float64))
PASS_BOUNDS = ("E", "L", "Q", "u0", "uc", "mu0", "mu_rising", "vr", "u_lo", "u_hi", "Ta_lo", "Tb_hi", "Om_lo", "Om_hi", "psi0", "decided")
ENTRY_BOUNDS = PASS_BOUNDS + ("asked", "steps")

# Per mechanism: (arms, the arm each arm is compared with, ratios) for census().  An arm is (step-loop culls, decisions at the
# start, entry cull, defer cull, zeta); zeta None = the caller's (-1: the library's), 0.0 = the pass cull off.  The pass cull is a
# test of the start cull and is off with it.  A ratio is (key, arm, over arm).
#   "all" / "both+pass" is the library as shipped, "start" / "start+pass" its GRADUS_MI355X_ESCAPE_CULL=0 arm, "no-entry"
#   GRADUS_MI355X_ENTRY_CULL=0, "no-defer" GRADUS_MI355X_DEFER_CULL=0, "off" / "full" every cull off.
# "escape_switch_bracket_ratio" is what tests/test_gpu_escape_cull.py brackets: accepted steps with GRADUS_MI355X_ESCAPE_CULL unset
# over =0, the decisions at the start on in both arms.
# The start cull and the step loop's culls, as the library was before the pass cull:
STEP = ({"off": (0, 0, 1, 1, 0.0), "start": (0, 1, 1, 1, 0.0), "step": (1, 0, 1, 1, 0.0), "both": (1, 1, 1, 1, 0.0)},
        "off",
        {"wave_steps_ratio_vs_escape_cull_alone": {"both": ("wave_steps", "both", "step")},
         "wave_steps_ratio_vs_off": {k: ("wave_steps", k, "off") for k in ("start", "step", "both")},
         "escape_switch_bracket_ratio": ("accepted_steps", "both", "start")})
# The pass cull on against off, under the start cull alone and under all culls (the launch):
PASS = ({"start": (0, 1, 1, 1, 0.0), "start+pass": (0, 1, 1, 1, None), "both": (1, 1, 1, 1, 0.0), "both+pass": (1, 1, 1, 1, None)},
        {"start": "start", "start+pass": "start", "both": "both", "both+pass": "both"},
        {"pass_wave_steps_ratio": ("wave_steps", "both+pass", "both"),
         "pass_accepted_steps_ratio": ("accepted_steps", "both+pass", "both"),
         "escape_switch_bracket_ratio": ("accepted_steps", "both+pass", "start+pass"),
         "escape_switch_bracket_ratio_pass_off": ("accepted_steps", "both", "start")})
# The entry cull on against off, every other cull on:
ENTRY = ({"start": (0, 1, 1, 1, None), "no-entry": (1, 1, 0, 1, None), "all": (1, 1, 1, 1, None)},
         "no-entry",
         {"entry_wave_steps_ratio": ("wave_steps", "all", "no-entry"),
          "entry_accepted_steps_ratio": ("accepted_steps", "all", "no-entry"),
          "escape_switch_bracket_ratio": ("accepted_steps", "all", "start")})
# The defer cull on against off, every other cull on, and the full trace:
DEFER = ({"all": (1, 1, 1, 1, None), "no-defer": (1, 1, 1, 0, None), "start": (0, 1, 1, 1, None), "full": (0, 0, 0, 0, 0.0)},
         "full",
         {"defer_wave_steps_ratio": ("wave_steps", "all", "no-defer"),
          "defer_accepted_steps_ratio": ("accepted_steps", "all", "no-defer"),
          "escape_switch_bracket_ratio": ("accepted_steps", "all", "start")})


class hhc_out(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _ in OUT]


def lib(defer_zeta=None):
    """The harness with the library's kDeferCullZeta, or (the census) built with another one.  Builds it where it is stale: a
    parent of worker processes calls this once before it starts them."""
    if defer_zeta is None:
        L = hostbuild.load("host_harness_culls.cpp")
    else:
        L = hostbuild.load("host_harness_culls.cpp", defines=[f"GR_DEFER_CULL_ZETA={float(defer_zeta)!r}"], suffix=f"_{float(defer_zeta):.4f}")
    for f in ("hhc_gate_radius", "hhc_zeta", "hhc_zeta_dip", "hhc_zeta_defer"):
        getattr(L, f).restype = C.c_double
    return L


def gate_radius(config):
    cfg = config.abi_config()
    return float(lib().hhc_gate_radius(C.byref(cfg)))


def zeta():
    """The library's ζ (kPassCullZeta): R_pass = ζ R_cull."""
    return float(lib().hhc_zeta())


def zeta_dip():
    """The entry cull's depth limit (kEntryCullZeta): R_dip = ζ_dip R_cull."""
    return float(lib().hhc_zeta_dip())


def zeta_defer(defer_zeta=None):
    """The defer cull's depth limit (kDeferCullZeta): R_defer = ζ_defer R_cull."""
    return float(lib(defer_zeta).hhc_zeta_defer())


def default_culls():
    """(Params::entry_cull, Params::defer_cull) as memset + derive_params leave them: what render_tiles' entry = defer = 1 trace with."""
    entry, defer = C.c_int32(-1), C.c_int32(-1)
    lib().hhc_default_culls(C.byref(entry), C.byref(defer))
    return entry.value, defer.value


def render_tiles(G, config, pf, tiles, step=1, start=1, entry=1, defer=1, zeta=-1.0, defer_zeta=None):
    """{name: (len(tiles), 64) array} over OUT: lane l of a tile is its column l // 8, row l % 8.  The defaults are the library as
    shipped.  step, start: the step loop's culls, the decisions at the start; zeta: -1 = the library's, 0 = pass cull off; entry,
    defer: 0 = that cull off alone.  at_start: Ray::init decided the ray; by_pass: ... and would not have with the pass cull off;
    marked: the start left the ray to the defer cull; defer_end: the defer cull ended it; entry_step: the attempted step at which the
    entry cull ended it (0: it did not); r_start, vr_start, r_last, vr_last: r and v^r at the start and after the last step."""
    from gradus_jl_amd.rendering import abi_pointfunction

    cfg, pl = config.abi_config(), config.abi_plane()
    s, keep = abi_pointfunction(pf)
    tiles = np.ascontiguousarray(tiles, dtype=np.int64)
    out = {k: np.zeros(tiles.size * 64, t) for k, t in OUT}
    o = hhc_out(*(v.ctypes.data for v in out.values()))
    rc = lib(defer_zeta).hhc_render_tiles(C.byref(cfg), C.byref(pl), C.byref(s), C.c_void_p(tiles.ctypes.data), C.c_int64(tiles.size),
                                          C.c_int(step), C.c_int(start), C.c_double(zeta), C.c_int(entry), C.c_int(defer), C.byref(o))
    assert rc == 0, rc
    return {k: v.reshape(tiles.size, 64) for k, v in out.items()}


def _bounds(fn, names, config, rays, zeta):
    cfg, pl = config.abi_config(), config.abi_plane()
    rays = np.ascontiguousarray(rays, dtype=np.int64)
    out = np.zeros((rays.size, len(names)))
    rc = fn(C.byref(cfg), C.byref(pl), C.c_void_p(rays.ctypes.data), C.c_int64(rays.size), C.c_double(zeta), C.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    return {k: out[:, i] for i, k in enumerate(names)}


def pass_bounds(config, rays, zeta=-1.0):
    """{name: array} over PASS_BOUNDS for the plane's rays `rays` (column-major indices, as the kernels number them)."""
    return _bounds(lib().hhc_pass_bounds, PASS_BOUNDS, config, rays, zeta)


def entry_bounds(config, rays, zeta=-1.0):
    """{name: array} over ENTRY_BOUNDS for the plane's rays `rays`, at the state in which Ray::step asks the entry cull ("asked" = 0:
    the ray never gets there, every entry is zero)."""
    return _bounds(lib().hhc_entry_bounds, ENTRY_BOUNDS, config, rays, zeta)


def _ratio(num, den):
    """num / den; 1.0 where den is 0: neither arm traced anything (every ray of the tiles was decided at the start)."""
    return num / den if den else 1.0


def census(G, config, pf, tiles, arms, base, ratios, zeta=-1.0, defer_zeta=None):
    """The arms of a mechanism (STEP, PASS, ENTRY or DEFER: `census(G, config, pf, tiles, *PASS)`) on the same tiles, each compared
    with its arm of `base`.  "wave_steps" is the sum over tiles of the longest lane's attempted steps (what a one-wave workgroup
    costs).  Of the rays an arm's base arm sees hit the disc (each must be 0): "wrongly_fired" counts those that took fewer steps
    than there, "wrongly_decided_by_pass" those the pass cull decided, "wrongly_ended_on_entry" those the entry cull ended,
    "wrongly_ended_early" those decided at the start, ended on entry or ended by the defer cull.  "decided_by_start_test" counts
    the decisions of the start cull's own test, "decided_at_start_any" those and the pass cull's."""
    runs = {arm: render_tiles(G, config, pf, tiles, step, start, entry, defer, zeta if z is None else z, defer_zeta)
            for arm, (step, start, entry, defer, z) in arms.items()}
    hit_code = int(G.StatusCodes.IntersectedWithGeometry)

    def base_of(arm):
        return runs[base if isinstance(base, str) else base[arm]]

    first = base_of(next(iter(arms)))
    res = {"tiles": int(len(tiles)), "rays": int(first["status"].size), "hit_fraction": float(np.mean(first["status"] == hit_code)), "arms": {}}
    for arm, r in runs.items():
        b = base_of(arm)
        hit = b["status"] == hit_code
        att = r["nacc"].astype(np.int64) + r["nrej"]
        fired = att < (b["nacc"].astype(np.int64) + b["nrej"])
        ended = r["entry_step"] > 0
        early = (r["at_start"] == 1) | (r["defer_end"] == 1) | ended
        res["arms"][arm] = {
            "same_image": r["image"].tobytes() == b["image"].tobytes(),
            "same_status": bool(np.array_equal(r["status"], b["status"])),
            "flagged": int(np.sum(r["status"] < 0)),
            "accepted_steps": int(r["nacc"].sum()),
            "attempted_steps": int(att.sum()),
            "wave_steps": int(att.max(axis=1).sum()),
            "lane_utilisation": float(att.sum() / (64.0 * max(int(att.max(axis=1).sum()), 1))),
            "fired": int(fired.sum()),
            "decided_at_start_any": int(r["at_start"].sum()),
            "decided_by_start_test": int(np.sum(r["at_start"] - r["by_pass"])),
            "decided_by_pass_cull": int(r["by_pass"].sum()),
            "marked_for_defer": int(r["marked"].sum()),
            "ended_by_defer": int(r["defer_end"].sum()),
            "ended_on_entry": int(ended.sum()),
            "entry_step_range": [int(r["entry_step"][ended].min()), int(r["entry_step"][ended].max())] if ended.any() else None,
            "whole_tiles_decided": int(np.sum(att.max(axis=1) == 0)),
            "wrongly_fired": int(np.sum(fired & hit)),
            "wrongly_decided_by_pass": int(np.sum((r["by_pass"] == 1) & hit)),
            "wrongly_ended_on_entry": int(np.sum(ended & hit)),
            "wrongly_ended_early": int(np.sum(early & hit)),
        }
    a = res["arms"]

    def ratio(spec):
        if isinstance(spec, dict):
            return {k: ratio(v) for k, v in spec.items()}
        key, num, den = spec
        return _ratio(a[num][key], a[den][key])

    res.update({name: ratio(spec) for name, spec in ratios.items()})
    return res, runs
