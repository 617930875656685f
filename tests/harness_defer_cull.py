"""ctypes binding of tests/host_harness_defer_cull.cpp: whole 8 x 8 tiles of an image plane traced by the HIP integrator compiled
for the host (g++) with the step loop's culls, the decisions at the start, the entry cull and the defer cull (Ray::start_decided,
Ray::step) switched one by one; the rays the start marked for the defer cull, the rays it ended and the rays the
entry cull ended."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = [os.path.join(HERE, "host_harness_defer_cull.cpp"), os.path.join(ROOT, "gradus.jl_amd", "csrc", "gr_device.hpp"),
       os.path.join(ROOT, "include", "gradus_mi355x.h"), os.path.join(ROOT, "gradus.jl_amd", "csrc", "gr_tabmetric.hpp")]
# name -> (step-loop culls, decisions at the start, entry cull, defer cull, zeta).  "all" is the library as shipped, "no-defer"
# GRADUS_MI355X_DEFER_CULL=0, "start" GRADUS_MI355X_ESCAPE_CULL=0, "full" every cull off.  zeta None = the caller's.
ARMS = {"all": (1, 1, 1, 1, None), "no-defer": (1, 1, 1, 0, None), "start": (0, 1, 1, 1, None), "full": (0, 0, 0, 0, 0.0)}
_libs = {}


def lib(defer_zeta=None):
    """The harness with the library's kDeferCullZeta, or (the census) built with another one."""
    key = None if defer_zeta is None else float(defer_zeta)
    if key not in _libs:
        so = os.path.join(HERE, "libhost_harness_defer_cull.so" if key is None else f"libhost_harness_defer_cull_{key:.4f}.so")
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SRC):
            extra = [] if key is None else [f"-DGR_DEFER_CULL_ZETA={key!r}"]
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", *extra, "-o", so, SRC[0]])
        L = C.CDLL(so)
        for f in ("hhd_gate_radius", "hhd_zeta", "hhd_zeta_dip", "hhd_zeta_defer"):
            getattr(L, f).restype = C.c_double
        _libs[key] = L
    return _libs[key]


def gate_radius(config):
    cfg = config.abi_config()
    return float(lib().hhd_gate_radius(C.byref(cfg)))


def zeta():
    """The library's ζ (kPassCullZeta): R_pass = ζ R_cull."""
    return float(lib().hhd_zeta())


def zeta_dip():
    """The entry cull's depth limit (kEntryCullZeta)."""
    return float(lib().hhd_zeta_dip())


def zeta_defer(defer_zeta=None):
    """The defer cull's depth limit (kDeferCullZeta): R_defer = ζ_defer R_cull."""
    return float(lib(defer_zeta).hhd_zeta_defer())


def default_defer_cull():
    """Params::defer_cull as memset + derive_params leave it (how the older harnesses fill Params)."""
    return int(lib().hhd_default_defer_cull())


def render_tiles(G, config, pf, tiles, step, start, entry, defer, zeta=-1.0, defer_zeta=None):
    """{image, status, nacc, nrej, at_start, marked, defer_end, entry_step, r_start, vr_start}, each (len(tiles), 64): lane l of a
    tile is its column l // 8, row l % 8.  zeta: -1 = the library's, 0 = pass cull off.  marked: the start left the ray to the
    defer cull; defer_end: the defer cull ended it; entry_step: the attempted step at which the entry cull ended it (0: not)."""
    from gradus_jl_amd.rendering import abi_pointfunction

    cfg, pl = config.abi_config(), config.abi_plane()
    s, keep = abi_pointfunction(pf)
    tiles = np.ascontiguousarray(tiles, dtype=np.int64)
    n = tiles.size * 64
    out = {"image": np.zeros(n), "status": np.zeros(n, np.int32), "nacc": np.zeros(n, np.int32), "nrej": np.zeros(n, np.int32),
           "at_start": np.zeros(n, np.int32), "marked": np.zeros(n, np.int32), "defer_end": np.zeros(n, np.int32),
           "entry_step": np.zeros(n, np.int32), "r_start": np.zeros(n), "vr_start": np.zeros(n)}
    rc = lib(defer_zeta).hhd_render_tiles(C.byref(cfg), C.byref(pl), C.byref(s), C.c_void_p(tiles.ctypes.data), C.c_int64(tiles.size),
                                          C.c_int(step), C.c_int(start), C.c_double(zeta), C.c_int(entry), C.c_int(defer),
                                          *(C.c_void_p(v.ctypes.data) for v in out.values()))
    assert rc == 0, rc
    return {k: v.reshape(tiles.size, 64) for k, v in out.items()}


def _ratio(num, den):
    """num / den; 1.0 where den is 0: neither arm traced anything (every ray of the tiles was decided at the start)."""
    return num / den if den else 1.0


def census(G, config, pf, tiles, zeta=-1.0, defer_zeta=None):
    """The arms of ARMS on the same tiles.  "wave_steps" is the sum over tiles of the longest lane's attempted steps (what a
    one-wave workgroup costs); "wrongly_ended" counts rays an arm ended early (at the start, on entry or by the defer cull)
    although the full trace hits the disc.  Every arm is compared with "full"."""
    runs = {arm: render_tiles(G, config, pf, tiles, step, start, entry, defer, zeta if z is None else z, defer_zeta)
            for arm, (step, start, entry, defer, z) in ARMS.items()}
    hit_code = int(G.StatusCodes.IntersectedWithGeometry)
    base = runs["full"]
    res = {"tiles": int(len(tiles)), "rays": int(base["status"].size), "arms": {}}
    for arm, r in runs.items():
        att = r["nacc"].astype(np.int64) + r["nrej"]
        early = (r["at_start"] == 1) | (r["defer_end"] == 1) | (r["entry_step"] > 0)
        res["arms"][arm] = {
            "same_image": r["image"].tobytes() == base["image"].tobytes(),
            "same_status": bool(np.array_equal(r["status"], base["status"])),
            "flagged": int(np.sum(r["status"] < 0)),
            "accepted_steps": int(r["nacc"].sum()),
            "attempted_steps": int(att.sum()),
            "wave_steps": int(att.max(axis=1).sum()),
            "lane_utilisation": float(att.sum() / (64.0 * max(int(att.max(axis=1).sum()), 1))),
            "decided_at_start": int(np.sum(r["at_start"] == 1)),
            "marked_for_defer": int(r["marked"].sum()),
            "ended_by_defer": int(r["defer_end"].sum()),
            "ended_on_entry": int(np.sum(r["entry_step"] > 0)),
            "wrongly_ended": int(np.sum(early & (base["status"] == hit_code))),
        }
    a = res["arms"]
    res["hit_fraction"] = float(np.mean(base["status"] == hit_code))
    # the launch: the defer cull on against off, every other cull on
    res["defer_wave_steps_ratio"] = _ratio(a["all"]["wave_steps"], a["no-defer"]["wave_steps"])
    res["defer_accepted_steps_ratio"] = _ratio(a["all"]["accepted_steps"], a["no-defer"]["accepted_steps"])
    # what tests/test_gpu_escape_cull.py brackets: accepted steps with GRADUS_MI355X_ESCAPE_CULL unset over =0
    res["escape_switch_bracket_ratio"] = _ratio(a["all"]["accepted_steps"], a["start"]["accepted_steps"])
    return res, runs
