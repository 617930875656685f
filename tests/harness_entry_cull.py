"""ctypes binding of tests/host_harness_entry_cull.cpp: whole 8 x 8 tiles of an image plane traced by the HIP integrator compiled
for the host (g++) with the step loop's culls, the decisions at the start and the entry cull (Ray::step) switched
one by one, the rays the entry cull ended and the step at which it did, and the bounds it decides by, ray by ray."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "libhost_harness_entry_cull.so")
SRC = [os.path.join(HERE, "host_harness_entry_cull.cpp"), os.path.join(ROOT, "gradus.jl_amd", "csrc", "gr_device.hpp"),
       os.path.join(ROOT, "include", "gradus_mi355x.h"), os.path.join(ROOT, "gradus.jl_amd", "csrc", "gr_tabmetric.hpp")]
# name -> (step-loop culls, decisions at the start, entry cull).  "start" is the GRADUS_MI355X_ESCAPE_CULL=0 arm of the library,
# "all" the library as shipped, "no-entry" GRADUS_MI355X_ENTRY_CULL=0.
ARMS = {"start": (0, 1, 1), "no-entry": (1, 1, 0), "all": (1, 1, 1)}
BOUNDS = ("E", "L", "Q", "u0", "uc", "mu0", "mu_rising", "vr", "u_lo", "u_hi", "Ta_lo", "Tb_hi", "Om_lo", "Om_hi", "psi0", "decided",
          "asked", "steps")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in SRC):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, SRC[0]])
        _lib = C.CDLL(SO)
        _lib.hhe_gate_radius.restype = C.c_double
        _lib.hhe_zeta.restype = C.c_double
        _lib.hhe_zeta_dip.restype = C.c_double
    return _lib


def gate_radius(config):
    cfg = config.abi_config()
    return float(lib().hhe_gate_radius(C.byref(cfg)))


def zeta():
    """The library's ζ (kPassCullZeta): R_pass = ζ R_cull."""
    return float(lib().hhe_zeta())


def zeta_dip():
    """The entry cull's depth limit (kEntryCullZeta): R_dip = ζ_dip R_cull."""
    return float(lib().hhe_zeta_dip())


def default_entry_cull():
    """Params::entry_cull as memset + derive_params leave it (how the older harnesses fill Params)."""
    return int(lib().hhe_default_entry_cull())


def render_tiles(G, config, pf, tiles, step, start, entry, zeta=-1.0):
    """{image, status, nacc, nrej, at_start, entry_step, r_last, vr_last, r_start}, each (len(tiles), 64): lane l of a tile is its
    column l // 8, row l % 8.  zeta: -1 = the library's, 0 = pass cull off.  entry_step: the attempted step at which the entry cull
    ended the ray (0: it did not)."""
    from gradus_jl_amd.rendering import abi_pointfunction

    cfg, pl = config.abi_config(), config.abi_plane()
    s, keep = abi_pointfunction(pf)
    tiles = np.ascontiguousarray(tiles, dtype=np.int64)
    n = tiles.size * 64
    out = {"image": np.zeros(n), "status": np.zeros(n, np.int32), "nacc": np.zeros(n, np.int32), "nrej": np.zeros(n, np.int32),
           "at_start": np.zeros(n, np.int32), "entry_step": np.zeros(n, np.int32), "r_last": np.zeros(n), "vr_last": np.zeros(n),
           "r_start": np.zeros(n)}
    rc = lib().hhe_render_tiles(C.byref(cfg), C.byref(pl), C.byref(s), C.c_void_p(tiles.ctypes.data), C.c_int64(tiles.size),
                                C.c_int(step), C.c_int(start), C.c_double(zeta), C.c_int(entry),
                                *(C.c_void_p(v.ctypes.data) for v in out.values()))
    assert rc == 0, rc
    return {k: v.reshape(tiles.size, 64) for k, v in out.items()}


def entry_bounds(config, rays, zeta=-1.0):
    """{name: array} over BOUNDS for the plane's rays `rays` (column-major indices, as the kernels number them), at the state in
    which Ray::step asks the entry cull ("asked" = 0: the ray never gets there, every entry is zero)."""
    cfg, pl = config.abi_config(), config.abi_plane()
    rays = np.ascontiguousarray(rays, dtype=np.int64)
    out = np.zeros((rays.size, len(BOUNDS)))
    rc = lib().hhe_entry_bounds(C.byref(cfg), C.byref(pl), C.c_void_p(rays.ctypes.data), C.c_int64(rays.size), C.c_double(zeta),
                                C.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    return {k: out[:, i] for i, k in enumerate(BOUNDS)}


def _ratio(num, den):
    """num / den; 1.0 where den is 0: neither arm traced anything (every ray of the tiles was decided at the start)."""
    return num / den if den else 1.0


def census(G, config, pf, tiles, zeta=-1.0):
    """The arms of ARMS on the same tiles.  "wave_steps" is the sum over tiles of the longest lane's attempted steps (what a
    one-wave workgroup costs); "wrongly_ended" counts rays the entry cull ended although the arm without it hits the disc.
    Every arm is compared with "no-entry"."""
    runs = {arm: render_tiles(G, config, pf, tiles, step, start, entry, zeta) for arm, (step, start, entry) in ARMS.items()}
    hit_code = int(G.StatusCodes.IntersectedWithGeometry)
    base = runs["no-entry"]
    res = {"tiles": int(len(tiles)), "rays": int(base["status"].size), "arms": {}}
    for arm, r in runs.items():
        att = r["nacc"].astype(np.int64) + r["nrej"]
        ended = r["entry_step"] > 0
        res["arms"][arm] = {
            "same_image": r["image"].tobytes() == base["image"].tobytes(),
            "same_status": bool(np.array_equal(r["status"], base["status"])),
            "flagged": int(np.sum(r["status"] < 0)),
            "accepted_steps": int(r["nacc"].sum()),
            "wave_steps": int(att.max(axis=1).sum()),
            "lane_utilisation": float(att.sum() / (64.0 * max(int(att.max(axis=1).sum()), 1))),
            "decided_at_start": int(np.sum(r["at_start"] == 1)),
            "ended_on_entry": int(ended.sum()),
            "entry_step_range": [int(r["entry_step"][ended].min()), int(r["entry_step"][ended].max())] if ended.any() else None,
            "whole_tiles_decided": int(np.sum(att.max(axis=1) == 0)),
            "wrongly_ended": int(np.sum(ended & (base["status"] == hit_code))),
        }
    a = res["arms"]
    res["hit_fraction"] = float(np.mean(base["status"] == hit_code))
    # the launch: the entry cull on against off, every other cull on
    res["entry_wave_steps_ratio"] = _ratio(a["all"]["wave_steps"], a["no-entry"]["wave_steps"])
    res["entry_accepted_steps_ratio"] = _ratio(a["all"]["accepted_steps"], a["no-entry"]["accepted_steps"])
    # what tests/test_gpu_escape_cull.py brackets: accepted steps with GRADUS_MI355X_ESCAPE_CULL unset over =0, the decisions at
    # the start on in both arms
    res["escape_switch_bracket_ratio"] = _ratio(a["all"]["accepted_steps"], a["start"]["accepted_steps"])
    return res, runs
