"""ctypes binding of tests/host_harness_pass_cull.cpp: whole 8 x 8 tiles of an image plane traced by the HIP integrator compiled
for the host (g++) with the step loop's culls, the start cull and the pass cull switched one by one, and the
bounds the pass cull decides by, ray by ray."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "libhost_harness_pass_cull.so")
SRC = [os.path.join(HERE, "host_harness_pass_cull.cpp"), os.path.join(ROOT, "gradus.jl_amd", "csrc", "gr_device.hpp"),
       os.path.join(ROOT, "include", "gradus_mi355x.h"), os.path.join(ROOT, "gradus.jl_amd", "csrc", "gr_tabmetric.hpp")]
# name -> (step-loop culls, start cull, pass cull); the pass cull is a test of the start cull and is off with it
ARMS = {"start": (0, 1, 0), "start+pass": (0, 1, 1), "both": (1, 1, 0), "both+pass": (1, 1, 1)}
BOUNDS = ("E", "L", "Q", "u0", "uc", "mu0", "mu_rising", "vr", "u_lo", "u_hi", "Ta_lo", "Tb_hi", "Om_lo", "Om_hi", "psi0", "decided")
# the bench scene at 64² and its variants chosen for where the signs and closed forms of the pass cull can go wrong: a wider wedge,
# a = 0 (Ω_lo = Ω_hi, the a -> 0 form of μ+), a retrograde hole, an observer nearer the axis, one below the plane (μ0 < 0)
ALIMS, BLIMS = (-60.0, 60.0), (-35.0, 35.0)
SCENES = {
    "bench64": dict(),
    "gtol0.1": dict(gtol=0.1),
    "a0": dict(a=0.0),
    "a-0.998": dict(a=-0.998),
    "theta30": dict(theta=30.0),
    "theta105": dict(theta=105.0),
}
_lib = None


def scene(G, a=0.998, theta=75.0, size=64, r_obs=1000.0, r_out=50.0, **kw):
    m = G.KerrMetric(1.0, a)
    x = np.array([0.0, r_obs, math.radians(theta), 0.0])
    cfg = G.render_configuration(m, x, G.ThinDisc(m.isco(), r_out), 2000.0, image_width=size, image_height=size,
                                 alpha_lims=ALIMS, beta_lims=BLIMS, **kw)
    pf = G.ConstPointFunctions.redshift(m, x) @ G.ConstPointFunctions.filter_intersected()
    return cfg, pf, a


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in SRC):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, SRC[0]])
        _lib = C.CDLL(SO)
        _lib.hhp_gate_radius.restype = C.c_double
        _lib.hhp_zeta.restype = C.c_double
    return _lib


def gate_radius(config):
    cfg = config.abi_config()
    return float(lib().hhp_gate_radius(C.byref(cfg)))


def zeta():
    """The library's ζ (kPassCullZeta): R_pass = ζ R_cull."""
    return float(lib().hhp_zeta())


def render_tiles(G, config, pf, tiles, step, start, zeta=-1.0):
    """{image, status, nacc, nrej, at_start}, each (len(tiles), 64): lane l of a tile is its column l // 8, row l % 8.
    zeta: -1 = the library's, 0 = pass cull off.  at_start: 0 traced, 1 the start cull's own test, 2 the pass cull."""
    from gradus_jl_amd.rendering import abi_pointfunction

    cfg, pl = config.abi_config(), config.abi_plane()
    s, keep = abi_pointfunction(pf)
    tiles = np.ascontiguousarray(tiles, dtype=np.int64)
    n = tiles.size * 64
    out = {"image": np.zeros(n), "status": np.zeros(n, np.int32), "nacc": np.zeros(n, np.int32), "nrej": np.zeros(n, np.int32),
           "at_start": np.zeros(n, np.int32)}
    rc = lib().hhp_render_tiles(C.byref(cfg), C.byref(pl), C.byref(s), C.c_void_p(tiles.ctypes.data), C.c_int64(tiles.size),
                                C.c_int(step), C.c_int(start), C.c_double(zeta),
                                *(C.c_void_p(out[k].ctypes.data) for k in ("image", "status", "nacc", "nrej", "at_start")))
    assert rc == 0, rc
    return {k: v.reshape(tiles.size, 64) for k, v in out.items()}


def pass_bounds(config, rays, zeta=-1.0):
    """{name: array} over BOUNDS for the plane's rays `rays` (column-major indices, as the kernels number them)."""
    cfg, pl = config.abi_config(), config.abi_plane()
    rays = np.ascontiguousarray(rays, dtype=np.int64)
    out = np.zeros((rays.size, 16))
    rc = lib().hhp_pass_bounds(C.byref(cfg), C.byref(pl), C.c_void_p(rays.ctypes.data), C.c_int64(rays.size), C.c_double(zeta),
                               C.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    return {k: out[:, i] for i, k in enumerate(BOUNDS)}


def _ratio(num, den):
    """num / den; 1.0 where den is 0: neither arm traced anything (every ray of the tiles was decided at the start)."""
    return num / den if den else 1.0


def census(G, config, pf, tiles, zeta=-1.0):
    """The four arms of ARMS on the same tiles.  "wave_steps" is the sum over tiles of the longest lane's attempted steps (what a
    one-wave workgroup costs); "wrongly_decided" counts rays the pass cull decided although the arm without it hits the disc.
    The pass arms are compared with the same arm without the pass cull."""
    runs = {arm: render_tiles(G, config, pf, tiles, step, start, zeta if on else 0.0) for arm, (step, start, on) in ARMS.items()}
    hit_code = int(G.StatusCodes.IntersectedWithGeometry)
    res = {"tiles": int(len(tiles)), "rays": int(runs["start"]["status"].size), "arms": {}}
    for arm, r in runs.items():
        base = runs[arm.replace("+pass", "")]
        att = r["nacc"].astype(np.int64) + r["nrej"]
        by_pass = r["at_start"] == 2
        res["arms"][arm] = {
            "same_image": r["image"].tobytes() == base["image"].tobytes(),
            "same_status": bool(np.array_equal(r["status"], base["status"])),
            "flagged": int(np.sum(r["status"] < 0)),
            "accepted_steps": int(r["nacc"].sum()),
            "wave_steps": int(att.max(axis=1).sum()),
            "lane_utilisation": float(att.sum() / (64.0 * max(int(att.max(axis=1).sum()), 1))),
            "decided_at_start": int(np.sum(r["at_start"] == 1)),
            "decided_by_pass_cull": int(by_pass.sum()),
            "whole_tiles_decided": int(np.sum(att.max(axis=1) == 0)),
            "wrongly_decided": int(np.sum(by_pass & (base["status"] == hit_code))),
        }
    a = res["arms"]
    res["hit_fraction"] = float(np.mean(runs["start"]["status"] == hit_code))
    # the launch: the pass cull on against off, every other cull on
    res["pass_wave_steps_ratio"] = _ratio(a["both+pass"]["wave_steps"], a["both"]["wave_steps"])
    res["pass_accepted_steps_ratio"] = _ratio(a["both+pass"]["accepted_steps"], a["both"]["accepted_steps"])
    # what tests/test_gpu_escape_cull.py brackets: accepted steps with GRADUS_MI355X_ESCAPE_CULL unset over =0, the decisions at
    # the start on in both arms
    res["escape_switch_bracket_ratio"] = _ratio(a["both+pass"]["accepted_steps"], a["start+pass"]["accepted_steps"])
    res["escape_switch_bracket_ratio_pass_off"] = _ratio(a["both"]["accepted_steps"], a["start"]["accepted_steps"])
    return res, runs
