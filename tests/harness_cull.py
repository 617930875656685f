"""ctypes binding of tests/host_harness_cull.cpp: whole 8 x 8 tiles of an image plane traced by the HIP integrator compiled for
the host (g++), with the start cull and the step loop's culls switched one by one."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "libhost_harness_cull.so")
SRC = [os.path.join(HERE, "host_harness_cull.cpp"), os.path.join(ROOT, "gradus.jl_amd", "csrc", "gr_device.hpp"),
       os.path.join(ROOT, "include", "gradus_mi355x.h"), os.path.join(ROOT, "gradus.jl_amd", "csrc", "gr_tabmetric.hpp")]
ARMS = {"off": (0, 0), "start": (0, 1), "step": (1, 0), "both": (1, 1)}      # name -> (step-loop culls, start cull)
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in SRC):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, SRC[0]])
        _lib = C.CDLL(SO)
        _lib.hhc_gate_radius.restype = C.c_double
    return _lib


def gate_radius(config):
    cfg = config.abi_config()
    return float(lib().hhc_gate_radius(C.byref(cfg)))


def render_tiles(G, config, pf, tiles, arm):
    """{image, status, nacc, nrej, at_start}, each (len(tiles), 64): lane l of a tile is its column l // 8, row l % 8."""
    from gradus_jl_amd.rendering import abi_pointfunction

    cfg, pl = config.abi_config(), config.abi_plane()
    s, keep = abi_pointfunction(pf)
    tiles = np.ascontiguousarray(tiles, dtype=np.int64)
    n = tiles.size * 64
    out = {"image": np.zeros(n), "status": np.zeros(n, np.int32), "nacc": np.zeros(n, np.int32), "nrej": np.zeros(n, np.int32),
           "at_start": np.zeros(n, np.int32)}
    step, start = ARMS[arm]
    rc = lib().hhc_render_tiles(C.byref(cfg), C.byref(pl), C.byref(s), C.c_void_p(tiles.ctypes.data), C.c_int64(tiles.size),
                                C.c_int(step), C.c_int(start), *(C.c_void_p(out[k].ctypes.data)
                                                                for k in ("image", "status", "nacc", "nrej", "at_start")))
    assert rc == 0, rc
    return {k: v.reshape(tiles.size, 64) for k, v in out.items()}


def _ratio(num, den):
    """num / den; 1.0 where den is 0: neither arm traced anything (every ray of the tiles was decided at the start)."""
    return num / den if den else 1.0


def census(G, config, pf, tiles):
    """All four arms on the same tiles, and what the culls are judged by.  "wave_steps" is the sum over tiles of the longest lane's
    attempted steps (what a one-wave workgroup costs); "wrongly_decided" counts rays an arm ended early although the full trace
    hits the disc."""
    runs = {arm: render_tiles(G, config, pf, tiles, arm) for arm in ARMS}
    off = runs["off"]
    hit = off["status"] == int(G.StatusCodes.IntersectedWithGeometry)
    res = {"tiles": int(len(tiles)), "rays": int(off["status"].size), "hit_fraction": float(hit.mean()), "arms": {}}
    for arm, r in runs.items():
        att = r["nacc"].astype(np.int64) + r["nrej"]
        fired = att < (off["nacc"].astype(np.int64) + off["nrej"])
        res["arms"][arm] = {
            "same_image": r["image"].tobytes() == off["image"].tobytes(),
            "same_status": bool(np.array_equal(r["status"], off["status"])),
            "flagged": int(np.sum(r["status"] < 0)),
            "accepted_steps": int(r["nacc"].sum()),
            "wave_steps": int(att.max(axis=1).sum()),
            "lane_utilisation": float(att.sum() / (64.0 * max(int(att.max(axis=1).sum()), 1))),
            "fired": int(fired.sum()),
            "decided_at_start": int(r["at_start"].sum()),
            "wrongly_decided": int(np.sum(fired & hit)),
        }
    a = res["arms"]
    res["wave_steps_ratio_vs_escape_cull_alone"] = {k: _ratio(a[k]["wave_steps"], a["step"]["wave_steps"]) for k in ("both",)}
    res["wave_steps_ratio_vs_off"] = {k: _ratio(a[k]["wave_steps"], a["off"]["wave_steps"]) for k in ("start", "step", "both")}
    # what tests/test_gpu_escape_cull.py brackets: accepted steps with GRADUS_MI355X_ESCAPE_CULL unset over =0 (start cull on in both)
    res["escape_switch_bracket_ratio"] = _ratio(a["both"]["accepted_steps"], a["start"]["accepted_steps"])
    return res, runs
