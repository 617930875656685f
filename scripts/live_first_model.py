#!/usr/bin/env python3
"""CPU model of the bench launch's schedule: what the order of its tiles is worth (DESIGN_measurements.md §M30).

1. CENSUS.  Every 8 x 8 tile of the 2048² bench image (Kerr a = 0.998, observer r = 1000, θ = 75°, ThinDisc(isco, 50), λ1 = 2000)
   is stepped through the KERNEL's own logic compiled for the host (tests/host_harness_culls.cpp, every cull on as shipped):
   per tile the attempted steps of its longest lane (what a one-wave workgroup runs: its wave-steps), the steps of all lanes, the
   step of the last lane that ends as a hit, and three candidate flags for the tile: its four corner rays are all decided at the
   start -- the flag k_tile_classify writes (gr_tile_order.hpp) --, one inner ray (lane 27) is, and the corners with a margin:
   the sixteen rays of the 4 x 4 lattice through the corners and one tile side beyond them are.  Printed: live and dead
   waves, wave-steps, lane utilisation, steps per ray, the share of wave-steps up to the last hit lane, how each flag compares
   with the tile (dead tiles it calls live and live tiles it calls dead), and where the dead tiles sit in the queue.
2. SLOTS.  An event simulation of the launch: 1024 SIMDs of 3 wave slots (3072 slots); workgroups leave a FIFO queue in tile
   order, the first 3072 dealt round-robin, each later one to the slot that falls free; a wave holds its slot for a latency of
   10 µs before it issues anything, then shares its SIMD's issue rate (0.96 instructions per 4 clocks at 2.22 GHz) equally with the
   other issuing waves of the SIMD; a wave that issues alone runs at half that rate (one wave cannot cover its own dependent
   chains).  A wave's work is an instruction count: DEAD for a wave without a step, LIVE + PER_STEP x wave-steps otherwise, with
   PER_STEP set so that the launch's total is the VALU count of the head profile (SQ_INSTS_VALU x waves, profiles/CURRENT).
   Printed: the launch in tile order, with the live tiles first and the dead last (by the census and by each of the three flags), and the floor (all work at the full rate on every SIMD).

These are model figures: nothing here runs on a device.  CPU only; the census takes a few minutes on eight cores and is kept in
--cache (an .npz) for the next run.

    python scripts/live_first_model.py [--size 2048] [--procs 8] [--cache census.npz]
"""
from __future__ import annotations

import argparse
import heapq
import json
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CORNER_LANES = (0, 7, 56, 63)      # gr_order::class_lane(3, k): the corners of an 8 x 8 tile
INNER_LANE = 27                    # one inner ray instead: the alternative the model rules out
SIMDS, SLOTS_PER_SIMD = 1024, 3    # 256 CUs x 4 SIMDs, three waves of the head kernel per SIMD (168 VGPRs)
CLOCK_GHZ, ISSUE = 2.22, 0.96      # profiles/r13_head_summary.json: clock under load; M14: issue rate of a full 2048² launch
LATENCY_US = 10.0                  # a wave's slot-holding time before its first instruction (M26: a dead wave lives 14-17 µs)
DEAD_INSTS, LIVE_INSTS = 300.0, 2500.0      # M26: instructions of a wave outside its steps


def _chunk(args):
    size, tiles = args
    import gradus_jl_amd as G
    import harness_culls as H
    from cull_scenes import bench_scene

    cfg, pf = bench_scene(G, size)
    r = H.render_tiles(G, cfg, pf, tiles)
    att = r["nacc"].astype(np.int64) + r["nrej"]
    hit = r["status"] == int(G.StatusCodes.IntersectedWithGeometry)
    return (tiles, att.max(axis=1), att.sum(axis=1), r["nacc"].sum(axis=1), np.where(hit, att, 0).max(axis=1),
            (r["at_start"][:, CORNER_LANES] << np.arange(4)).sum(axis=1).astype(np.uint8), r["at_start"][:, INNER_LANE].astype(np.uint8), hit.sum(axis=1))


def census(size, procs):
    import harness_culls as H

    H.lib()      # build the harness once, before the workers load it
    nt = (size // 8) ** 2
    chunks = [(size, np.arange(a, min(a + 512, nt), dtype=np.int64)) for a in range(0, nt, 512)]
    out = {k: np.zeros(nt, np.int64) for k in ("wave_steps", "lane_steps", "accepted", "hit_steps", "corners", "flag_inner", "hits")}
    with mp.Pool(procs) as pool:
        for tiles, ws, ls, acc, hs, corners, inner, hits in pool.imap_unordered(_chunk, chunks):
            for k, v in zip(out, (ws, ls, acc, hs, corners, inner, hits)):
                out[k][tiles] = v
    return out


def lattice_flag(corners, size):
    """The corners' flag with a margin of one tile, from the tiles' corner bits (bit k = corner lane CORNER_LANES[k] is decided at the start): lattice
    column a of a tile is the first column of the tile before it, its own first, its own last, the last of the tile after it
    (clamped at the image's edges), rows alike."""
    nt = size // 8
    c = corners.reshape(nt, nt)          # [tile column, tile row]: tiles count down the columns
    bit = {(0, 0): 0, (0, 1): 1, (1, 0): 2, (1, 1): 3}      # (last column?, last row?) -> bit
    flag = np.ones((nt, nt), dtype=bool)
    idx = np.arange(nt)
    for da, ca in ((-1, 0), (0, 0), (0, 1), (1, 1)):
        tx = np.clip(idx + da, 0, nt - 1)
        for db, rb in ((-1, 0), (0, 0), (0, 1), (1, 1)):
            ty = np.clip(idx + db, 0, nt - 1)
            flag &= ((c[np.ix_(tx, ty)] >> bit[(ca, rb)]) & 1).astype(bool)
    return flag.reshape(-1)


def simulate(order, work, simds=SIMDS, slots=SLOTS_PER_SIMD):
    """Launch time in µs of the waves `order` (indices into `work`, instruction counts) through the slot model."""
    rate = CLOCK_GHZ * 1e3 / 4.0 * ISSUE      # instructions per µs of one SIMD
    n = len(order)
    res = [[] for _ in range(simds)]          # per SIMD: [latency left, work left] per resident wave
    last = [0.0] * simds                      # the time each SIMD's state is valid for
    ver = [0] * simds
    heap = []

    def advance(s, now):
        dt = now - last[s]
        if dt > 0.0:
            issuing = [w for w in res[s] if w[0] <= 0.0]
            share = (rate * 0.5) if len(issuing) == 1 else (rate / len(issuing) if issuing else 0.0)
            for w in res[s]:
                if w[0] > 0.0:
                    w[0] -= dt
                else:
                    w[1] -= share * dt
        last[s] = now

    def schedule(s):
        ver[s] += 1
        if not res[s]:
            return
        issuing = sum(1 for w in res[s] if w[0] <= 1e-12)
        share = (rate * 0.5) if issuing == 1 else (rate / issuing if issuing else 0.0)
        nxt = min((w[0] if w[0] > 1e-12 else max(w[1], 0.0) / share) for w in res[s])
        heapq.heappush(heap, (last[s] + nxt, s, ver[s]))

    head = 0
    for k in range(min(n, simds * slots)):
        res[k % simds].append([LATENCY_US, float(work[order[k]])])
        head += 1
    for s in range(simds):
        schedule(s)
    now = 0.0
    while heap:
        t, s, v = heapq.heappop(heap)
        if v != ver[s]:
            continue
        now = t
        advance(s, now)
        for w in res[s]:
            if 0.0 < w[0] <= 1e-9:
                w[0] = 0.0
        done = [w for w in res[s] if w[0] <= 0.0 and w[1] <= 1e-6]
        for w in done:
            res[s].remove(w)
            if head < n:
                res[s].append([LATENCY_US, float(work[order[head]])])
                head += 1
        schedule(s)
    return now


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--cache", default=None, help="an .npz that keeps the census (read if it exists, written if not)")
    a = ap.parse_args()
    if a.cache and os.path.exists(a.cache):
        c = dict(np.load(a.cache))
    else:
        c = census(a.size, a.procs)
        if a.cache:
            np.savez_compressed(a.cache, **c)
    nt = c["wave_steps"].size
    live = c["wave_steps"] > 0
    ws = int(c["wave_steps"].sum())
    res = {"tiles": int(nt), "live_waves": int(live.sum()), "dead_waves": int((~live).sum()), "wave_steps": ws,
           "wave_steps_per_live_wave": ws / max(int(live.sum()), 1),
           "lane_utilisation_in_the_loop": float(c["lane_steps"].sum() / (64.0 * ws)),
           "steps_per_ray": float(c["lane_steps"].sum() / (64.0 * nt)),          # accepted + rejected, as bench.py counts them
           "accepted_steps_per_ray": float(c["accepted"].sum() / (64.0 * nt)),
           "share_of_wave_steps_up_to_the_last_hit_lane": float(c["hit_steps"].sum() / ws)}
    flag, four, inner = lattice_flag(c["corners"], a.size), c["corners"] == 15, c["flag_inner"] != 0
    for name, f in (("corners", four), ("inner_ray", inner), ("corners_and_margin", flag)):
        res["flag_by_" + name] = {"flag_dead": int(f.sum()), "dead_tiles_called_live": int((~live & ~f).sum()),
                                  "live_tiles_called_dead": int((live & f).sum()),
                                  "wave_steps_of_live_tiles_called_dead": int(c["wave_steps"][live & f].sum())}
    first_live, last_live = int(np.flatnonzero(live)[0]), int(np.flatnonzero(live)[-1])
    res["dead_tiles_before_the_first_live_tile"] = first_live
    res["dead_tiles_after_the_last_live_tile"] = int(nt - 1 - last_live)
    # the work of a wave in instructions: the launch's total is the profile's VALU count
    valu_total = None
    try:
        cur = json.load(open(os.path.join(ROOT, "profiles", "CURRENT")))
        head = json.load(open(os.path.join(ROOT, cur["head"])))
        if a.size == 2048:
            valu_total = float(head["counters"]["SQ_INSTS_VALU"])
    except (OSError, KeyError, ValueError):
        pass
    per_step = 965.0 if valu_total is None else (valu_total - DEAD_INSTS * res["dead_waves"] - LIVE_INSTS * res["live_waves"]) / ws
    work = np.where(live, LIVE_INSTS + per_step * c["wave_steps"], DEAD_INSTS)
    rate = CLOCK_GHZ * 1e3 / 4.0 * ISSUE
    tile = np.arange(nt)
    orders = {"tile_order": tile,
              "live_first_by_census": np.concatenate([tile[live], tile[~live]]),
              "live_first_by_corners": np.concatenate([tile[~four], tile[four]]),
              "live_first_by_corners_and_margin": np.concatenate([tile[~flag], tile[flag]]),
              "live_first_by_inner_ray": np.concatenate([tile[~inner], tile[inner]])}
    res["model"] = {"slots": SIMDS * SLOTS_PER_SIMD, "instructions_per_wave_step": per_step, "latency_us": LATENCY_US,
                    "floor_us": float(work.sum() / (SIMDS * rate))}
    for name, order in orders.items():
        res["model"][name + "_us"] = simulate(order, work)
    t0 = res["model"]["tile_order_us"]
    for name in ("live_first_by_census", "live_first_by_corners", "live_first_by_corners_and_margin", "live_first_by_inner_ray"):
        res["model"][name + "_gain"] = 1.0 - res["model"][name + "_us"] / t0
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
