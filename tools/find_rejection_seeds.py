#!/usr/bin/env python3
"""Directed seeds for the Lemire rejection branch: scan seeds 0, 1, 2, ... through the CPU oracle's
rejection trace and write tests/golden/lemire_rejections.json.

A bounded draw integers(0, n) takes a 32-bit half r of the stream, m = r * n, left = m mod 2^32; it
is rejected (one more half taken) when left < 2^32 mod n, which needs left < n first.  With the
traffic resets' n <= 470 (the squares of a 25-tile map) that is a few draws in 10^8, so no small test meets one by luck.  This tool
finds the seeds whose reset (step 0) or idle step (action 4, step t >= 1) contains such a draw, per
site (oracle.SITES): Floyd's and the shuffle's draws of choice(np, k, replace=False), the initial
per-car route draws, the car pass, the map generator.  It uses the oracle only; the fixture holds
seeds and the oracle's own results (np, k, the trace records, the crc32 of the car list).

Usage: python tools/find_rejection_seeds.py [--budget 10000000] [--step-budget 1000000]
           [--workers N (<= 16)] [--configs cfg3,dense5x5,tall_map,wide_map] [--out PATH]
Selection is in seed order over fixed-size blocks, so the result does not depend on the worker count.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import multiprocessing as mp
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    "cfg3": dict(random_map_width=5, random_map_height=5, traffic_density=0.5),  # the bench shape
    "dense5x5": dict(random_map_width=5, random_map_height=5, traffic_density=1.0),
    "tall_map": dict(random_map_width=2, random_map_height=9, traffic_density=0.5),
    "wide_map": dict(random_map_width=9, random_map_height=2, traffic_density=0.5),
}
GROUPS = (16, 12, 8, 4, 3, 2)  # lanes per env of the device's initial-traffic kernel
# (site quota name) -> entries wanted per configuration
QUOTA = {"floyd": 6, "shuffle": 3, "init_route": 2, "car_pass": 3}
QUOTA_CFG3 = ("stretch_first", "stretch_last", "stretch_start", "wide_first", "wide_last")  # one each (see stretch_tags)
WIDE = (16, 12)  # the groups whose first / last stretch is a small part of the draws
EXTRA_CAP = {"double": 2, "mapgen": 2}  # kept as they turn up, no quota
IDLE_STEPS = 60
BLOCK = 20000       # seeds per work item (resets)
STEP_BLOCK = 2000   # seeds per work item (60 idle steps each)
OUT = os.path.join(ROOT, "tests", "golden", "lemire_rejections.json")


def stretch_tags(d: int, k: int) -> list[str]:
    """Where draw d of the D = 2k-1 draws of choice(np, k) falls in the stretches [D s/g, D (s+1)/g)
    that the g lanes of a group evaluate: 'first' / 'last' stretch of some g (g = 2 serves: any Floyd hit
    is in the first half and any shuffle hit in the last), exactly a stretch start, and the first / last
    stretch of a 16- or 12-lane group ('wide_first': a rejection on lane 0 that shifts every other lane;
    'wide_last': one on the last lane with nothing after it)."""
    D = 2 * k - 1
    tags = set()
    for g in GROUPS:
        for s in range(g):
            a, b = D * s // g, D * (s + 1) // g
            if a <= d < b:
                if s == 0:
                    tags.add("stretch_first")
                if s == g - 1:
                    tags.add("stretch_last")
                if s >= 1 and d == a:
                    tags.add("stretch_start")
                if g in WIDE and s == 0:
                    tags.add("wide_first")
                if g in WIDE and s == g - 1:
                    tags.add("wide_last")
    return sorted(tags)


_W = {}


def _worker_env(name):
    if name not in _W:
        import warnings
        from oracle import oracle as O
        from pgtg_amd.config import make_spec
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec = make_spec(**CONFIGS[name])
        cfg = O.config_from_spec(spec)
        L = O.lib()
        h = L.orc_create(C.byref(cfg))
        win = L.orc_window(h)
        obs = (C.c_uint8 * (len(spec.channels) * win * win + 8))()
        _W[name] = (O, L, h, obs, O.OrcOut(), (O.OrcTraceRec * 256)(), (O.OrcCar * 4096)(), cfg)
    return _W[name]


def _cars_crc(L, h, cars) -> int:
    n = L.orc_get_cars(h, cars, 4096)
    return zlib.crc32(bytes(memoryview(cars)[:n]))  # == crc32 of the int32 [n, 7] array


def _records(O, buf, n):
    return [{"site": O.SITES[r.site], "d": r.ord, "n": int(r.n), "buffered": r.buffered, "car": r.car,
             "rejects": r.rejects} for r in buf[:n]]


def scan_resets(args):
    """(name, lo, hi) -> hits [(seed, 0, np, k, crc, draws)] of the seeded resets lo .. hi-1, and the
    number of resets the oracle refused (configurations it cannot run)."""
    name, lo, hi = args
    O, L, h, obs, out, buf, cars, _ = _worker_env(name)
    hits, failed = [], 0
    L.orc_trace_begin(buf, 256)
    np_, k = C.c_int32(), C.c_int32()
    for seed in range(lo, hi):
        L.orc_trace_clear()
        if L.orc_reset(h, seed, obs, C.byref(out)):
            failed += 1
            continue
        n = L.orc_trace_count()
        if n:
            L.orc_get_traffic_reset(h, C.byref(np_), C.byref(k))
            hits.append((seed, 0, np_.value, k.value, _cars_crc(L, h, cars), _records(O, buf, min(n, 256))))
    L.orc_trace_end()
    return lo, hi, hits, failed


def scan_steps(args):
    """(name, lo, hi) -> car-pass hits [(seed, t, np, k, crc after step t, draws)] within IDLE_STEPS idle
    steps of each seed; a hit counts only when the episode runs at least three steps beyond it."""
    name, lo, hi = args
    O, L, h, obs, out, buf, cars, _ = _worker_env(name)
    hits = []
    L.orc_trace_begin(buf, 256)
    np_, k = C.c_int32(), C.c_int32()
    for seed in range(lo, hi):
        if L.orc_reset(h, seed, obs, C.byref(out)):
            continue
        cand, alive = [], IDLE_STEPS + 3
        for t in range(1, IDLE_STEPS + 4):
            L.orc_trace_clear()
            if L.orc_step(h, 4, obs, C.byref(out)) or out.terminated:
                alive = t - 1
                break
            n = L.orc_trace_count()
            if n and t <= IDLE_STEPS:
                recs = [r for r in _records(O, buf, min(n, 256)) if r["site"] == "car_pass"]
                if recs:
                    L.orc_get_traffic_reset(h, C.byref(np_), C.byref(k))
                    cand.append((seed, t, np_.value, k.value, _cars_crc(L, h, cars), recs))
        hits += [c for c in cand if c[1] + 3 <= alive]
    L.orc_trace_end()
    return lo, hi, hits, 0


def classify(hit) -> list[str]:
    """quota names an entry serves"""
    _, step, _, k, _, draws = hit
    tags = set()
    nrej = 0
    for r in draws:
        if r["site"] in ("floyd", "shuffle") and r["rejects"] > 0:
            tags.add(r["site"])
            tags.update(stretch_tags(r["d"], k))
            nrej += 1
            if r["rejects"] > 1:
                tags.add("double")
        if r["site"] == "init_route":
            tags.add("init_route")  # left < n sends the group to the one-lane loop, rejected or not
        if r["site"] == "car_pass" and step > 0:
            tags.add("car_pass")
        if r["site"] == "mapgen" and r["rejects"] > 0:
            tags.add("mapgen")
    if nrej > 1:
        tags.add("double")
    return sorted(tags)


def waves(pool, fn, name, budget, block, per_wave=32):
    """fn over [0, budget) in blocks, in seed order, a wave of blocks at a time (so that a caller that
    stops early leaves at most one wave's work behind, and stops at the same block whatever the pool's size)"""
    starts = list(range(0, budget, block))
    for w in range(0, len(starts), per_wave):
        yield from pool.map(fn, [(name, a, min(a + block, budget)) for a in starts[w:w + per_wave]], chunksize=1)


def run_config(name: str, pool, budget: int, step_budget: int, log) -> dict:
    want = dict(QUOTA)
    if name == "cfg3":
        want.update({q: 1 for q in QUOTA_CFG3})
    have = {q: 0 for q in list(want) + list(EXTRA_CAP)}
    seen = {q: 0 for q in have}  # every hit of the scan, kept or not
    entries = []
    scanned = {"reset": 0, "steps": 0}
    failed = 0

    def take(hit, phase):
        tags = classify(hit)
        for q in tags:
            if q in seen:
                seen[q] += 1
        need = [q for q in tags if (q in want and have[q] < want[q]) or (q in EXTRA_CAP and have[q] < EXTRA_CAP[q])]
        if phase == "reset":
            need = [q for q in need if q != "car_pass"]
        if not need:
            return
        for q in tags:
            if q in have:
                have[q] += 1
        seed, step, np_, k, crc, draws = hit
        entries.append({"config": name, "seed": seed, "step": step, "np": np_, "k": k, "crc32": crc,
                        "tags": tags, "draws": draws})

    def met(keys):
        return all(have[q] >= want[q] for q in keys)

    reset_keys = [q for q in want if q != "car_pass"]
    t0 = time.time()
    for lo, hi, hits, nf in waves(pool, scan_resets, name, budget, BLOCK):
        scanned["reset"] = hi
        failed += nf
        for hit in hits:
            take(hit, "reset")
        if met(reset_keys):
            break
    log(f"{name}: {scanned['reset']} resets in {time.time() - t0:.0f} s, have {have}")
    t0 = time.time()
    for lo, hi, hits, _ in waves(pool, scan_steps, name, step_budget, STEP_BLOCK):
        scanned["steps"] = hi
        for hit in hits:
            take(hit, "steps")
        if met(["car_pass"]):
            break
    log(f"{name}: {scanned['steps']} seeds x {IDLE_STEPS} idle steps in {time.time() - t0:.0f} s, have {have}")
    sites = {}
    for q in have:
        phase = "steps" if q == "car_pass" else "reset"
        sites[q] = {"wanted": want.get(q, 0), "kept": have[q], "found": seen[q], "seeds_scanned": scanned[phase]}
    return {"kwargs": CONFIGS[name], "scanned": scanned, "resets_refused": failed, "sites": sites,
            "not_reached": sorted(q for q in want if have[q] < want[q]),
            "entries": sorted(entries, key=lambda e: (e["step"] > 0, e["seed"], e["step"]))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--budget", type=int, default=10_000_000, help="seeded resets per configuration")
    ap.add_argument("--step-budget", type=int, default=1_000_000, help="seeds run for 60 idle steps per configuration")
    ap.add_argument("--workers", type=int, default=0)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    workers = max(1, min(a.workers or avail, avail, 16))
    from oracle import oracle as O
    O.build()

    def log(s):
        print(s, file=sys.stderr, flush=True)

    doc = {"about": "Seeds whose reset (step 0) or idle step (action 4) meets the Lemire rejection branch, "
                    "found by tools/find_rejection_seeds.py with the CPU oracle's rejection trace. "
                    "d: draw ordinal (Floyd 0..k-1, shuffle k..2k-2; initial route: car index; car pass: "
                    "bounded draws of the step), n: the draw's bound, rejects: halves rejected (0: left < n "
                    "only), crc32: zlib.crc32 of the oracle's int32 car list [n, 7] after that reset or step.",
           "idle_steps": IDLE_STEPS, "groups": list(GROUPS), "configs": {}}
    with mp.Pool(workers) as pool:
        for name in a.configs.split(","):
            doc["configs"][name] = run_config(name, pool, a.budget, a.step_budget, log)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    log(f"wrote {a.out}")


if __name__ == "__main__":
    main()
