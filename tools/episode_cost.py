"""Per-tick cost of the episode-statistics pass (k_episode, include/pgtg.h pgtg_set_episode_stats).

Times pgtg_step_many over resident actions with the statistics bound and unbound on ONE handle per
workload, the two alternating (`--rounds` pairs of `--ticks` ticks each, after a warm-up of both), with a
host clock around work that ends in a device synchronise.  Prints one JSON line per timed window and a
summary line per workload with the byte model beside it: 34 B x N over the measured stream-copy
bandwidth (pgtg_measure_hbm).

    python tools/episode_cost.py [--workloads cfg5,train] [--ticks 200] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_ENV_STEP = 34  # 8 + 1 + 1 read, 8 + 8 accumulators read and written, 8 outputs written


def main():
    import torch

    import bench
    from pgtg_amd import _abi
    from pgtg_amd.config import make_spec
    from pgtg_amd.vector import PGTGVecEnv
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg5,train")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    gbs = C.c_double()
    rc = _abi.lib().pgtg_measure_hbm(0, 1 << 30, 20, C.byref(gbs))
    assert rc == 0, rc
    for name in args.workloads.split(","):
        _, _, n, kw = bench.WORKLOADS[name]
        kw = dict(kw)
        n = args.envs or n
        limit = kw.pop("max_episode_steps", None)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec = make_spec(**kw)
        env = PGTGVecEnv(n, spec=spec, device=0, autoreset=True, max_episode_steps=limit)
        env.reset(seed=0)
        actions = env.random_actions(args.ticks, seed=1)
        ep = env.enable_episode_stats()
        env.disable_episode_stats()

        def window(on):
            if on:
                env.enable_episode_stats(*ep)
            else:
                env.disable_episode_stats()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.step_many(actions)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.ticks * 1e6

        for on in (False, True):  # warm-up of both
            window(on)
        us = {False: [], True: []}
        for r in range(args.rounds):
            for on in (False, True):
                v = window(on)
                us[on].append(v)
                emit({"workload": name, "envs": n, "round": r, "stats": on, "ticks": args.ticks, "us_per_tick": round(v, 3)})
        off, on_ = statistics.median(us[False]), statistics.median(us[True])
        model_us = BYTES_PER_ENV_STEP * n / (gbs.value * 1e9) * 1e6
        emit({"workload": name, "envs": n, "kernel": env.step_kernel(), "us_per_tick_off_median": round(off, 3),
              "us_per_tick_on_median": round(on_, 3), "cost_us_per_tick": round(on_ - off, 3),
              "off_spread_us": round(max(us[False]) - min(us[False]), 3),
              "copy_gbs": round(gbs.value, 1), "byte_model_us": round(model_us, 3),
              "episodes": env.episode_summary()["episodes"]})
        env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
