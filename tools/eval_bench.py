"""Cost of an evaluation step (pgtg_amd/evaluate.py; include/pgtg.h pgtg_eval_step) against a collection step.

At `--envs` envs of the caller's settings (pgtg/train.py:21-38) with a time limit, in one process after a
warm-up of both, interleaved over `--rounds` rounds (the evaluation loop first in odd rounds, the collection
loop first in even ones, so that an effect of the order would show as spread) and timed with HIP events:

1. Evaluation.run's step: k_policy (argmax), the tick and k_eval -- `--steps` steps with every env open
   (n_episodes is set so high that no quota is met in the window, so k_eval does its full work every step);
2. Rollout.collect's step: k_policy (sample), the tick and the value-only pass on the terminal rows -- the
   path this library trains with, which the evaluation does not touch;
3. k_eval alone: the launch-to-launch interval of `--launches` back-to-back launches of record_from on the
   env's last rewards and flags that are all zero (no episode ends: no record row is written, every env
   accumulates).  An interval, not the kernel's time: at this size a launch is shorter than the gap between
   launches.  The kernel's own time is the k_eval row of a kernel trace of this tool, taken in a run of its own
   (`rocprofv3 --kernel-trace --stats -- python tools/eval_bench.py ...`), never in a run whose timings are used.

Beside the interval stands k_eval's byte model for that loop: per open env-step 14 B read (reward, two flags,
cnt) and 28 B of accumulators read and written, over the measured stream-copy bandwidth (pgtg_measure_hbm).
Prints one JSON line; `--out` also writes it to a file.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TRAIN = dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=0.2,
             random_map_percentage_of_connections=0.8, traffic_density=0.2, conservative_driver_percentage=0.15,
             normal_driver_percentage=0.50, aggressive_driver_percentage=0.20, elderly_driver_percentage=0.10,
             reckless_driver_percentage=0.05, sliding_observation_window_size=5, max_allowed_deviation=15,
             use_sliding_observation_window=True, use_next_subgoal_direction=True, final_goal_bonus=200,
             standing_still_penalty=1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=32, help="steps of a timed window (the rollout's length)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=2000, help="k_eval launches of a timed window")
    ap.add_argument("--limit", type=int, default=100, help="max_episode_steps")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from pgtg_amd import _abi
    from pgtg_amd.policy import DevicePolicy, MlpPolicyReference
    from pgtg_amd.vector import PGTGVecEnv

    N, T = args.envs, args.steps
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = PGTGVecEnv(N, device=0, autoreset=True, max_episode_steps=args.limit, **TRAIN)
    gbs = C.c_double()
    assert _abi.lib().pgtg_measure_hbm(0, 1 << 30, 20, C.byref(gbs)) == 0
    torch.manual_seed(0)
    policy = DevicePolicy(env, seed=1)
    policy.load_state_dict(MlpPolicyReference(policy.obs_dim).state_dict())
    ro = env.rollout(T)
    # a quota per env that no timed window reaches: every env stays open, so k_eval does its full work
    ev = env.evaluation(N * (T + 1))
    no_flag = torch.zeros(N, dtype=torch.bool, device=env.device)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def collect_steps():  # (what Rollout.collect does per step after begin(), without k_gae)
        while ro.t < T:
            ro.act(policy)

    def eval_steps():
        a, v, lp = ev._actions, ev._values, ev._log_probs
        for _ in range(T):
            policy.act(ev.obs, a, v, lp, deterministic=True)
            ev.step(a)

    def eval_alone():
        for _ in range(args.launches):
            ev.record_from(env.reward, no_flag, no_flag)

    c_ms, e_ms, k_ms = [], [], []
    def collect_round():
        ro.begin(seed=3)
        ms = timed(collect_steps) / T
        ro.close()
        return ms

    def eval_round():
        ev.begin(seed=3)
        return timed(eval_steps) / T

    for rnd in range(args.rounds + 1):  # (round 0 warms both paths up and is dropped)
        if rnd % 2:
            e, c = eval_round(), collect_round()
            ev.begin(seed=3)  # (the collection unbound the evaluation's rows)
        else:
            c, e = collect_round(), eval_round()
        ev.clear()
        k = timed(eval_alone) / args.launches
        assert ev.open_envs() == N  # (no quota was met: k_eval worked on every env in every launch)
        ev.close()
        if rnd:
            c_ms.append(c), e_ms.append(e), k_ms.append(k)
    med = statistics.median
    model_bytes = N * (14 + 2 * 28)
    rec = {"tool": "eval_bench", "envs": N, "obs_dim": policy.obs_dim, "steps": T, "rounds": args.rounds,
           "max_episode_steps": args.limit, "copy_gbs": gbs.value, "device": torch.cuda.get_device_name(0),
           "step_kernel": env.step_kernel(),
           "eval_ms_per_step": med(e_ms), "eval_min": min(e_ms), "eval_max": max(e_ms),
           "collect_ms_per_step": med(c_ms), "collect_min": min(c_ms), "collect_max": max(c_ms),
           "eval_over_collect": med(e_ms) / med(c_ms),
           "launches": args.launches,
           "k_eval_interval_ms": med(k_ms), "k_eval_interval_min": min(k_ms), "k_eval_interval_max": max(k_ms),
           "k_eval_model_bytes": model_bytes,
           "eval_env_steps_per_s": N / med(e_ms) * 1e3, "collect_env_steps_per_s": N / med(c_ms) * 1e3,
           "errors": env.error_count()[0]}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()
