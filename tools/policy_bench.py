"""Cost of the fused policy (pgtg_amd/policy.py; include/pgtg.h pgtg_policy) against the torch-eager path.

At `--envs` envs of the caller's settings (pgtg/train.py:21-38), on int8 rows of a really stepped batch:

1. one k_policy SAMPLE launch against the torch path of the same function on the same tensors --
   obs.float(), the MlpPolicyReference forward, Categorical sample and log_prob -- each timed with HIP
   events around `--launches` launches, the two interleaved over `--rounds` rounds in this one process
   after a warm-up of both; also at 4 096 and 1 048 576 rows (the batch's rows, cut or repeated);
2. Rollout.collect per step against the same loop with the torch policy (Rollout.step fed by torch).

Beside the kernel's time stands its byte model: N * D observation bytes read and 9 B written per env from
HBM (W1 is re-read by every block of 64 envs, from L2) over the measured stream-copy bandwidth
(pgtg_measure_hbm).  Prints one JSON line; `--out` also writes it to a file.
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
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32, help="rollout length of the collect comparison")
    ap.add_argument("--limit", type=int, default=100, help="max_episode_steps")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from torch.distributions import Categorical

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
    D = policy.obs_dim
    module = MlpPolicyReference(D).cuda()
    policy.load_state_dict(module.state_dict())
    ro = env.rollout(T)

    def torch_policy(obs):
        with torch.no_grad():
            logits, value = module(obs.float())
            dist = Categorical(logits=logits)
            a = dist.sample()
            return a, value, dist.log_prob(a)

    def torch_value(obs):
        with torch.no_grad():
            return module(obs.float())[1]

    def torch_collect():
        obs = ro.begin()
        for _ in range(T):
            a, v, lp = torch_policy(obs)
            obs, _, _ = ro.step(a.to(torch.uint8), v, lp)
            ro.set_terminal_values(torch_value(ro.terminal_obs))
        ro.finish(torch_value(obs))

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    # real rows: a warm rollout with the fused policy
    ro.begin(seed=3)
    ro.collect(policy)
    rows = ro.obs[T // 2].clone()
    sizes = {}
    for n in sorted({4096, N, 1048576}):
        obs = rows[:n].contiguous() if n <= N else rows.repeat((n + N - 1) // N, 1)[:n].contiguous()
        outs = (torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda"))
        fused = lambda: policy.act(obs, *outs)  # noqa: E731
        eager = lambda: torch_policy(obs)  # noqa: E731
        reps = args.launches
        timed(fused, 10), timed(eager, 10)
        f_ms, t_ms = [], []
        for _ in range(args.rounds):
            f_ms.append(timed(fused, reps))
            t_ms.append(timed(eager, reps))
        fm, tm = statistics.median(f_ms), statistics.median(t_ms)
        model_bytes = n * D + 9 * n
        sizes[str(n)] = {"fused_ms": fm, "fused_ms_min": min(f_ms), "fused_ms_max": max(f_ms), "torch_ms": tm,
                         "torch_ms_min": min(t_ms), "torch_ms_max": max(t_ms), "torch_over_fused": tm / fm,
                         "model_bytes": model_bytes, "model_gbs": model_bytes / fm / 1e6,
                         "frac_of_copy_peak": model_bytes / fm / 1e6 / gbs.value,
                         "tflops_f32": 2.0 * n * (D * 128 + 2 * 64 * 64 + 640) / fm / 1e9,
                         "env_steps_per_s": n / fm * 1e3}
        del obs, outs
    # the collection loop, per step
    timed(lambda: ro.collect(policy), 2), timed(torch_collect, 2)
    c_ms, tc_ms = [], []
    for _ in range(args.rounds):
        c_ms.append(timed(lambda: ro.collect(policy), 3) / T)
        tc_ms.append(timed(torch_collect, 3) / T)
    rec = {"tool": "policy_bench", "envs": N, "obs_dim": D, "launches": args.launches, "rounds": args.rounds,
           "copy_gbs": gbs.value, "device": torch.cuda.get_device_name(0), "sizes": sizes,
           "collect": {"steps": T, "max_episode_steps": args.limit, "fused_ms_per_step": statistics.median(c_ms),
                       "fused_min": min(c_ms), "fused_max": max(c_ms), "torch_ms_per_step": statistics.median(tc_ms),
                       "torch_min": min(tc_ms), "torch_max": max(tc_ms),
                       "fused_env_steps_per_s": N / statistics.median(c_ms) * 1e3,
                       "torch_env_steps_per_s": N / statistics.median(tc_ms) * 1e3}}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ro.close()
    env.close()


if __name__ == "__main__":
    main()
