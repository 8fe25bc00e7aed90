"""Time one PPO epoch of Rollout.update with torch.optim.Adam (ppo_grad + torch's clip_grad_norm_, Adam and a repack
per minibatch: the path before DeviceAdam) against the same epoch with DeviceAdam (adv_stats + ppo_grad + pgtg_ppo_step),
the two alternating window by window in one session, and DeviceAdam.step and DevicePolicy.adv_stats alone.  Prints one
JSON line per batch size; every window is reported.

    python tools/ppo_step_bench.py [--envs 65536] [--steps 8] [--windows 5] [--out profiles/ppo_step/update_bench.jsonl]
"""
import argparse
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgtg_amd import policy as P  # noqa: E402

TRAIN = dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=0.2,
             random_map_percentage_of_connections=0.8, traffic_density=0.2, conservative_driver_percentage=0.15,
             normal_driver_percentage=0.50, aggressive_driver_percentage=0.20, elderly_driver_percentage=0.10,
             reckless_driver_percentage=0.05, sliding_observation_window_size=5, max_allowed_deviation=15,
             use_sliding_observation_window=True, use_next_subgoal_direction=True, final_goal_bonus=200,
             standing_still_penalty=1)
REPS = 50  # calls per window of the two single-call measurements


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = PGTGVecEnv(a.envs, device=0, autoreset=True, max_episode_steps=100, **TRAIN)
    # one rollout, two (policy, module, optimiser) sets from the same weights
    pt, pd = P.DevicePolicy(env, seed=0), P.DevicePolicy(env, seed=0)
    torch.manual_seed(0)
    mt, md = P.MlpPolicyReference(pt.obs_dim).cuda(), P.MlpPolicyReference(pt.obs_dim).cuda()
    md.load_state_dict(mt.state_dict())
    pt.load_state_dict(mt.state_dict())
    pd.load_state_dict(md.state_dict())
    ro = env.rollout(a.steps)
    ro.begin(seed=0)
    ro.collect(pt)
    ot = torch.optim.Adam(mt.parameters(), lr=3e-4, eps=1e-5)
    od = P.DeviceAdam(pd, md, lr=3e-4, eps=1e-5)
    total = a.steps * a.envs
    lines = []
    for bs in (4096, 65536):
        if bs > total:
            continue
        torch_arm = lambda: ro.update(pt, mt, ot, n_epochs=1, batch_size=bs)  # noqa: E731
        device_arm = lambda: ro.update(pd, md, od, n_epochs=1, batch_size=bs)  # noqa: E731
        idx = torch.randperm(total, device="cuda")[:bs]
        out = torch.zeros(2, device="cuda")
        grads = {k: p.grad for k, p in md.named_parameters()}
        step = lambda: [od.step(grads=grads) for _ in range(REPS)]  # noqa: E731
        stats = lambda: [pd.adv_stats(ro, idx, out=out) for _ in range(REPS)]  # noqa: E731
        for fn in (torch_arm, device_arm):  # warm-up: one epoch each (and the .grad tensors exist afterwards)
            fn()
        grads = {k: p.grad for k, p in md.named_parameters()}
        step()
        stats()
        torch.cuda.synchronize()
        t, d = [], []
        for _ in range(a.windows):  # the two arms alternate
            t.append(round(window(torch_arm), 3))
            d.append(round(window(device_arm), 3))
        s = [round(window(step) / REPS, 4) for _ in range(a.windows)]
        v = [round(window(stats) / REPS, 4) for _ in range(a.windows)]
        lines.append(dict(envs=a.envs, steps=a.steps, obs_dim=pt.obs_dim, batch=bs, minibatches=-(-total // bs),
                          torch_adam_epoch_ms=t, device_adam_epoch_ms=d, device_adam_step_ms=s, adv_stats_ms=v))
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(ln) + "\n" for ln in lines)
    ro.close()
    env.close()


if __name__ == "__main__":
    main()
