"""Time one PPO epoch over a collected rollout: Rollout.update (k_ppo_loss, k_ppo_dw1, k_ppo_reduce + torch's clip
and Adam) against the written-out torch loop (Rollout.get + autograd of SB3's loss + the same clip and Adam), and
DevicePolicy.ppo_grad alone.  Prints one JSON line per measurement; every window is reported.

    python tools/ppo_bench.py [--envs 65536] [--steps 8] [--windows 5] [--out profiles/ppo_grad/update_bench.jsonl]
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


def sb3_loss(module, obs, act, old, adv, ret, clip=0.2, ent=0.0, vf=0.5):
    logits, values = module(obs)
    lsm = torch.log_softmax(logits, dim=1)
    logp = lsm.gather(1, act[:, None])[:, 0]
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(logp - old)
    pol = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    return pol + ent * (-(-(lsm.exp() * lsm).sum(dim=1)).mean()) + vf * torch.nn.functional.mse_loss(ret, values)


def torch_epoch(module, opt, ro, bs):
    total = ro.n_steps * ro.num_envs
    perm = torch.randperm(total, device=ro.device)
    for lo in range(0, total, bs):
        obs_b, act_b, _, logp_b, adv_b, ret_b = next(ro.get(indices=perm[lo:lo + bs]))
        loss = sb3_loss(module, obs_b, act_b, logp_b, adv_b, ret_b)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(module.parameters(), 0.5)
        opt.step()


def timed(fn, windows):
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(round(e0.elapsed_time(e1), 3))
    return out


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
    pol = P.DevicePolicy(env, seed=0)
    torch.manual_seed(0)
    mk, mt = P.MlpPolicyReference(pol.obs_dim).cuda(), P.MlpPolicyReference(pol.obs_dim).cuda()
    mt.load_state_dict(mk.state_dict())
    pol.load_state_dict(mk.state_dict())
    ro = env.rollout(a.steps)
    ro.begin(seed=0)
    ro.collect(pol)
    ok, ot = torch.optim.Adam(mk.parameters(), lr=3e-4, eps=1e-5), torch.optim.Adam(mt.parameters(), lr=3e-4, eps=1e-5)
    lines = []
    total = a.steps * a.envs
    for bs in (4096, 65536):
        if bs > total:
            continue
        fused = lambda: ro.update(pol, mk, ok, n_epochs=1, batch_size=bs)  # noqa: E731
        eager = lambda: torch_epoch(mt, ot, ro, bs)  # noqa: E731
        idx = torch.randperm(total, device="cuda")[:bs]
        grad = lambda: [pol.ppo_grad(ro, idx) for _ in range(20)]  # noqa: E731
        for fn in (fused, eager, grad):  # warm-up
            fn()
        torch.cuda.synchronize()
        f, e, g = timed(fused, a.windows), timed(eager, a.windows), [round(x / 20, 4) for x in timed(grad, a.windows)]
        med = sorted(g)[len(g) // 2]
        lines.append(dict(envs=a.envs, steps=a.steps, obs_dim=pol.obs_dim, batch=bs, minibatches=-(-total // bs),
                          update_epoch_ms=f, torch_epoch_ms=e, ppo_grad_ms=g,
                          dw1_model_tflops_if_all_time=round(2 * bs * pol.obs_dim * 128 / (med * 1e-3) / 1e12, 2)))
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(ln) + "\n" for ln in lines)
    ro.close()
    env.close()


if __name__ == "__main__":
    main()
