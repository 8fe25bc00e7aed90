"""Cost of the device rollout buffer (pgtg_amd/rollout.py; include/pgtg.h pgtg_gae).

1. k_gae: device time of one launch (HIP events around it, after a warm-up; median and spread of `--reps`
   launches) at the caller's shape and at a wide, short one, beside its byte model -- 18 B per sample plus
   4 B per truncated sample over the measured stream-copy bandwidth (pgtg_measure_hbm) -- and beside the
   same formula as a loop of torch operations on the device (the yardstick of the speed-up, not code under
   test; its result is compared with the kernel's).
2. Recording: time per tick through Rollout.step against the device path without it -- fresh flat rows and
   scalars bound for every step, the same kernels -- on ONE handle, the two alternating (`--rounds` pairs
   of `--ticks` ticks after a warm-up of both), host clock around work that ends in a synchronise.

    python tools/rollout_cost.py [--shapes 65536x128,1048576x16] [--reps 20] [--workload train]
                                 [--ticks 64] [--rounds 5] [--out profiles/rollout/NAME.json]
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


def torch_gae(rew, val, dones, tonly, tval, last_values, gamma, gae_lambda):
    """The formula of include/pgtg.h pgtg_gae as torch operations, one row at a time."""
    import torch
    T = rew.shape[0]
    g = torch.tensor(gamma, dtype=torch.float32, device=rew.device)
    gl = torch.tensor(gamma * gae_lambda, dtype=torch.float32, device=rew.device)
    adv = torch.empty_like(rew)
    last = torch.zeros_like(last_values)
    for t in range(T - 1, -1, -1):
        r = torch.where(tonly[t], rew[t] + g * tval[t], rew[t])
        nnt = 1.0 - dones[t + 1].to(torch.float32)
        nv = last_values if t == T - 1 else val[t + 1]
        last = (r + (g * nv) * nnt) - val[t] + (gl * nnt) * last
        adv[t] = last
    return adv, adv + val


def main():
    import torch

    import bench
    from pgtg_amd import _abi
    from pgtg_amd.config import make_spec
    from pgtg_amd.vector import PGTGVecEnv
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x128,1048576x16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--workload", default="train")
    ap.add_argument("--envs", type=int, default=0)
    ap.add_argument("--ticks", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    lib = _abi.lib()
    gbs = C.c_double()
    assert lib.pgtg_measure_hbm(0, 1 << 30, 20, C.byref(gbs)) == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tiny = PGTGVecEnv(2, spec=make_spec(random_map_width=3, random_map_height=3), device=0)

    def timed(fn, reps):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) * 1e3)
        return ms

    # -- 1. the scan -------------------------------------------------------------------------------
    gamma, lam = 0.99, 0.95
    for shape in args.shapes.split(","):
        n, T = (int(x) for x in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s: torch.randn(*s, device="cuda", generator=g) * 100  # noqa: E731
        rew, val, tval, lv = rnd(T, n), rnd(T, n), rnd(T, n), rnd(n)
        u = torch.rand(T + 1, n, device="cuda", generator=g)
        dones = u < 0.02           # about an episode end per 50 steps,
        tonly = dones[1:] & (u[1:] < 0.01)  # half of them truncations
        adv, ret = torch.empty_like(rew), torch.empty_like(rew)
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        a = _abi.PgtgGae(n=n, steps=T, gamma=gamma, gae_lambda=lam, rewards=p(rew), values=p(val), dones=p(dones),
                         truncated_only=p(tonly), terminal_values=p(tval), last_values=p(lv), advantages=p(adv),
                         returns=p(ret))
        tiny._bind_stream()

        def kernel():
            assert lib.pgtg_gae(tiny._h, C.byref(a)) == 0

        timed(kernel, 3)
        k_us = timed(kernel, args.reps)
        t_adv, t_ret = torch_gae(rew, val, dones, tonly, tval, lv, gamma, lam)  # (warm-up and the comparison)
        same = bool(torch.equal(t_adv.view(torch.int32), adv.view(torch.int32))
                    and torch.equal(t_ret.view(torch.int32), ret.view(torch.int32)))
        t_us = timed(lambda: torch_gae(rew, val, dones, tonly, tval, lv, gamma, lam), args.torch_reps)
        nbytes = 18 * n * T + 4 * int(tonly.sum())
        model = nbytes / (gbs.value * 1e9) * 1e6
        km, tm = statistics.median(k_us), statistics.median(t_us)
        emit({"what": "k_gae", "envs": n, "steps": T, "reps": args.reps, "k_gae_us_median": round(km, 2),
              "k_gae_us_min": round(min(k_us), 2), "k_gae_us_max": round(max(k_us), 2), "bytes": nbytes,
              "copy_gbs": round(gbs.value, 1), "byte_model_us": round(model, 2), "over_model": round(km / model, 2),
              "torch_loop_us_median": round(tm, 1), "torch_loop_us_min": round(min(t_us), 1),
              "torch_loop_us_max": round(max(t_us), 1), "torch_over_k_gae": round(tm / km, 1),
              "torch_loop_bit_equal": same})
        del rew, val, tval, dones, tonly, adv, ret, t_adv, t_ret, u
        torch.cuda.empty_cache()
    tiny.close()

    # -- 2. recording ------------------------------------------------------------------------------
    if args.workload:
        _, _, n, kw = bench.WORKLOADS[args.workload]
        kw = dict(kw)
        n = args.envs or n
        limit = kw.pop("max_episode_steps", 100)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec = make_spec(**kw)
        env = PGTGVecEnv(n, spec=spec, device=0, autoreset=True, max_episode_steps=limit)
        ro = env.rollout(args.ticks)
        D, dt = ro.obs_dim, ro.obs.dtype
        acts = env.random_actions(args.ticks, seed=1)
        ro.begin(seed=0)

        def window(recorded):
            if recorded:
                ro.begin()  # (row T to row 0: once per rollout, outside the per-tick figure)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if recorded:
                for t in range(args.ticks):
                    ro.step(acts[t])
            else:
                for t in range(args.ticks):
                    flat = torch.empty((n, D), dtype=dt, device="cuda")
                    fin = torch.empty((n, D), dtype=dt, device="cuda")
                    sc = (torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.bool, device="cuda"),
                          torch.empty(n, dtype=torch.bool, device="cuda"))
                    env._bind_flat_ptrs(flat, fin, ro._dtype_code)
                    env._bind_flat_scalar_ptrs(*sc)
                    env.step_actions(acts[t])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.ticks * 1e6

        for m in (False, True):
            window(m)
        us = {False: [], True: []}
        for r in range(args.rounds):
            for m in (False, True):
                v = window(m)
                us[m].append(v)
                emit({"what": "recording", "workload": args.workload, "envs": n, "round": r, "rollout": m,
                      "ticks": args.ticks, "us_per_tick": round(v, 2)})
        off, on = statistics.median(us[False]), statistics.median(us[True])
        emit({"what": "recording_summary", "workload": args.workload, "envs": n, "obs_dim": D, "kernel": env.step_kernel(),
              "rollout_bytes": ro.nbytes, "fresh_us_per_tick_median": round(off, 2), "rollout_us_per_tick_median": round(on, 2),
              "difference_us": round(on - off, 2), "fresh_spread_us": round(max(us[False]) - min(us[False]), 2),
              "rollout_spread_us": round(max(us[True]) - min(us[True]), 2)})
        ro.close()
        env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
