"""Cost of the rollout's reward normalisation (pgtg_amd/csrc/pgtg_norm.h; include/pgtg.h pgtg_reward_norm) beside
k_gae and k_cost_scan.

    python tools/norm_bench.py [--shape 65536x128] [--reps 20] [--windows 5] [--out profiles/reward_norm/finish.jsonl]

On synthetic device arrays (about an episode end per 50 steps, half of them truncations), HIP events around `reps`
back-to-back calls on the handle's stream, `windows` windows after a warm-up window, microseconds per call (launch
gaps included): pgtg_gae, pgtg_cost_scan, pgtg_reward_norm training and frozen, and the three chained as finish()
chains them; each against its byte model at the copy bandwidth pgtg_measure_hbm reports (18, 13 and 5.375 + 8 bytes
per sample: the scan reads 4 + 1 and writes 24 per 64 envs, the apply reads 4 and writes 4).  Then Rollout.finish()
itself with and without norm_reward (one call per event pair: the host's part included).  Under
`rocprofv3 --kernel-trace --stats` the same run gives each kernel's own time."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgtg_amd import _abi  # noqa: E402
from pgtg_amd.vector import PGTGVecEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="65536x128")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
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
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def windows(fn, reps):
        out = []
        for w in range(args.windows + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            if w:  # (the first window warms up)
                out.append(a.elapsed_time(b) * 1e3 / reps)
        return out

    def stat(us):
        return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}

    n, T = (int(x) for x in args.shape.split("x"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tiny = PGTGVecEnv(2, device=0, random_map_width=3, random_map_height=3)
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    rew, val, tval, lv = rnd(T, n) * 50, rnd(T, n), rnd(T, n), rnd(n)
    cost = (torch.rand(T, n, device="cuda", generator=g) < 0.1).to(torch.float32)
    u = torch.rand(T + 1, n, device="cuda", generator=g)
    dones = u < 0.02
    tonly = dones[1:] & (u[1:] < 0.01)
    adv, ret, pen, nrm = (torch.empty_like(rew) for _ in range(4))
    carry = torch.zeros(n, dtype=torch.float64, device="cuda")
    lam = torch.full((1,), 0.5, device="cuda")
    summary = torch.zeros(5, dtype=torch.int64, device="cuda")
    nbytes = C.c_uint64()
    assert lib.pgtg_cost_workspace_bytes(n, C.byref(nbytes)) == 0
    ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device="cuda")
    assert lib.pgtg_reward_norm_workspace_bytes(n, T, C.byref(nbytes)) == 0
    nws = torch.empty(nbytes.value // 8, dtype=torch.float64, device="cuda")
    rets = torch.zeros(n, dtype=torch.float64, device="cuda")
    rms = torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64, device="cuda")
    row_var = torch.zeros(T, dtype=torch.float64, device="cuda")

    def gae_args(r):
        return _abi.PgtgGae(n=n, steps=T, gamma=0.99, gae_lambda=0.95, rewards=p(r), values=p(val), dones=p(dones),
                            truncated_only=p(tonly), terminal_values=p(tval), last_values=p(lv), advantages=p(adv),
                            returns=p(ret))

    def cost_args(r):
        return _abi.PgtgCost(n=n, steps=T, rewards=p(r), costs=p(cost), dones=p(dones), ep_cost=p(carry), penalised=p(pen),
                             lambda_=p(lam), cost_limit=1.0, lambda_lr=0.0, lambda_max=100.0, summary=p(summary),
                             workspace=p(ws))

    def norm_args(training):
        return _abi.PgtgRewardNorm(n=n, steps=T, gamma=0.99, epsilon=1e-8, clip=10.0, training=training, rewards=p(rew),
                                   dones=p(dones), returns=p(rets), rms=p(rms), row_var=p(row_var), normalised=p(nrm),
                                   workspace=p(nws))
    g_raw, g_pen, c_raw, c_nrm, n_on, n_off = gae_args(rew), gae_args(pen), cost_args(rew), cost_args(nrm), norm_args(1), norm_args(0)
    tiny._bind_stream()
    call = lambda f, a: (lambda: _ok(f(tiny._h, C.byref(a))))  # noqa: E731

    def _ok(rc):
        assert rc == 0

    def chain():
        _ok(lib.pgtg_reward_norm(tiny._h, C.byref(n_on)))
        _ok(lib.pgtg_cost_scan(tiny._h, C.byref(c_nrm)))
        _ok(lib.pgtg_gae(tiny._h, C.byref(g_pen)))

    fns = (("k_gae", call(lib.pgtg_gae, g_raw)), ("cost_scan", call(lib.pgtg_cost_scan, c_raw)),
           ("reward_norm", call(lib.pgtg_reward_norm, n_on)), ("reward_norm_frozen", call(lib.pgtg_reward_norm, n_off)),
           ("norm_then_cost_then_gae", chain), ("k_gae_again", call(lib.pgtg_gae, g_raw)))
    us = {k: windows(f, args.reps) for k, f in fns}
    W = (n + 63) // 64
    bw = gbs.value * 1e9
    model = {"k_gae": (18 * n * T + 4 * int(tonly.sum())) / bw * 1e6, "cost_scan": (13 * n * T + 16 * n) / bw * 1e6,
             "reward_norm": (5 * n * T + 16 * n + 2 * 24 * W * T + 8 * n * T) / bw * 1e6,
             "reward_norm_frozen": 8 * n * T / bw * 1e6}
    emit({"what": "kernels", "envs": n, "steps": T, "reps": args.reps, "windows": args.windows,
          "copy_gbs": round(gbs.value, 1), "us_per_call": {k: stat(v) for k, v in us.items()},
          "byte_model_us": {k: round(v, 2) for k, v in model.items()},
          "over_model": {k: round(statistics.median(us[k]) / v, 2) for k, v in model.items()},
          "norm_over_gae": round(statistics.median(us["reward_norm"]) / statistics.median(us["k_gae"]), 3)})
    del rew, val, tval, cost, u, dones, tonly, adv, ret, pen, nrm, nws
    torch.cuda.empty_cache()
    tiny.close()

    # -- Rollout.finish() itself ------------------------------------------------------------------------
    kw = dict(random_map_width=3, random_map_height=3, use_sliding_observation_window=True,
              sliding_observation_window_size=1)  # (the smallest rows: obs is not what is timed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = PGTGVecEnv(n, device=0, autoreset=True, max_episode_steps=100, **kw)
    res = {}
    for name, extra in (("without_norm_reward", {}), ("with_norm_reward", dict(norm_reward=True))):
        ro = env.rollout(T, **extra)
        g = torch.Generator(device="cuda").manual_seed(2)
        ro.begin(seed=0)
        ro.rewards.copy_(torch.randn(T, n, device="cuda", generator=g) * 50)
        ro.values.copy_(torch.randn(T, n, device="cuda", generator=g))
        ro.dones.copy_(torch.rand(T + 1, n, device="cuda", generator=g) < 0.02)
        ro.t = T  # (rows filled by hand in place of T steps)
        last = torch.randn(n, device="cuda", generator=g)
        res[name] = stat(windows(lambda: ro.finish(last), 1))
        ro.close()
        del ro
        torch.cuda.empty_cache()
    emit({"what": "Rollout.finish", "envs": n, "steps": T, "windows": args.windows, "us_per_call": res})
    env.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
