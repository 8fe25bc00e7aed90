"""Cost of the rollout's cost scan (pgtg_amd/csrc/pgtg_cost.h; include/pgtg.h pgtg_cost_scan) beside k_gae.

    python tools/cost_bench.py [--shapes 65536x128] [--reps 20] [--windows 5] [--out profiles/cost/finish.jsonl]

Per shape, on synthetic device arrays (about an episode end per 50 steps, half of them truncations), HIP events
around `reps` back-to-back calls on the handle's stream, `windows` windows after a warm-up window, microseconds
per call (launch gaps included):
  k_gae alone (pgtg_gae, with the bootstrap) -- what finish() is without cost_limit;
  k_cost_scan + k_cost_dual alone (pgtg_cost_scan);
  both, the scan feeding k_gae its penalised rewards -- what finish() is with cost_limit;
and each against its byte model at the copy bandwidth pgtg_measure_hbm reports (18 B and 13 B per sample).
Then Rollout.finish() itself, with and without cost_limit, on a rollout of the first shape (one call per event
pair: the host's part of the call included)."""
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
    ap.add_argument("--shapes", default="65536x128")
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

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tiny = PGTGVecEnv(2, device=0, random_map_width=3, random_map_height=3)
    for shape in args.shapes.split(","):
        n, T = (int(x) for x in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
        rew, val, tval, lv = rnd(T, n), rnd(T, n), rnd(T, n), rnd(n)
        cost = (torch.rand(T, n, device="cuda", generator=g) < 0.1).to(torch.float32)
        u = torch.rand(T + 1, n, device="cuda", generator=g)
        dones = u < 0.02
        tonly = dones[1:] & (u[1:] < 0.01)
        adv, ret, pen = torch.empty_like(rew), torch.empty_like(rew), torch.empty_like(rew)
        carry = torch.zeros(n, dtype=torch.float64, device="cuda")
        lam = torch.full((1,), 0.5, device="cuda")
        summary = torch.zeros(5, dtype=torch.int64, device="cuda")
        nbytes = C.c_uint64()
        assert lib.pgtg_cost_workspace_bytes(n, C.byref(nbytes)) == 0
        ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device="cuda")

        def gae_args(r):
            return _abi.PgtgGae(n=n, steps=T, gamma=0.99, gae_lambda=0.95, rewards=p(r), values=p(val), dones=p(dones),
                                truncated_only=p(tonly), terminal_values=p(tval), last_values=p(lv), advantages=p(adv),
                                returns=p(ret))
        g_raw, g_pen = gae_args(rew), gae_args(pen)
        c = _abi.PgtgCost(n=n, steps=T, rewards=p(rew), costs=p(cost), dones=p(dones), ep_cost=p(carry), penalised=p(pen),
                          lambda_=p(lam), cost_limit=1.0, lambda_lr=0.0, lambda_max=100.0, summary=p(summary), workspace=p(ws))
        tiny._bind_stream()

        def gae():
            assert lib.pgtg_gae(tiny._h, C.byref(g_raw)) == 0

        def scan():
            assert lib.pgtg_cost_scan(tiny._h, C.byref(c)) == 0

        def both():
            assert lib.pgtg_cost_scan(tiny._h, C.byref(c)) == 0
            assert lib.pgtg_gae(tiny._h, C.byref(g_pen)) == 0

        us = {k: windows(f, args.reps) for k, f in (("k_gae", gae), ("cost_scan", scan), ("cost_scan_then_k_gae", both),
                                                    ("k_gae_again", gae))}
        model = {"k_gae": (18 * n * T + 4 * int(tonly.sum())) / (gbs.value * 1e9) * 1e6,
                 "cost_scan": (13 * n * T + 16 * n) / (gbs.value * 1e9) * 1e6}
        emit({"what": "kernels", "envs": n, "steps": T, "reps": args.reps, "windows": args.windows,
              "copy_gbs": round(gbs.value, 1), "us_per_call": {k: stat(v) for k, v in us.items()},
              "byte_model_us": {k: round(v, 2) for k, v in model.items()},
              "over_model": {k: round(statistics.median(us[k]) / v, 2) for k, v in model.items()},
              "scan_over_gae": round(statistics.median(us["cost_scan"]) / statistics.median(us["k_gae"]), 3)})
        del rew, val, tval, cost, u, dones, tonly, adv, ret, pen
        torch.cuda.empty_cache()
    tiny.close()

    # -- Rollout.finish() itself ------------------------------------------------------------------------
    n, T = (int(x) for x in args.shapes.split(",")[0].split("x"))
    kw = dict(random_map_width=3, random_map_height=3, use_sliding_observation_window=True,
              sliding_observation_window_size=1, separate_reward_cost=True)  # (the smallest rows: obs is not what is timed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = PGTGVecEnv(n, device=0, autoreset=True, max_episode_steps=100, **kw)
    res = {}
    for name, extra in (("without_cost_limit", {}), ("with_cost_limit", dict(cost_limit=1.0))):
        ro = env.rollout(T, **extra)
        g = torch.Generator(device="cuda").manual_seed(2)
        ro.begin(seed=0)
        ro.rewards.copy_(torch.randn(T, n, device="cuda", generator=g))
        ro.values.copy_(torch.randn(T, n, device="cuda", generator=g))
        ro.dones.copy_(torch.rand(T + 1, n, device="cuda", generator=g) < 0.02)
        if extra:
            ro.costs.copy_((torch.rand(T, n, device="cuda", generator=g) < 0.1).to(torch.float32))
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
