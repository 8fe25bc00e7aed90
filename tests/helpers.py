"""Shared test helpers: golden-fixture loading and vectorised replay of the CPU oracle."""
from __future__ import annotations

import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TESTDATA = os.path.join(ROOT, "tests", "golden", "maps")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pgtg_amd.config import add_rule, make_spec  # noqa: E402


def load_traj(name: str, sub: str = "") -> dict:
    """sub: a folder below tests/golden ("fuzz")"""
    z = np.load(os.path.join(GOLDEN, sub, f"traj_{name}.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(bytes(d["meta"]).decode())
    return d


def traj_names(sub: str = "") -> list[str]:
    return sorted(f[5:-4] for f in os.listdir(os.path.join(GOLDEN, sub)) if f.startswith("traj_"))


def spec_for(meta: dict):
    kw = dict(meta["kwargs"])
    for k in ("random_map_start_position", "random_map_goal_position", "traffic_light_phases_duration"):
        if isinstance(kw.get(k), list):
            kw[k] = tuple(kw[k])
    mp = os.path.join(TESTDATA, meta["map_file"]) if meta["map_file"] else None
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec = make_spec(mp, **kw)
    if "rules" in meta:  # a case with its own traffic rules (tools/gen_golden.py RULE_CASES)
        spec.rules = []
        for r in meta["rules"]:
            add_rule(spec, r)
    return spec


def digest(arr) -> int:
    return zlib.crc32(np.ascontiguousarray(arr, dtype=np.int32).tobytes())


def channel_perm(spec, keys: list[str]) -> list[int]:
    """index into our channel order for each golden key"""
    ours = [k for k, _ in spec.channels]
    return [ours.index(k) for k in keys]


def replay_oracle(d: dict, n_envs: int | None = None, steps: int | None = None) -> list[str]:
    """Replay the golden trajectory through the CPU oracle; return a list of mismatch strings."""
    from oracle.oracle import OracleEnv
    meta = d["meta"]
    spec = spec_for(meta)
    perm = channel_perm(spec, meta["keys"])
    N = meta["N"] if n_envs is None else min(n_envs, meta["N"])
    T = meta["T"] if steps is None else min(steps, meta["T"])
    reset_map = {(int(t), int(i)): k for k, (t, i) in enumerate(d["reset_idx"])}
    bad: list[str] = []
    for i in range(N):
        env = OracleEnv(spec)
        r = env.reset(meta["seed_base"] + i)
        if not np.array_equal(r["obs"][perm], d["init_obs"][i]):
            bad.append(f"env{i} reset obs")
        if tuple(r["pos"]) != tuple(d["init_pos"][i]):
            bad.append(f"env{i} reset pos")
        if digest(env.cars()) != int(d["init_cars_dig"][i]):
            bad.append(f"env{i} reset cars")
        for t in range(T):
            r = env.step(int(d["actions"][t, i]))
            tag = f"env{i} t{t}"
            if not np.array_equal(r["obs"][perm], d["obs"][t, i]):
                diff = [meta["keys"][c] for c in range(len(perm)) if not np.array_equal(r["obs"][perm[c]], d["obs"][t, i, c])]
                bad.append(f"{tag} obs {diff}")
            if tuple(r["pos"]) != tuple(d["pos"][t, i]) or tuple(r["vel"]) != tuple(d["vel"][t, i]):
                bad.append(f"{tag} pos/vel {r['pos']} {r['vel']} vs {d['pos'][t, i]} {d['vel'][t, i]}")
            if r["reward"] != d["reward"][t, i] or r["cost"] != d["cost"][t, i]:
                bad.append(f"{tag} reward {r['reward']} vs {d['reward'][t, i]}")
            if r["terminated"] != bool(d["terminated"][t, i]):
                bad.append(f"{tag} terminated")
            if spec.next_subgoal and r["nsd"] != d["nsd"][t, i]:
                bad.append(f"{tag} nsd {r['nsd']} vs {d['nsd'][t, i]}")
            if bool(r["braking"]) != bool(d["braking"][t, i]):
                bad.append(f"{tag} braking")
            if "triggered" in d and int(r["braking"]) != int(d["triggered"][t, i]):
                bad.append(f"{tag} triggered rules {int(r['braking']):#04x} vs {int(d['triggered'][t, i]):#04x}")
            if digest(env.cars()) != int(d["cars_dig"][t, i]):
                bad.append(f"{tag} cars")
            if r["terminated"]:
                k = reset_map[(t, i)]
                r = env.reset(None)
                if not np.array_equal(r["obs"][perm], d["reset_obs"][k]):
                    bad.append(f"{tag} autoreset obs")
                if tuple(r["pos"]) != tuple(d["reset_pos"][k]):
                    bad.append(f"{tag} autoreset pos")
                if digest(env.cars()) != int(d["reset_cars_dig"][k]):
                    bad.append(f"{tag} autoreset cars")
            if len(bad) > 20:
                return bad
    return bad


def has_traffic(meta: dict) -> bool:
    return float(meta["kwargs"].get("traffic_density", 0) or 0) > 0


def _compare_tick(env, d: dict, spec, perm, ix, planted: bool, t: int, reset_map: dict, bad: list) -> None:
    """The handle's outputs after tick t against the trajectory's, at the envs ix: mismatch strings appended
    to bad.  (replay_vec's comparison of a step, whether the tick was a launch of its own or the last of a
    pgtg_step_many call.)"""
    import torch
    meta, N = d["meta"], len(ix)
    torch.cuda.synchronize()
    m = env.obs_map.cpu().numpy()[ix][:, perm]
    fm = env.final_map.cpu().numpy()[ix][:, perm]
    pos, vel = env.position.cpu().numpy()[ix], env.velocity.cpu().numpy()[ix]
    fpos, fvel = env.final_position.cpu().numpy()[ix], env.final_velocity.cpu().numpy()[ix]
    rew, term = env.reward.cpu().numpy()[ix], env.terminated.cpu().numpy()[ix]
    trunc = env.truncated.cpu().numpy()[ix]
    cost = env.cost.cpu().numpy()[ix] if env.cost is not None else np.zeros(N)
    brk = env.braking.cpu().numpy()[ix]
    nsd = env.nsd.cpu().numpy()[ix] if env.nsd is not None else None
    fnsd = env.final_nsd.cpu().numpy()[ix] if env.final_nsd is not None else None
    check_cars = has_traffic(meta)
    for i, b in enumerate(ix):
        tag = f"env{i}@{b} t{t}" if planted else f"env{i} t{t}"
        if check_cars:
            dig = digest(env.cars(b))
            want = d["reset_cars_dig"][reset_map[(t, i)]] if term[i] and (t, i) in reset_map else d["cars_dig"][t, i]
            if dig != int(want):
                bad.append(f"{tag} cars")
        if bool(term[i]) != bool(d["terminated"][t, i]) or trunc[i]:
            bad.append(f"{tag} terminated {term[i]} vs {d['terminated'][t, i]}")
            continue
        if bool(brk[i]) != bool(d["braking"][t, i]):
            bad.append(f"{tag} braking {brk[i]} vs {d['braking'][t, i]}")
        if "triggered" in d and int(brk[i]) != int(d["triggered"][t, i]):
            bad.append(f"{tag} triggered rules {int(brk[i]):#04x} vs {int(d['triggered'][t, i]):#04x}")
        if rew[i] != d["reward"][t, i] or cost[i] != d["cost"][t, i]:
            bad.append(f"{tag} reward {rew[i]} vs {d['reward'][t, i]} cost {cost[i]} vs {d['cost'][t, i]}")
        if term[i]:
            if not np.array_equal(fm[i], d["obs"][t, i]):
                bad.append(f"{tag} final obs")
            if tuple(fpos[i]) != tuple(d["pos"][t, i]) or tuple(fvel[i]) != tuple(d["vel"][t, i]):
                bad.append(f"{tag} final pos/vel")
            if fnsd is not None and fnsd[i] != d["nsd"][t, i]:
                bad.append(f"{tag} final nsd")
            k = reset_map[(t, i)]
            if not np.array_equal(m[i], d["reset_obs"][k]):
                bad.append(f"{tag} autoreset obs")
            if tuple(pos[i]) != tuple(d["reset_pos"][k]):
                bad.append(f"{tag} autoreset pos")
            if nsd is not None and nsd[i] != d["reset_nsd"][k]:
                bad.append(f"{tag} autoreset nsd")
        else:
            if not np.array_equal(m[i], d["obs"][t, i]):
                diff = [meta["keys"][c] for c in range(len(perm)) if not np.array_equal(m[i, c], d["obs"][t, i, c])]
                bad.append(f"{tag} obs {diff}")
            if tuple(pos[i]) != tuple(d["pos"][t, i]) or tuple(vel[i]) != tuple(d["vel"][t, i]):
                bad.append(f"{tag} pos/vel {pos[i]} {vel[i]} vs {d['pos'][t, i]} {d['vel'][t, i]}")
            if nsd is not None and nsd[i] != d["nsd"][t, i]:
                bad.append(f"{tag} nsd {nsd[i]} vs {d['nsd'][t, i]}")
        if len(bad) > 30:
            return


def replay_vec(d: dict, n_envs: int | None = None, steps: int | None = None, n_batch: int | None = None,
               at=None, tune: dict | None = None, info: dict | None = None, chunks=None) -> list[str]:
    """Replay a golden trajectory through the HIP vector env (auto-reset); mismatch strings.

    n_batch, at: plant the fixture's envs in a batch of n_batch envs, env j at batch index at[j].  The
    batch is reset with one seed per env: seed_base + j at at[j], a filler seed (fixed rng, far above
    every fixture's seeds) everywhere else; the fillers step with fixed random actions.  Every
    comparison is made at the planted indices.  tune: PGTGVecEnv's.  info (dict): gets "step_kernel"
    and, after the last step, "errors" (error_count()[0]).
    chunks (list of call lengths that sum to the steps): instead of a step per tick, one step_many call per
    chunk over resident [len, batch] action tensors, the comparison made after the last tick of each call;
    info also gets "calls", "step_launches" (the step-kernel launches the calls took) and "end_ticks"."""
    import torch
    from pgtg_amd.vector import PGTGVecEnv
    meta = d["meta"]
    spec = spec_for(meta)
    perm = channel_perm(spec, meta["keys"])
    N = meta["N"] if n_envs is None else min(n_envs, meta["N"])
    T = meta["T"] if steps is None else min(steps, meta["T"])
    planted = n_batch is not None or at is not None
    ix = list(range(N)) if at is None else [int(b) for b in at][:N]
    B = N if n_batch is None else int(n_batch)
    assert len(ix) == N and len(set(ix)) == N and all(0 <= b < B for b in ix), (ix, N, B)
    if chunks is not None:
        chunks = [int(k) for k in chunks]
        assert all(k >= 1 for k in chunks) and sum(chunks) == T, (chunks, T)
    env = PGTGVecEnv(B, spec=spec, autoreset=True, tune=tune)
    bad: list[str] = []
    try:
        if info is not None:
            info["step_kernel"] = env.step_kernel()
        if planted:
            rng = np.random.default_rng(0xF177)
            seeds = (1_000_003 + rng.integers(0, 2**31, B)).tolist()
            for j, b in enumerate(ix):
                seeds[b] = meta["seed_base"] + j
            filler = rng.integers(0, 9, (T, B)).astype(np.uint8)
            obs, _ = env.reset(seed=seeds)
        else:
            obs, _ = env.reset(seed=meta["seed_base"])
        torch.cuda.synchronize()
        m = env.obs_map.cpu().numpy()[ix][:, perm]
        pos = env.position.cpu().numpy()[ix]
        nsd = env.nsd.cpu().numpy()[ix] if env.nsd is not None else None
        for i, b in enumerate(ix):
            tag = f"env{i}@{b}" if planted else f"env{i}"
            if has_traffic(meta) and digest(env.cars(b)) != int(d["init_cars_dig"][i]):
                bad.append(f"{tag} reset cars")
            if not np.array_equal(m[i], d["init_obs"][i]):
                bad.append(f"{tag} reset obs")
            if tuple(pos[i]) != tuple(d["init_pos"][i]):
                bad.append(f"{tag} reset pos {pos[i]} vs {d['init_pos'][i]}")
            if spec.next_subgoal and int(nsd[i]) != int(d["init_nsd"][i]):
                bad.append(f"{tag} reset nsd")
        reset_map = {(int(t), int(i)): k for k, (t, i) in enumerate(d["reset_idx"])}

        def actions(t):
            if planted:
                a = filler[t].copy()
                a[ix] = d["actions"][t, :N]
                return a
            return d["actions"][t, :N].astype(np.uint8)

        if chunks is None:
            for t in range(T):
                env.step(torch.as_tensor(actions(t).astype(np.uint8)).cuda())
                _compare_tick(env, d, spec, perm, ix, planted, t, reset_map, bad)
                if len(bad) > 30:
                    return bad
        else:
            acts = torch.as_tensor(np.stack([actions(t).astype(np.uint8) for t in range(T)])).cuda()
            l0, t0, ends = env.step_launches(), 0, []
            for k in chunks:
                env.step_many(acts[t0:t0 + k])
                t0 += k
                ends.append(t0 - 1)
                _compare_tick(env, d, spec, perm, ix, planted, t0 - 1, reset_map, bad)
                if len(bad) > 30:
                    return bad
            if info is not None:
                info.update(calls=len(chunks), step_launches=env.step_launches() - l0, end_ticks=ends)
        if info is not None:
            info["errors"] = int(env.error_count()[0])
    finally:
        env.close()
    return bad


def vec_vs_oracle(vec, spec_orc, n, steps, seed, rng, tag, envs=None, stats=None, orcs=None):
    """Autoreset batch vs per-env oracles: reward, termination, observation and braking mask.  The
    oracles are reset with seed + i, the batch is expected to have been.  `envs`: the env indices to
    compare (default all n).  `stats` (dict): gets per-rule firing counts ("rule", 8 ints) and the
    number of compared steps with two or more rules ("multi") added.  `orcs` (dict env -> OracleEnv):
    oracles of an earlier call to carry on with (an empty dict is filled).  Returns the steps that braked."""
    import torch
    from oracle.oracle import OracleEnv
    envs = list(range(n)) if envs is None else list(envs)
    if not orcs:
        orcs = {} if orcs is None else orcs
        for i in envs:
            orcs[i] = OracleEnv(spec_orc)
            orcs[i].reset(seed + i)
    fired = 0
    for t in range(steps):
        acts = rng.integers(0, 9, n).astype(np.uint8)
        vec.step(torch.as_tensor(acts))
        torch.cuda.synchronize()
        m, rew = vec.obs_map.cpu().numpy(), vec.reward.cpu().numpy()
        term, mask = vec.terminated.cpu().numpy(), vec.braking.cpu().numpy()
        for i, o in orcs.items():
            r = o.step(int(acts[i]))
            assert rew[i] == r["reward"] and bool(term[i]) == r["terminated"], f"{tag} t{t} env{i}"
            assert int(mask[i]) == int(r["braking"]), f"{tag} t{t} env{i} braking"
            fired += int(mask[i] != 0)
            if stats is not None:
                b = int(r["braking"])
                stats.setdefault("rule", [0] * 8)
                for k in range(8):
                    stats["rule"][k] += (b >> k) & 1
                stats["multi"] = stats.get("multi", 0) + int(bin(b).count("1") >= 2)
            if r["terminated"]:
                r = o.reset(None)
            assert np.array_equal(m[i], r["obs"]), f"{tag} t{t} env{i} obs"
    return fired
