"""The device digest formula (pgtg_amd/digest.py, torch) equals the restatement's
(oracle/pgtg_oracle.c orc_rollout_digest, C) on the same outputs, so the exhaustive GPU parity tests
can compare whole batches digest by digest.  Runs on CPU tensors (no GPU needed).

With a time limit (orc_rollout_digest_tl, gymnasium's TimeLimit over same-step auto-reset) the Python
side counts the steps since each env's last reset itself around OracleEnv.step / reset(None): the
independent restatement of the C loop that tests/test_gpu_truncation.py compares the kernels with."""
import ctypes as C
import hashlib
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers
from oracle import oracle
from oracle.oracle import OracleEnv
from pgtg_amd import config as cfg
from pgtg_amd.digest import Digest, car_term

M64 = (1 << 64) - 1
N, T, OFF, SEED = 24, 30, 1000, 0xA11CE


def action(seed: int, t: int, g: int) -> int:
    z = seed ^ ((t * 0x9E3779B97F4A7C15) & M64) ^ ((g * 0xD1B54A32D192ED03) & M64)
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return ((z >> 32) * 9) >> 32


CONFIGS = [
    dict(random_map_width=3, random_map_height=3),
    dict(random_map_width=4, random_map_height=4, use_next_subgoal_direction=True, separate_reward_cost=True,
         random_map_obstacle_probability=0.5, standing_still_penalty=0.5),
    dict(random_map_width=3, random_map_height=3, traffic_density=0.3, use_sliding_observation_window=True),
    dict(random_map_width=4, random_map_height=3, traffic_density=0.5),
]
LIMITS = [1, 3, 7]


def _check_formula(kw, L):
    """Digest (torch) over outputs stepped here env by env == rollout_digest(max_episode_steps=L) at
    every step; returns the oracle's flags after checking them against the flags counted here."""
    spec = cfg.make_spec(**kw)
    ref, flags = oracle.rollout_digest(spec, N, T, SEED, env_offset=OFF, threads=2, max_episode_steps=L, flags_out=True)
    envs = [OracleEnv(spec) for _ in range(N)]
    first = [e.reset(OFF + i) for i, e in enumerate(envs)]
    D = first[0]["obs"].size
    fake = SimpleNamespace(device=torch.device("cpu"), obs_map=torch.zeros((N,) + first[0]["obs"].shape, dtype=torch.uint8))
    dg = Digest(fake)
    assert dg.D == D
    elapsed = [0] * N  # steps since the env's last reset
    for t in range(T):
        rs, fin = [], np.zeros((N,) + first[0]["obs"].shape, np.uint8)
        for i, e in enumerate(envs):
            r = e.step(action(SEED, t, OFF + i))
            assert not r["truncated"]  # (the single env knows no time limit: TimeLimit wraps it)
            elapsed[i] += 1
            trunc = L > 0 and elapsed[i] >= L  # gymnasium TimeLimit, also on a terminating step
            if r["terminated"] or trunc:
                fin[i] = r["obs"]
                nr = e.reset(None)
                elapsed[i] = 0
                r = dict(nr, reward=r["reward"], cost=r["cost"], terminated=r["terminated"])
            rs.append(dict(r, truncated=trunc))
        fake.obs_map = torch.as_tensor(np.stack([r["obs"] for r in rs]))
        fake.final_map = torch.as_tensor(fin)
        fake.position = torch.tensor([r["pos"] for r in rs], dtype=torch.int32)
        fake.velocity = torch.tensor([r["vel"] for r in rs], dtype=torch.int32)
        fake.reward = torch.tensor([r["reward"] for r in rs], dtype=torch.float64)
        fake.terminated = torch.tensor([r["terminated"] for r in rs])
        fake.truncated = torch.tensor([r["truncated"] for r in rs])
        fake.nsd = torch.tensor([r["nsd"] for r in rs], dtype=torch.int32) if spec.next_subgoal else None
        fake.cost = torch.tensor([r["cost"] for r in rs], dtype=torch.float64) if spec.separate_reward_cost else None
        fake.has_cars = spec.traffic_density > 0
        terms = [car_term(e.cars()) for e in envs]
        fake.car_digest = lambda: torch.tensor(np.array(terms, dtype=np.uint64).view(np.int64))
        got = dg.step_digest().numpy().view(np.uint64)
        assert np.array_equal(got, ref[t]), f"t{t}: {np.nonzero(got != ref[t])[0][:5]}"
        want_flags = np.array([int(r["terminated"]) | int(r["truncated"]) << 1 for r in rs], np.uint8)
        assert np.array_equal(flags[t], want_flags), f"t{t} flags"
    return flags


@pytest.mark.parametrize("kw", CONFIGS)
def test_digest_formula_matches_oracle(kw):
    flags = _check_formula(kw, 0)
    assert not (flags & 2).any() and (flags & 1).any()


@pytest.mark.parametrize("L", LIMITS)
@pytest.mark.parametrize("kw", CONFIGS)
def test_digest_formula_matches_oracle_truncated(kw, L):
    flags = _check_formula(kw, L)
    assert (flags == 2).any(), "no env was truncated without terminating"
    if L == 1:
        assert ((flags & 2) != 0).all()  # every step of every env ends its episode
    else:
        # an episode never outlasts the limit: every run of L steps of an env holds a done step
        done = flags != 0
        for t in range(T - L + 1):
            assert done[t:t + L].any(0).all(), t
        assert (flags == 1).any(), "no env terminated before its limit"


def test_truncated_cases_reach_every_flag_combination():
    """Across the parametrisation above: truncated only, terminated only, and both on one step."""
    seen = set()
    for kw in CONFIGS:
        for L in LIMITS:
            _, flags = oracle.rollout_digest(cfg.make_spec(**kw), N, T, SEED, env_offset=OFF, max_episode_steps=L,
                                             flags_out=True)
            seen |= set(np.unique(flags).tolist())
    assert seen == {0, 1, 2, 3}, seen


def _sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("k", range(len(CONFIGS)))
def test_no_limit_reproduces_the_digests_from_before_the_time_limit(k):
    """max_episode_steps = 0 and any limit beyond the rollout's length leave every digest as it was
    before the rollout knew a time limit: equal to the old entry point, to each other, and to the
    digests recorded from the oracle of that time (tests/golden/digest_no_limit.json, sha256 of the
    [T, N] uint64 array)."""
    spec = cfg.make_spec(**CONFIGS[k])
    ref, flags = oracle.rollout_digest(spec, N, T, SEED, env_offset=OFF, flags_out=True)
    assert not (flags & 2).any()
    c = oracle.config_from_spec(spec)
    old = np.zeros((T, N), np.uint64)
    assert oracle.lib().orc_rollout_digest(C.byref(c), N, OFF, T, SEED, old.ctypes.data) == 0
    assert np.array_equal(old, ref)
    for L in (T + 1, 10 ** 6):
        got, f = oracle.rollout_digest(spec, N, T, SEED, env_offset=OFF, max_episode_steps=L, flags_out=True)
        assert np.array_equal(got, ref) and np.array_equal(f, flags), L
    # the limit reached on the last step only: that step's truncated bit and nothing before it
    got, f = oracle.rollout_digest(spec, N, T, SEED, env_offset=OFF, max_episode_steps=T, flags_out=True)
    assert np.array_equal(got[:T - 1], ref[:T - 1]) and np.array_equal(f[:T - 1], flags[:T - 1])
    with open(os.path.join(helpers.GOLDEN, "digest_no_limit.json")) as fh:
        rec = json.load(fh)
    assert rec["n_envs"] == N and rec["steps"] == T and rec["env_offset"] == OFF and rec["act_seed"] == SEED
    assert _sha(ref) == rec["sha256"][k]
