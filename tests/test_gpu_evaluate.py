"""Evaluation end to end on the device: DevicePolicy acting, the tick and k_eval over a real batch, against
evaluate_reference on the streams the steps produced; run(), evaluate_policy and the error paths."""
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401

pytestmark = pytest.mark.gpu

N, N_EPISODES, LIMIT, SEED = 300, 637, 9, 4242   # quotas of 2 and 3; every quota met within 3 * 9 = 27 steps
KW = dict(random_map_width=3, random_map_height=3, traffic_density=0.2)


def _vec(n, **kw):
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PGTGVecEnv(n, device=0, **kw)


def _policy(env, seed=0):
    from pgtg_amd.policy import DevicePolicy, MlpPolicyReference
    policy = DevicePolicy(env)
    torch.manual_seed(seed)
    policy.load_state_dict(MlpPolicyReference(policy.obs_dim).state_dict())
    return policy


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


RECORDS = ("rec_return", "rec_discounted", "rec_length", "rec_last_reward", "rec_end_step", "rec_flags", "cnt")


@pytest.fixture(scope="module")
def setup():
    """The env, the policy, and the manual loop's result: the device records next to evaluate_reference of the
    streams copied out step by step.  Computed once; the tests leave it unchanged."""
    from pgtg_amd import evaluate as ev
    env = _vec(N, max_episode_steps=LIMIT, **KW)
    policy = _policy(env)
    e = env.evaluation(N_EPISODES, gamma=0.99)
    assert e.slots == 3 and set(e.quota) == {2, 3} and e.max_steps == 27
    obs = e.begin(seed=SEED)
    rew, term, trunc = [], [], []
    for _ in range(e.max_steps):
        actions, _, _ = policy.act(obs, deterministic=True)
        e.step(actions)
        rew.append(env.reward.cpu().numpy().copy())
        term.append(env.terminated.cpu().numpy().copy())
        trunc.append(env.truncated.cpu().numpy().copy())
    manual = e.records()
    want = ev.evaluate_reference(np.stack(rew), np.stack(term), np.stack(trunc), N_EPISODES, 0.99)
    out = dict(env=env, policy=policy, evaluation=e, manual=manual, want=want, open_envs=e.open_envs(),
               episodes=e.episodes(), errors=env.error_count()[0])
    yield out
    e.close()
    env.close()


def test_manual_loop_equals_the_restatement(setup):
    got, want = setup["manual"], setup["want"]
    for name in RECORDS + ("ret", "disc", "g", "len"):
        assert got[name].dtype == want[name].dtype, name
        assert np.array_equal(_bits(got[name]), _bits(want[name])), name
    assert setup["open_envs"] == want["open_envs"] == 0  # every quota is met within the cap by construction
    assert np.array_equal(got["cnt"], want["quota"]) and got["cnt"].sum() == N_EPISODES
    eps = want["episodes"]
    print("terminated", int(eps["terminated"].sum()), "truncated only", int((eps["truncated"] & ~eps["terminated"]).sum()),
          "lengths", np.bincount(eps["lengths"]).tolist())
    assert eps["terminated"].any() and (eps["truncated"] & ~eps["terminated"]).any()  # both kinds of ending occur
    assert setup["errors"] == 0


@pytest.mark.parametrize("poll_every", (1, 16))
def test_run_gives_the_same_records(setup, poll_every):
    env, e = setup["env"], setup["evaluation"]
    kw = {} if poll_every == 16 else {"poll_every": poll_every}  # (16 is the default)
    steps = e.run(setup["policy"], seed=SEED, **kw)
    assert 1 <= steps <= e.max_steps
    got = e.records()
    for name in RECORDS:
        assert np.array_equal(_bits(got[name]), _bits(setup["manual"][name])), name
    assert e.open_envs() == 0
    s = e.summary()
    assert s["episodes"] == N_EPISODES and s["open_envs"] == 0
    if poll_every == 1:  # it stops at the step that closes the last env
        assert steps == int(setup["manual"]["rec_end_step"].max()) + 1
    assert env.error_count()[0] == 0


def test_evaluate_policy_is_sb3s(setup):
    from pgtg_amd.evaluate import evaluate_policy
    env, policy = setup["env"], setup["policy"]
    # the same episodes twice: an unseeded reset continues each env's seed sequence from the seeded one
    env.reset(seed=SEED + 1)
    returns, lengths = evaluate_policy(policy, env, n_eval_episodes=N_EPISODES, return_episode_rewards=True)
    env.reset(seed=SEED + 1)
    mean, std = evaluate_policy(policy, env, n_eval_episodes=N_EPISODES)
    assert len(returns) == len(lengths) == N_EPISODES and all(1 <= x <= LIMIT for x in lengths)
    tol = N_EPISODES * 2.0 ** -52 * max(abs(x) for x in returns)
    print(f"mean device={mean!r} numpy={np.mean(returns)!r}; std device={std!r} numpy={np.std(returns)!r}; tol={tol:.3e}")
    assert abs(mean - np.mean(returns)) <= tol and abs(std - np.std(returns)) <= tol
    # the lists come in (end_step, env) order: the order of an Evaluation's episodes() on the same episodes
    env.reset(seed=SEED + 1)
    e = env.evaluation(N_EPISODES, gamma=1.0)
    e.run(policy)
    eps = e.episodes()
    e.close()
    key = list(zip(eps["end_step"], eps["env"]))
    assert key == sorted(key) and len(set(key)) == N_EPISODES
    assert returns == [float(x) for x in eps["returns"]] and lengths == [int(x) for x in eps["lengths"]]
    assert env.error_count()[0] == 0


def test_error_paths_launch_nothing(setup):
    policy = setup["policy"]
    with pytest.raises(ValueError):
        setup["env"].evaluation(0)
    with pytest.raises(ValueError):
        setup["env"].evaluation(-3)
    frozen = _vec(4, autoreset=False, **KW)
    with pytest.raises(ValueError):
        frozen.evaluation(4)
    frozen.close()
    endless = _vec(4, **KW)  # no time limit
    e = endless.evaluation(4)
    assert e.max_steps is None
    p4 = _policy(endless)
    before = endless.counters()
    with pytest.raises(ValueError):
        e.run(p4)
    assert endless.counters() == before and e.t == 0
    assert e.run(p4, max_steps=3, seed=1) == 3  # (bounded by the caller: fine)
    e.close()
    endless.close()
    other = _vec(4, max_episode_steps=LIMIT, use_next_subgoal_direction=True, **KW)
    e = other.evaluation(4)
    assert e.obs_dim != policy.obs_dim
    before = other.counters()
    with pytest.raises(ValueError):
        e.run(policy)
    assert other.counters() == before and e.t == 0
    e.close()
    other.close()
