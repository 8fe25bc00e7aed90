"""The evaluation kernels alone (include/pgtg.h pgtg_eval_step, pgtg_eval_summary): k_eval through
Evaluation.record_from on synthetic streams, bit for bit against evaluate_reference at the wave and workgroup
edges and at quotas of zero, one and mixed; the recorded reference fixture replayed; k_eval_reduce against
numpy on the same records."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

T = 24
NS = (1, 63, 64, 65, 255, 256, 257, 513)   # partial waves, whole and partial workgroups, more than one workgroup
GAMMAS = (1.0, 0.99)
FIXTURE = os.path.join(helpers.ROOT, "tests", "golden", "eval_reference.npz")


def _episode_counts(N):
    return (N // 2, N, 2 * N + 37)  # quotas of 0 and 1; all 1; mixed 2 and 3 (N = 1: 39)


@pytest.fixture(scope="module")
def envs():
    """envs(n): the module's one env of n envs, made at first use."""
    cache = {}

    def get(n):
        if n not in cache:
            from pgtg_amd.vector import PGTGVecEnv
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                cache[n] = PGTGVecEnv(n, device=0, random_map_width=3, random_map_height=3, max_episode_steps=9)
        return cache[n]
    yield get
    for e in cache.values():
        e.close()


def _streams(N, seed):
    """[T, N] reward, terminated, truncated: env 0 finishes on consecutive steps (2 .. 8), step 5 has both
    flags set on every third env, the last env (N >= 2) never finishes, the rest end episodes at random."""
    rng = np.random.default_rng(seed)
    rew = rng.normal(size=(T, N)) * 50 - 20
    term = rng.random((T, N)) < 0.2
    trunc = rng.random((T, N)) < 0.1
    term[2:9, 0] = True
    trunc[2:9, 0] = False
    term[5, ::3] = True
    trunc[5, ::3] = True
    if N >= 2:
        term[:, N - 1] = False
        trunc[:, N - 1] = False
    return rew, term, trunc


def _replay(evaluation, rew, term, trunc, check_open=None):
    """record_from over the rows of device copies of the streams."""
    d_rew = torch.as_tensor(np.ascontiguousarray(rew, dtype=np.float64)).cuda()
    d_term = torch.as_tensor(np.ascontiguousarray(term).astype(bool)).cuda()
    d_trunc = torch.as_tensor(np.ascontiguousarray(trunc).astype(bool)).cuda()
    evaluation.clear()
    for s in range(rew.shape[0]):
        evaluation.record_from(d_rew[s], d_term[s], d_trunc[s])
        if check_open is not None:
            assert evaluation.open_envs() == check_open[s], f"open envs after step {s}"
    torch.cuda.synchronize()
    return d_rew, d_term, d_trunc


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _same_records(got, want):
    for name in ("rec_return", "rec_discounted", "rec_length", "rec_last_reward", "rec_end_step", "rec_flags",
                 "cnt", "ret", "disc", "g", "len"):
        assert got[name].dtype == want[name].dtype, name
        assert np.array_equal(_bits(got[name]), _bits(want[name])), name


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("which", (0, 1, 2))
@pytest.mark.parametrize("N", NS)
def test_k_eval_matches_the_restatement_bit_for_bit(envs, N, which, gamma):
    from pgtg_amd import evaluate as ev
    n_episodes = _episode_counts(N)[which]
    env = envs(N)
    if n_episodes < 1:  # (N = 1: N // 2 episodes is no evaluation)
        with pytest.raises(ValueError):
            env.evaluation(n_episodes, gamma)
        return
    rew, term, trunc = _streams(N, 1000 * N + which)
    want = ev.evaluate_reference(rew, term, trunc, n_episodes, gamma)
    finishes = (term | trunc).sum(axis=0)
    # what the streams must hold for the case to mean something
    assert (term[2:9, 0] | trunc[2:9, 0]).all() and (term[5] & trunc[5]).any()
    if which == 1 or N > 1:
        assert (finishes > want["quota"]).any()  # envs that finish more episodes than their quota
    if which == 0:
        assert (want["quota"] == 0).any()
    e = env.evaluation(n_episodes, gamma)
    _replay(e, rew, term, trunc, check_open=want["open_per_step"])
    got = e.records()
    _same_records(got, want)
    assert e.open_envs() == want["open_envs"]
    assert (got["cnt"] <= want["quota"]).all() and not got["cnt"][want["quota"] == 0].any()
    if N >= 2:  # the env that never finishes stays open, and its running episode is in no record
        assert want["quota"][N - 1] >= 1 and e.open_envs() > 0 and got["cnt"][N - 1] == 0
        assert got["len"][N - 1] == T and N - 1 not in set(e.episodes()["env"])
    eps, weps = e.episodes(), want["episodes"]
    for k in weps:
        assert np.array_equal(_bits(eps[k]), _bits(weps[k])), k
    assert env.error_count()[0] == 0


@pytest.mark.parametrize("N, which, gamma", [(1, 2, 0.99), (65, 0, 0.99), (257, 2, 1.0), (513, 1, 0.99), (513, 2, 0.99)])
def test_summary_against_numpy_on_the_same_records(envs, N, which, gamma):
    """Counts and extrema exactly; each mean and std within n 2^-52 max|x| of numpy's on the device's own
    records (the fp64 summation error of n terms, in either order); two calls give the same bits."""
    from pgtg_amd import evaluate as ev
    n_episodes = _episode_counts(N)[which]
    rew, term, trunc = _streams(N, 77 * N + which)
    e = envs(N).evaluation(n_episodes, gamma)
    _replay(e, rew, term, trunc)
    eps = e.episodes()
    want = ev.summarize(eps, int((e.records()["cnt"] < e.quota).sum()))
    s1, s2 = e.summary(), e.summary()
    n = want["episodes"]
    assert n > 0
    for k in ("episodes", "open_envs", "terminated", "truncated_only", "last_reward_positive", "last_reward_negative",
              "negative_discounted", "length_sum", "length_min", "length_max", "return_min", "return_max"):
        assert s1[k] == want[k], k
    for stem, key in (("return", "returns"), ("discounted", "discounted")):
        tol = n * 2.0 ** -52 * float(np.abs(eps[key]).max())
        for stat in ("_mean", "_std"):
            err = abs(s1[stem + stat] - want[stem + stat])
            print(f"N={N} n={n} {stem + stat}: device={s1[stem + stat]!r} numpy={want[stem + stat]!r} err={err:.3e} tol={tol:.3e}")
            assert err <= tol, stem + stat
    assert s1.keys() == s2.keys()
    for k in s1:
        assert np.array_equal(_bits(np.array([s1[k]], dtype=np.float64)), _bits(np.array([s2[k]], dtype=np.float64))), k


def test_summary_without_episodes(envs):
    e = envs(65).evaluation(65, 0.99)
    e.clear()
    s = e.summary()
    assert s["episodes"] == 0 and s["open_envs"] == 65 and s["length_sum"] == 0 and s["length_max"] == 0
    assert s["length_min"] == 2 ** 31 - 1 and s["return_min"] == float("inf") and s["return_max"] == float("-inf")
    assert all(s[k] is None for k in ("return_mean", "return_std", "discounted_mean", "discounted_std"))
    assert e.open_envs() == 65


@pytest.mark.parametrize("N", (1, 257))
def test_reference_fixture_replayed(envs, N):
    """The stream the reference's ModularEvaluator saw, as every env's stream: its counters, N times."""
    z = np.load(FIXTURE)
    number, gamma = int(z["number"]), float(z["GAMMA"])
    terminated, truncated, over_max, negative = (int(x) for x in z["counters"])
    tile = lambda a: np.repeat(np.asarray(a)[:, None], N, axis=1)  # noqa: E731
    e = envs(N).evaluation(number * N, gamma)
    _replay(e, tile(z["rewards"]), tile(z["terminated"]), tile(z["truncated"]))
    s = e.summary()
    assert over_max == 0
    assert (s["episodes"], s["open_envs"]) == (number * N, 0) and e.open_envs() == 0
    assert (s["terminated"], s["truncated_only"], s["negative_discounted"]) == (terminated * N, truncated * N, negative * N)
    ends = np.nonzero(z["terminated"] | z["truncated"])[0]
    wins, losses = int((z["rewards"][ends] > 0).sum()), int((z["rewards"][ends] < 0).sum())
    assert wins >= 1 and losses >= 1 and (s["last_reward_positive"], s["last_reward_negative"]) == (wins * N, losses * N)
    disc = e.records()["rec_discounted"]
    assert disc.shape == (number, N) and (disc == disc[:, :1]).all()
    bounds = np.r_[z["episode_start"], len(z["rewards"])]
    for i in range(number):  # each discounted return within the bound derived in tests/test_evaluate_cpu.py
        r = z["rewards"][bounds[i]:bounds[i + 1]]
        bound = (len(r) + 2) * 2.0 ** -52 * float(np.sum(np.abs(r) * gamma ** np.arange(len(r))))
        assert abs(float(disc[i, 0]) - float(z["returns"][i])) <= bound


def test_invalid_arguments_launch_nothing(envs):
    from pgtg_amd import _abi
    env = envs(65)
    e = env.evaluation(100, 0.99)
    e.clear()
    before = e.records()
    lib = env._lib

    def call(**changes):
        a = _abi.PgtgEval.from_buffer_copy(bytes(e._args))
        for k, v in changes.items():
            setattr(a, k, v)
        return lib.pgtg_eval_step(env._h, C.byref(a))

    assert call() == _abi.PGTG_OK
    torch.cuda.synchronize()
    after_one = e.records()
    for changes in (dict(n=64), dict(n_episodes=0), dict(gamma=1.5), dict(gamma=-0.1), dict(gamma=float("nan")),
                    dict(reward=None), dict(cnt=None), dict(rec_flags=None), dict(open_rows=None), dict(step=2 ** 31)):
        assert call(**changes) == _abi.PGTG_E_INVALID, changes
        assert lib.pgtg_last_error(env._h)
    ws, out = C.c_void_p(e._workspace.data_ptr()), C.c_void_p(e._summary.data_ptr())
    assert lib.pgtg_eval_summary(env._h, C.byref(e._args), None, ws) == _abi.PGTG_E_INVALID
    assert lib.pgtg_eval_summary(env._h, C.byref(e._args), out, None) == _abi.PGTG_E_INVALID
    nbytes = C.c_uint64()
    assert lib.pgtg_eval_workspace_bytes(0, 1, C.byref(nbytes)) == _abi.PGTG_E_INVALID
    torch.cuda.synchronize()
    now = e.records()
    for k in now:
        assert np.array_equal(_bits(now[k]), _bits(after_one[k])), k
    assert before["len"].sum() == 0 and after_one["len"].sum() == 65
