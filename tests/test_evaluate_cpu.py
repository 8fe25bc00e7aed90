"""pgtg_amd.evaluate without a GPU: the numpy restatement of k_eval against the fixture recorded from the
reference's ModularEvaluator (tests/golden/eval_reference.npz, tools/gen_eval_golden.py), SB3's per-env
quotas, the completion order of episodes(), and the ABI additions (layout, version)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import helpers
from pgtg_amd import _abi
from pgtg_amd import evaluate as ev

FIXTURE = os.path.join(helpers.ROOT, "tests", "golden", "eval_reference.npz")


@pytest.fixture(scope="module")
def fixture():
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def replay(fixture):
    """evaluate_reference on the logged stream as one env (N = 1, n_episodes = number)."""
    f = fixture
    return ev.evaluate_reference(f["rewards"][:, None], f["terminated"][:, None], f["truncated"][:, None],
                                 int(f["number"]), float(f["GAMMA"]))


def test_fixture_holds_what_the_checks_need(fixture):
    f = fixture
    terminated, truncated, over_max, negative = (int(x) for x in f["counters"])
    assert terminated >= 1 and truncated >= 1 and over_max == 0  # (the evaluator's own cut is out of scope)
    assert int(f["max_steps"]) > int(f["time_limit"])
    assert len(f["returns"]) == int(f["number"]) == len(f["episode_start"])
    # the logged boundaries are where the stream's flags end an episode
    ends = np.nonzero(f["terminated"] | f["truncated"])[0]
    assert np.array_equal(f["episode_start"][1:], ends[:-1] + 1) and f["episode_start"][0] == 0
    assert ends[-1] == len(f["rewards"]) - 1
    # every outcome the summary counts occurs and none is trivial: a goal-reaching episode (terminated with a
    # positive last reward, a positive discounted return), crashes and time-outs with negative ones
    last = f["rewards"][ends]
    assert (last > 0).any() and (last < 0).any()
    assert (f["terminated"][ends][last > 0] == 1).all()
    assert 1 <= negative < int(f["number"]) and (f["returns"] > 0).any() and (f["returns"] < 0).any()
    assert int(f["run_number"].sum()) == int(f["number"])


def test_reference_counters_exactly(fixture, replay):
    terminated, truncated, over_max, negative = (int(x) for x in fixture["counters"])
    s = replay["summary"]
    assert s["episodes"] == int(fixture["number"]) and s["open_envs"] == 0 and replay["open_envs"] == 0
    assert (s["terminated"], s["truncated_only"], s["negative_discounted"]) == (terminated, truncated, negative)
    assert over_max == 0
    # the last-reward outcome of Evaluator.evaluate (evaluator.py:117-129), from the stream itself
    ends = np.nonzero(fixture["terminated"] | fixture["truncated"])[0]
    last = fixture["rewards"][ends]
    assert s["last_reward_positive"] == int((last > 0).sum()) and s["last_reward_negative"] == int((last < 0).sum())
    assert s["last_reward_positive"] >= 1 and s["last_reward_negative"] >= 1
    # a "win" is an episode the reference returned a positive discounted return for (rewards before the goal are 0)
    assert s["last_reward_positive"] == int((fixture["returns"] > 0).sum())
    assert s["length_sum"] == len(fixture["rewards"])


def test_reference_discounted_returns_within_the_derived_bound(fixture, replay):
    """|ours - reference| <= (L + 2) 2^-52 sum_t |r_t| gamma^t per episode: the running product of at most L
    factors against np.power (<= 1 ulp each), one rounding per product and per sum."""
    f = fixture
    gamma = float(f["GAMMA"])
    eps = replay["episodes"]
    assert np.array_equal(eps["env"], np.zeros(len(eps["env"]), dtype=np.int64))
    bounds = np.r_[f["episode_start"], len(f["rewards"])]
    for i in range(int(f["number"])):
        r = f["rewards"][bounds[i]:bounds[i + 1]]
        L = len(r)
        assert eps["lengths"][i] == L and eps["end_step"][i] == bounds[i + 1] - 1
        bound = (L + 2) * 2.0 ** -52 * float(np.sum(np.abs(r) * gamma ** np.arange(L)))
        err = abs(float(eps["discounted"][i]) - float(f["returns"][i]))
        print(f"episode {i}: L={L} ours={eps['discounted'][i]!r} reference={f['returns'][i]!r} err={err:.3e} bound={bound:.3e}")
        assert err <= bound
        assert eps["returns"][i] == np.cumsum(r)[-1]  # (the undiscounted return: the same left-to-right sum)


@pytest.mark.parametrize("n_envs, n_episodes", [(8, 3), (8, 8), (8, 21), (300, 637), (1, 5), (257, 256)])
def test_quotas_are_sb3s(n_envs, n_episodes):
    q = ev.quotas(n_episodes, n_envs)
    assert q.sum() == n_episodes
    assert list(q) == [(n_episodes + i) // n_envs for i in range(n_envs)]  # evaluate_policy's episode_count_targets
    assert q.max() == ev.episode_slots(n_episodes, n_envs)
    assert (q == 0).any() == (n_episodes < n_envs)


def _streams(T, N, seed):
    rng = np.random.default_rng(seed)
    rew = rng.normal(size=(T, N)) * 10
    term = rng.random((T, N)) < 0.25
    trunc = rng.random((T, N)) < 0.15
    return rew, term, trunc


def test_envs_with_quota_zero_record_nothing():
    rew, term, trunc = _streams(12, 8, 0)
    out = ev.evaluate_reference(rew, term, trunc, 3, 0.99)
    assert list(out["quota"]) == [0, 0, 0, 0, 0, 1, 1, 1]
    assert not out["cnt"][:5].any() and not out["len"][:5].any() and not out["ret"][:5].any()
    assert (out["g"][:5] == 1.0).all()
    assert not out["rec_flags"][:, :5].any() and set(out["episodes"]["env"]) <= {5, 6, 7}
    assert (out["cnt"] <= out["quota"]).all()


@pytest.mark.parametrize("n_episodes", [5, 8, 21])
def test_episode_order_is_appending_per_step_in_env_order(n_episodes):
    """An independent loop in SB3's shape: per step, per env in env order, append if under the target."""
    T, N, gamma = 30, 8, 0.9
    rew, term, trunc = _streams(T, N, n_episodes)
    out = ev.evaluate_reference(rew, term, trunc, n_episodes, gamma)
    targets = [(n_episodes + i) // N for i in range(N)]
    counts, cur_r, cur_l = [0] * N, [0.0] * N, [0] * N
    want = []
    for s in range(T):
        for i in range(N):
            if counts[i] < targets[i]:
                cur_r[i] += rew[s, i]
                cur_l[i] += 1
                if term[s, i] or trunc[s, i]:
                    want.append((i, cur_r[i], cur_l[i], s, bool(term[s, i]), bool(trunc[s, i])))
                    counts[i] += 1
                    cur_r[i], cur_l[i] = 0.0, 0
    eps = out["episodes"]
    got = list(zip(eps["env"], eps["returns"], eps["lengths"], eps["end_step"], eps["terminated"], eps["truncated"]))
    assert [tuple(x) for x in got] == want
    assert out["summary"]["episodes"] == len(want) == sum(counts)
    assert out["open_envs"] == sum(c < t for c, t in zip(counts, targets))
    assert out["summary"]["truncated_only"] == sum(1 for w in want if w[5] and not w[4])


def test_summary_is_none_without_episodes():
    out = ev.evaluate_reference(np.ones((3, 4)), np.zeros((3, 4)), np.zeros((3, 4)), 4, 1.0)
    s = out["summary"]
    assert s["episodes"] == 0 and s["open_envs"] == 4 and s["return_mean"] is None and s["discounted_std"] is None
    assert (out["ret"] == 3.0).all() and (out["len"] == 3).all()


def test_abi_layout_and_version():
    src = open(os.path.join(helpers.ROOT, "include", "pgtg.h")).read()
    assert re.search(r"^#define PGTG_ABI_VERSION 9$", src, re.M) and _abi.PGTG_ABI_VERSION == 9
    for name in ("pgtg_eval_step", "pgtg_eval_summary", "pgtg_eval_workspace_bytes"):
        assert name in _abi.EXPORTED
    structs = {"PgtgEval": _abi.PgtgEval, "PgtgEvalSummary": _abi.PgtgEvalSummary}
    lines = []
    for sname, st in structs.items():
        lines.append(f'printf("%zu\\n", sizeof({sname}));')
        lines += [f'printf("%zu\\n", offsetof({sname}, {f}));' for f, _ in st._fields_]
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"pgtg.h\"\nint main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.run(["gcc", "-I", os.path.join(helpers.ROOT, "include"), "-o", os.path.join(d, "p"),
                        os.path.join(d, "p.c")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for st in structs.values():
        want.append(C.sizeof(st))
        want += [getattr(st, f).offset for f, _ in st._fields_]
    assert got == want
    # the header's field lists are the mirrors', in order
    for sname, st in structs.items():
        body = re.search(r"typedef struct \{([^}]*)\} " + sname + ";", src).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)\s*[;,]", body)
        assert names == [f for f, _ in st._fields_], sname
