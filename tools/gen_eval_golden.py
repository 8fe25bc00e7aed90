"""Container-only: run the REFERENCE's ModularEvaluator.evaluate (pgtg/evaluator.py:284-339, imported through
tools/refload.py) and write what it saw and what it returned to tests/golden/eval_reference.npz.  The
reference itself never travels; only this data file does.

The evaluator runs on the reference PGTGEnv behind a small time-limit stand-in (gymnasium's TimeLimit rule:
truncated once the episode has taken `TIME_LIMIT` steps) that logs every step's (reward, terminated,
truncated) and where each episode starts.  Two runs, combined as the reference's evaluate_multiple_agents
combines its agents' (the returned lists one after the other, the counters added):

1. 12 episodes on 3x3 maps with a scripted agent: in two of three episodes it draws uniform actions from a
   seeded generator (the car crashes: terminated, negative last reward), in the third it coasts (action 4)
   and stands still until the time limit truncates the episode;
2. one episode that reaches the goal (terminated with a positive last reward and a positive discounted
   return): the first episode of env 3 of tests/golden/fuzz/traj_wide_28.npz, replayed from that file's
   seed and action column on the configuration tests/fuzz_configs.py wide_kwargs(28); the replayed rewards
   are checked against the golden's.

max_steps is above the time limit, so that the evaluator's own cut ("over max steps", its counter 2) never
fires: that cut is outside what pgtg_amd.evaluate restates.

Usage:  python tools/gen_eval_golden.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refload  # noqa: E402

env_mod = refload.load()[0]
import evaluator as ref_evaluator  # noqa: E402  (reference pgtg/evaluator.py)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.append(_p)
import fuzz_configs  # noqa: E402  (tests/fuzz_configs.py)

OUT = os.path.join(REPO, "tests", "golden", "eval_reference.npz")
KWARGS = dict(random_map_width=3, random_map_height=3, standing_still_penalty=1)
SEED, AGENT_SEED = 2024, 11
NUMBER, MAX_STEPS, GAMMA, TIME_LIMIT = 12, 20, 0.99, 9
GOAL_CASE, GOAL_K, GOAL_ENV = "wide_28", 28, 3   # tests/golden/fuzz/traj_wide_28.npz, env 3's first episode


class LoggedTimeLimit:
    """The env the evaluator sees: reset() and step() of the reference env, with the time limit and a log.
    reseed: every reset is seeded (the evaluator resets once before its first episode; an episode recorded
    from reset(seed=s) is met again only by another reset(seed=s))."""

    def __init__(self, env, limit, seed, reseed=False):
        self.env, self.limit, self.seed, self.reseed = env, limit, seed, reseed
        self.log, self.starts, self.elapsed, self.resets = [], [], 0, 0

    def reset(self):
        out = self.env.reset(seed=self.seed) if self.resets == 0 or self.reseed else self.env.reset()
        self.resets += 1
        self.elapsed = 0
        self.starts.append(len(self.log))
        return out

    def step(self, action):
        obs, reward, terminated, _, info = self.env.step(action)
        self.elapsed += 1
        truncated = self.elapsed >= self.limit
        self.log.append((float(reward), bool(terminated), bool(truncated)))
        return obs, reward, terminated, truncated, info


class ScriptedAgent:
    def __init__(self, env):
        self.env, self.rng = env, np.random.default_rng(AGENT_SEED)

    def act(self, state):
        episode = self.env.resets - 2  # (the evaluator resets once before its first episode)
        return 4 if episode % 3 == 2 else int(self.rng.integers(0, 9))


class ReplayAgent:
    """The recorded action column, by the episode's step."""

    def __init__(self, env, actions):
        self.env, self.actions = env, [int(a) for a in actions]

    def act(self, state):
        return self.actions[self.env.elapsed]


def make_env(kwargs, seed, reseed=False):
    cwd = os.getcwd()
    os.chdir(REPO)
    env = LoggedTimeLimit(env_mod.PGTGEnv(None, **kwargs), TIME_LIMIT, seed, reseed)
    os.chdir(cwd)
    return env


def main():
    env = make_env(KWARGS, SEED)
    returns, counters = ref_evaluator.ModularEvaluator(env, ScriptedAgent(env)).evaluate(NUMBER, MAX_STEPS, GAMMA)
    returns, counters = list(returns), list(counters)
    log, starts = list(env.log), env.starts[1:]  # (the first reset is followed by no step)
    assert len(starts) == NUMBER and len(returns) == NUMBER

    z = np.load(os.path.join(REPO, "tests", "golden", "fuzz", f"traj_{GOAL_CASE}.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    end = int(np.nonzero(z["terminated"][:, GOAL_ENV])[0][0])
    assert z["reward"][end, GOAL_ENV] > 0 and end + 1 < TIME_LIMIT
    genv = make_env(fuzz_configs.wide_kwargs(GOAL_K), meta["seed_base"] + GOAL_ENV, reseed=True)
    agent = ReplayAgent(genv, z["actions"][:end + 1, GOAL_ENV])
    g_returns, g_counters = ref_evaluator.ModularEvaluator(genv, agent).evaluate(1, MAX_STEPS, GAMMA)
    assert [r for r, _, _ in genv.log] == [float(x) for x in z["reward"][:end + 1, GOAL_ENV]]  # the golden's episode
    assert genv.log[-1][1] and genv.log[-1][0] > 0 and g_returns[0] > 0
    starts = starts + [len(log) + s for s in genv.starts[1:]]
    log += genv.log
    returns += list(g_returns)
    counters = [a + b for a, b in zip(counters, g_counters)]
    number = NUMBER + 1

    term = np.array([t for _, t, _ in log], dtype=np.uint8)
    trunc = np.array([t for _, _, t in log], dtype=np.uint8)
    assert len(starts) == number and len(returns) == number
    assert counters[2] == 0 and counters[0] >= 1 and counters[1] >= 1 and counters[3] < number, counters
    assert (term | trunc).sum() == number and (term | trunc)[-1]
    np.savez_compressed(OUT, rewards=np.array([r for r, _, _ in log], dtype=np.float64), terminated=term,
                        truncated=trunc, episode_start=np.array(starts, dtype=np.int64), number=np.int64(number),
                        run_number=np.array([NUMBER, 1], dtype=np.int64), max_steps=np.int64(MAX_STEPS),
                        GAMMA=np.float64(GAMMA), time_limit=np.int64(TIME_LIMIT),
                        returns=np.array([float(x) for x in returns], dtype=np.float64),
                        counters=np.array(counters, dtype=np.int64))
    print(OUT, os.path.getsize(OUT), "bytes;", len(log), "steps; counters", counters)
    print("returns", [round(float(x), 3) for x in returns])


if __name__ == "__main__":
    main()
