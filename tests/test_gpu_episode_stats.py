"""Episode returns and lengths on the device (include/pgtg.h pgtg_set_episode_stats, the HIP kernel
k_episode): SB3's VecMonitor (pgtg/train.py:55) for the whole batch.

The checker is a numpy restatement of VecMonitor's rule, float32 return and int32 length per env, fed
with the step's own reward / terminated / truncated outputs (which the rest of the suite pins to the
oracle); it shares nothing with the kernel.  SB3 itself cannot be imported here, so the rule is restated
(parity unpinned, like the flatten layout):

    ret += float32(reward); len += 1; ep_return = ret; ep_length = len
    terminated | truncated: the episode (ret, len, truncated and not terminated) joins the summary; ret = len = 0

Per-env values are compared bit for bit.  The summary's counts, length sum and min / max values are
compared exactly; return_sum (the fp64 sum of the episodes' float32 returns, whose order over a
workgroup's lanes is the kernel's) within n * 2^-52 * sum|r_i| of numpy's fp64 sum, the worst case of any
summation order of n terms.  The 3x3 config pays a non-integer standing-still penalty, so float32
rounding takes part (asserted)."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
from pgtg_amd import _abi
from pgtg_amd import config as cfg

pytestmark = pytest.mark.gpu

SMALL = dict(random_map_width=3, random_map_height=3, standing_still_penalty=0.3)
# the caller's settings (pgtg/train.py:21-40), all of them: the goal bonus and the standing-still penalty
# shape the rewards that are accumulated here (the TimeLimit is the test's L)
CALLER = dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=0.2,
              random_map_percentage_of_connections=0.8, traffic_density=0.2,
              conservative_driver_percentage=0.15, normal_driver_percentage=0.50,
              aggressive_driver_percentage=0.20, elderly_driver_percentage=0.10,
              reckless_driver_percentage=0.05, sliding_observation_window_size=5,
              max_allowed_deviation=15, use_sliding_observation_window=True,
              use_next_subgoal_direction=True, final_goal_bonus=200, standing_still_penalty=1)
INT32_MAX = 2**31 - 1


def _spec(**kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cfg.make_spec(**kw)


class Model:
    """VecMonitor's accumulators for N envs and the list of finished episodes."""

    def __init__(self, n):
        self.ret = np.zeros(n, np.float32)
        self.len = np.zeros(n, np.int32)
        self.ret64 = np.zeros(n, np.float64)  # the same return without float32 rounding
        self.inexact = 0                      # finished or running returns that differ from it
        self.r, self.l, self.tonly = [], [], []

    def step(self, reward, term, trunc):
        term, trunc = np.asarray(term, bool), np.asarray(trunc, bool)
        r32 = np.asarray(reward, np.float64).astype(np.float32)  # rounded once
        self.ret = self.ret + r32
        assert self.ret.dtype == np.float32
        self.len = self.len + np.int32(1)
        self.ret64 += np.asarray(reward, np.float64)
        self.inexact += int((self.ret.astype(np.float64) != self.ret64).sum())
        out_r, out_l = self.ret.copy(), self.len.copy()
        done = term | trunc
        for i in np.nonzero(done)[0]:  # env order (any order gives the same exact fields)
            self.r.append(out_r[i])
            self.l.append(int(out_l[i]))
            self.tonly.append(bool(trunc[i] and not term[i]))
        self.zero(done)
        return out_r, out_l

    def zero(self, mask=None):
        m = slice(None) if mask is None else np.asarray(mask, bool)
        self.ret[m] = 0
        self.len[m] = 0
        self.ret64[m] = 0

    def mark(self):
        return len(self.r)

    def summary(self, since=0):
        r = np.array(self.r[since:], np.float32)
        ln = np.array(self.l[since:], np.int64)
        n = len(r)
        return {"episodes": n, "truncated_only": int(sum(self.tonly[since:])), "length_sum": int(ln.sum()),
                "length_min": int(ln.min()) if n else INT32_MAX, "length_max": int(ln.max()) if n else 0,
                "return_sum": float(r.astype(np.float64).sum()),
                "return_min": float(r.min()) if n else float("inf"), "return_max": float(r.max()) if n else float("-inf"),
                "abs_sum": float(np.abs(r.astype(np.float64)).sum())}


EXACT = ("episodes", "truncated_only", "length_sum", "length_min", "length_max", "return_min", "return_max")


def check_summary(got, want, tag=""):
    for k in EXACT:
        print(f"summary {tag} {k}: got {got[k]!r} want {want[k]!r}")
        assert got[k] == want[k], (tag, k, got[k], want[k])
    n = want["episodes"]
    bound = n * 2.0**-52 * want["abs_sum"]
    print(f"summary {tag} return_sum: got {got['return_sum']!r} want {want['return_sum']!r} bound {bound!r}")
    assert abs(got["return_sum"] - want["return_sum"]) <= bound, (tag, got["return_sum"], want["return_sum"], bound)
    if n:
        assert got["return_mean"] == got["return_sum"] / n and got["length_mean"] == got["length_sum"] / n
    else:
        assert got["return_mean"] is None and got["length_mean"] is None


def bits(summary):
    """A summary as comparable bits (return_sum included)."""
    return tuple((k, np.float64(v).tobytes() if isinstance(v, float) else v) for k, v in sorted(summary.items()))


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def mostly_still(rng, n):
    """Mostly stand still (tests/test_gpu_vec.py test_time_limit_truncates_and_resets_in_kernel): both
    terminations (crashes) and TimeLimit truncations occur."""
    return np.where(rng.random(n) < 0.8, 4, rng.integers(0, 9, n)).astype(np.uint8)


def uniform(rng, n):
    return rng.integers(0, 9, n).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def rollout(kind, N, L, T, tune=None, extra=5):
    """One monitored run, computed once and shared: per tick the kernel's rows and the model's, the
    summaries read mid-run and at the end without reset, the read with reset, and the summary of `extra`
    further ticks after it."""
    from pgtg_amd.vector import PGTGVecEnv
    spec = _spec(**(SMALL if kind == "small" else CALLER))
    draw = mostly_still if kind == "small" else uniform
    env = PGTGVecEnv(N, spec=spec, device=0, autoreset=True, max_episode_steps=L, tune=dict(tune) if tune else None)
    er, el = env.enable_episode_stats()
    env.reset(seed=40)
    model = Model(N)
    rng = np.random.default_rng(5)
    rec = {"ticks": [], "kernel": env.step_kernel()}
    for t in range(T + extra):
        _, rew, term, trunc, infos = env.step(torch.as_tensor(draw(rng, N)))
        assert infos["episode_return"] is er and infos["episode_length"] is el
        assert torch.equal(infos["_episode"], term | trunc)
        want = model.step(rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy())
        rec["ticks"].append((er.cpu().numpy(), el.cpu().numpy()) + want)
        if t == T // 2:
            rec["mid"] = (env.episode_summary(reset=False), model.summary())
        if t == T - 1:
            rec["end"] = (env.episode_summary(reset=False), model.summary())
            rec["end_reset"] = env.episode_summary(reset=True)
            rec["zero"] = env.episode_summary(reset=False)
            mark = model.mark()
    rec["after"] = (env.episode_summary(reset=False), model.summary(since=mark))
    rec["inexact"] = model.inexact
    env.close()
    return rec


def check_rows(rec):
    for t, (got_r, got_l, want_r, want_l) in enumerate(rec["ticks"]):
        assert got_r.dtype == np.float32 and got_l.dtype == np.int32
        assert same_bits(got_r, want_r), (t, np.nonzero(got_r != want_r)[0][:8])
        assert np.array_equal(got_l, want_l), (t, np.nonzero(got_l != want_l)[0][:8])


def check_summaries(rec):
    for key in ("mid", "end", "after"):
        check_summary(*rec[key], tag=key)
    assert rec["mid"][0]["episodes"] < rec["end"][0]["episodes"]
    assert bits(rec["end_reset"]) == bits(rec["end"][0])  # the read with reset returns the full summary ...
    check_summary(rec["zero"], Model(1).summary(), tag="zero")  # ... and the count restarts
    assert rec["zero"]["return_sum"] == 0.0


SIZES = [1, 67, 257, 1000]  # lane tail, wave tail, workgroup tail, four partial rows


@pytest.mark.parametrize("N", SIZES)
def test_every_row_every_tick(N):
    rec = rollout("small", N, 5, 25)
    check_rows(rec)
    end = rec["end"][1]
    assert end["truncated_only"] > 0 and end["episodes"] - end["truncated_only"] > 0, end
    if N > 1:
        assert rec["inexact"] > 0  # float32 rounding took part: a return differs from its fp64 sum


@pytest.mark.parametrize("N", SIZES)
def test_summary(N):
    check_summaries(rollout("small", N, 5, 25))


def test_summary_is_reproducible_across_handles():
    """Two handles with the same seeds and actions: bit-equal summaries, return_sum included (a handle
    made after the cached one was closed)."""
    a = rollout("small", 1000, 5, 25)
    b = rollout.__wrapped__("small", 1000, 5, 25)
    for key in ("mid", "end", "after"):
        assert bits(a[key][0]) == bits(b[key][0]), key


@pytest.mark.parametrize("mode", [1, 2])
def test_summary_is_the_same_for_every_queue_mode(mode):
    """tune queue_mode 1 / 2 (the map-queue step kernels where the config allows the queue; the grid of
    k_episode does not depend on the step kernel or the device)."""
    a = rollout("small", 1000, 5, 25)
    b = rollout("small", 1000, 5, 25, tune=(("queue_mode", mode),))
    print("step kernels:", a["kernel"], b["kernel"])
    check_rows(b)
    for key in ("mid", "end", "after"):
        assert bits(a[key][0]) == bits(b[key][0]), key


def test_traffic_at_the_callers_settings():
    rec = rollout("caller", 64, 7, 25)
    check_rows(rec)
    check_summaries(rec)
    assert rec["end"][1]["episodes"] > 0


def test_oracle_end_to_end():
    """Rewards and done flags from the CPU oracle driven like the reference behind TimeLimit
    (tests/test_gpu_vec.py:34-65); the model is fed those."""
    from oracle.oracle import OracleEnv
    from pgtg_amd.vector import PGTGVecEnv
    spec = _spec(**SMALL)
    N, L, T = 12, 5, 15
    env = PGTGVecEnv(N, spec=spec, device=0, autoreset=True, max_episode_steps=L)
    er, el = env.enable_episode_stats()
    env.reset(seed=40)
    orcs = [OracleEnv(spec) for _ in range(N)]
    for i, o in enumerate(orcs):
        o.reset(40 + i)
    elapsed = np.zeros(N, int)
    model = Model(N)
    rng = np.random.default_rng(5)
    for t in range(T):
        acts = mostly_still(rng, N)
        env.step(torch.as_tensor(acts))
        rew, term, trunc = np.zeros(N), np.zeros(N, bool), np.zeros(N, bool)
        for i in range(N):
            r = orcs[i].step(int(acts[i]))
            elapsed[i] += 1
            rew[i], term[i], trunc[i] = r["reward"], r["terminated"], elapsed[i] >= L
            if term[i] or trunc[i]:
                orcs[i].reset(None)
                elapsed[i] = 0
        want_r, want_l = model.step(rew, term, trunc)
        assert same_bits(er.cpu().numpy(), want_r) and np.array_equal(el.cpu().numpy(), want_l), t
    assert model.mark() > 0
    check_summary(env.episode_summary(), model.summary(), tag="oracle")
    env.close()


def test_step_many_equals_the_loop_of_steps():
    from pgtg_amd.vector import PGTGVecEnv
    spec = _spec(**SMALL)
    N, T = 257, 12
    envs = [PGTGVecEnv(N, spec=spec, device=0, autoreset=True, max_episode_steps=5) for _ in range(2)]
    outs = [e.enable_episode_stats() for e in envs]
    for e in envs:
        e.reset(seed=9)
    rng = np.random.default_rng(3)
    actions = torch.as_tensor(np.stack([mostly_still(rng, N) for _ in range(T)])).cuda()
    envs[0].step_many(actions)
    for t in range(T):
        envs[1].step(actions[t])
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(envs[0].reward, envs[1].reward) and torch.equal(envs[0].obs_map, envs[1].obs_map)
    s = [e.episode_summary() for e in envs]
    assert s[0]["episodes"] > 0 and bits(s[0]) == bits(s[1])
    for e in envs:
        e.close()


def _tick(env, model, outs, acts):
    env.step(torch.as_tensor(acts))
    want_r, want_l = model.step(env.reward.cpu().numpy(), env.terminated.cpu().numpy(), env.truncated.cpu().numpy())
    assert same_bits(outs[0].cpu().numpy(), want_r) and np.array_equal(outs[1].cpu().numpy(), want_l)


def test_resets_zero_the_accumulators_and_keep_the_summary():
    from pgtg_amd.vector import PGTGVecEnv
    spec = _spec(**SMALL)
    N = 67
    env = PGTGVecEnv(N, spec=spec, device=0, autoreset=True, max_episode_steps=9)
    outs = env.enable_episode_stats()
    env.reset(seed=21)
    model = Model(N)
    rng = np.random.default_rng(8)
    for _ in range(7):
        _tick(env, model, outs, mostly_still(rng, N))
    assert (model.len > 0).any()
    before = env.episode_summary(reset=False)
    # a masked seeded reset mid-episode: only the masked envs restart their count
    mask = np.arange(N) % 3 == 0
    assert (model.len[mask] > 0).any() and (model.len[~mask] > 0).any()
    env.reset(seed=500, mask=torch.as_tensor(mask))
    model.zero(mask)
    assert bits(env.episode_summary(reset=False)) == bits(before)
    _tick(env, model, outs, mostly_still(rng, N))
    assert (model.len[~mask] > 1).any()
    # an unseeded reset of every env
    env.reset()
    model.zero()
    _tick(env, model, outs, mostly_still(rng, N))
    assert (model.len <= 1).all()
    # load_state: the accumulators are not in the blob and restart for every env; the summary stays
    blob = env.dump_state()
    for _ in range(3):
        _tick(env, model, outs, mostly_still(rng, N))
    before = env.episode_summary(reset=False)
    env.load_state(blob)
    model.zero()
    assert bits(env.episode_summary(reset=False)) == bits(before)
    _tick(env, model, outs, mostly_still(rng, N))
    assert (model.len <= 1).all()
    check_summary(env.episode_summary(), model.summary(), tag="resets")
    env.close()


def test_without_autoreset_the_count_restarts_at_the_explicit_reset():
    from pgtg_amd.vector import PGTGVecEnv
    spec = _spec(**SMALL)
    N = 4
    env = PGTGVecEnv(N, spec=spec, device=0, autoreset=False)
    outs = env.enable_episode_stats()
    env.reset(seed=3)
    model = Model(N)
    rng = np.random.default_rng(2)
    for _ in range(30):
        _tick(env, model, outs, uniform(rng, N))
        done = (env.terminated | env.truncated).cpu().numpy()
        if done.any():  # (the model's rule zeroed these already; the reset must leave the others)
            env.reset(mask=torch.as_tensor(done))
            model.zero(done)
    assert (model.len > 0).any()  # at least the running values were compared
    check_summary(env.episode_summary(), model.summary(), tag="no autoreset")
    env.close()


def test_off_by_default_and_unbinding():
    from pgtg_amd.vector import PGTGVecEnv
    spec = _spec(**SMALL)
    N = 67
    plain = PGTGVecEnv(N, spec=spec, device=0, autoreset=True, max_episode_steps=5)
    stats = PGTGVecEnv(N, spec=spec, device=0, autoreset=True, max_episode_steps=5)
    er, el = stats.enable_episode_stats()
    assert plain.step_kernel() == stats.step_kernel()
    with pytest.raises(ValueError):
        plain.episode_summary()  # never bound
    for e in (plain, stats):
        e.reset(seed=12)
    rng = np.random.default_rng(6)
    for t in range(10):
        a = torch.as_tensor(mostly_still(rng, N))
        _, _, _, _, infos = plain.step(a)
        assert "episode_return" not in infos and "_episode" not in infos
        stats.step(a)
        for name in ("obs_map", "position", "velocity", "reward", "terminated", "truncated", "final_map", "braking"):
            assert torch.equal(getattr(plain, name), getattr(stats, name)), (t, name)
    assert int(el.max()) > 0
    stats.disable_episode_stats()
    er.fill_(-7.0)
    el.fill_(-7)
    _, _, _, _, infos = stats.step(torch.as_tensor(mostly_still(rng, N)))
    torch.cuda.synchronize()
    assert "episode_return" not in infos
    assert bool((er == -7.0).all()) and bool((el == -7).all())
    with pytest.raises(ValueError):
        stats.enable_episode_stats(torch.zeros(N, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        stats.enable_episode_stats(ep_length=torch.zeros(N + 1, dtype=torch.int32, device="cuda"))
    plain.close()
    stats.close()


def test_bind_time_refusals():
    """Through ctypes; no step call follows a refusal."""
    L = _abi.lib()
    N = 8
    cs = _abi.config_struct(_spec(**SMALL), True, 5)
    h = C.c_void_p()
    assert L.pgtg_create(C.byref(cs), N, 0, C.byref(h)) == _abi.PGTG_OK
    er = torch.zeros(N, dtype=torch.float32, device="cuda")
    el = torch.zeros(N, dtype=torch.int32, device="cuda")
    rew = torch.zeros(N, dtype=torch.float64, device="cuda")
    term = torch.zeros(N, dtype=torch.uint8, device="cuda")
    trunc = torch.zeros(N, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = _abi.PgtgEpisodeSummary()
    try:
        assert L.pgtg_episode_summary(h, C.byref(s), 0) == _abi.PGTG_E_INVALID  # never bound
        assert L.pgtg_set_episode_stats(h, p(er), p(el)) == _abi.PGTG_E_INVALID  # before pgtg_set_outputs
        full = _abi.PgtgOutputs()
        full.reward, full.terminated, full.truncated = rew.data_ptr(), term.data_ptr(), trunc.data_ptr()
        assert L.pgtg_set_outputs(h, C.byref(full)) == _abi.PGTG_OK
        assert L.pgtg_set_episode_stats(h, p(er), None) == _abi.PGTG_E_INVALID  # one pointer
        assert L.pgtg_set_episode_stats(h, None, p(el)) == _abi.PGTG_E_INVALID
        assert L.pgtg_episode_summary(h, C.byref(s), 0) == _abi.PGTG_E_INVALID  # still never bound
        assert L.pgtg_set_episode_stats(h, p(er), p(el)) == _abi.PGTG_OK
        part = _abi.PgtgOutputs()
        part.terminated, part.truncated = term.data_ptr(), trunc.data_ptr()
        assert L.pgtg_set_outputs(h, C.byref(part)) == _abi.PGTG_E_INVALID  # reward dropped while bound
        assert L.pgtg_last_error(h)
        assert L.pgtg_set_outputs(h, C.byref(full)) == _abi.PGTG_OK
        assert L.pgtg_episode_summary(h, C.byref(s), 1) == _abi.PGTG_OK
        assert (s.episodes, s.length_min, s.length_max, s.return_sum) == (0, INT32_MAX, 0, 0.0)
        assert s.return_min == float("inf") and s.return_max == float("-inf")
        assert L.pgtg_set_episode_stats(h, None, None) == _abi.PGTG_OK  # off
        assert L.pgtg_set_outputs(h, C.byref(part)) == _abi.PGTG_OK  # ... and the outputs are free again
    finally:
        L.pgtg_destroy(h)
