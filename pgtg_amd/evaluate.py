"""Device-resident policy evaluation: ModularEvaluator.evaluate (pgtg/evaluator.py:284-339) and SB3's
`evaluate_policy` for the batch.

`PGTGVecEnv.evaluation(n_episodes, gamma)` gives an `Evaluation`: the bookkeeping of n_episodes evaluation
episodes spread over the N envs of the batch, on the env's GPU.  Env i contributes its first
`(n_episodes + i) // N` episodes -- SB3's quota, so that in a lockstep batch an env that crashes after three
steps does not count ten times where a careful one counts once.  After every tick one launch of the HIP
kernel k_eval (include/pgtg.h pgtg_eval_step) adds the step's fp64 reward to each open env's undiscounted and
discounted return and, where an episode ends under its quota, writes one record row: return, discounted
return, length, last reward, the step it ended at and its terminated / truncated flags.  `summary()` is the
fixed-order reduction k_eval_reduce over those records.

    ev = env.evaluation(1000, gamma=0.99)
    ev.run(policy, seed=7)                  # per step: k_policy, the tick, k_eval; one host sync every 16 steps
    s = ev.summary()                        # episodes, terminated, truncated_only, return_mean, return_std, ...
    eps = ev.episodes()                     # per-episode host arrays in SB3's completion order

    mean, std = evaluate_policy(policy, env, n_eval_episodes=1000)

While an Evaluation is active it owns the handle's flat bindings (set_flat_outputs / set_flat_scalars), as a
Rollout does: bind nothing else to them until `close()`.

`evaluate_reference` restates the kernel's rule in numpy fp64 on host arrays (SB3 is not a dependency; the
restatement is the yardstick of the tests, as gae_reference and policy_reference are).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .flat import check_flattenable, flat_dim

BLOCK = 256  # envs per k_eval workgroup: one row of `open` each
RECORD_DTYPES = {"rec_return": np.float64, "rec_discounted": np.float64, "rec_length": np.int32,
                 "rec_last_reward": np.float64, "rec_end_step": np.int32, "rec_flags": np.uint8}
SUMMARY_FIELDS = tuple(f for f, _ in _abi.PgtgEvalSummary._fields_)
_MOMENTS = ("return_mean", "return_std", "discounted_mean", "discounted_std")


def quotas(n_episodes: int, num_envs: int):
    """Episodes env i contributes, SB3's evaluate_policy: (n_episodes + i) // num_envs (int64 [num_envs])."""
    return (int(n_episodes) + np.arange(int(num_envs), dtype=np.int64)) // int(num_envs)


def episode_slots(n_episodes: int, num_envs: int) -> int:
    """Q = ceil(n_episodes / num_envs): the largest quota, the rows of the [Q, N] record arrays."""
    return -(-int(n_episodes) // int(num_envs))


def _ordered(rec: dict, cnt) -> dict:
    """The rows k < cnt[e] of [Q, N] record arrays as per-episode arrays sorted by (end_step, env): the order
    in which a loop over the steps, appending the finished envs in env order, meets them (SB3's)."""
    Q, N = rec["rec_return"].shape
    k, e = np.nonzero(np.arange(Q)[:, None] < np.asarray(cnt)[None, :])
    order = np.lexsort((e, rec["rec_end_step"][k, e]))
    k, e = k[order], e[order]
    flags = rec["rec_flags"][k, e]
    return {"env": e.astype(np.int64), "returns": rec["rec_return"][k, e], "discounted": rec["rec_discounted"][k, e],
            "lengths": rec["rec_length"][k, e], "last_reward": rec["rec_last_reward"][k, e],
            "end_step": rec["rec_end_step"][k, e], "terminated": (flags & 1) != 0, "truncated": (flags & 2) != 0}


def summarize(eps: dict, open_envs: int) -> dict:
    """The fields of PgtgEvalSummary from per-episode arrays, with np.mean and np.std (ddof 0)."""
    n = len(eps["returns"])
    s = {"episodes": n, "open_envs": int(open_envs), "terminated": int(eps["terminated"].sum()),
         "truncated_only": int((eps["truncated"] & ~eps["terminated"]).sum()),
         "last_reward_positive": int((eps["last_reward"] > 0).sum()),
         "last_reward_negative": int((eps["last_reward"] < 0).sum()),
         "negative_discounted": int((eps["discounted"] < 0).sum()),
         "length_sum": int(eps["lengths"].astype(np.int64).sum()),
         "length_min": int(eps["lengths"].min()) if n else 2 ** 31 - 1, "length_max": int(eps["lengths"].max()) if n else 0,
         "return_min": float(eps["returns"].min()) if n else float("inf"),
         "return_max": float(eps["returns"].max()) if n else float("-inf")}
    for name, key in (("return", "returns"), ("discounted", "discounted")):
        s[name + "_mean"] = float(np.mean(eps[key])) if n else None
        s[name + "_std"] = float(np.std(eps[key])) if n else None
    return s


def evaluate_reference(rewards, terminated, truncated, n_episodes: int, gamma: float) -> dict:
    """What T launches of k_eval compute, in numpy fp64, statement for statement (the running product g
    included): rewards, terminated, truncated [T, N] host arrays, row s = evaluation step s.  Returns a dict:
    the six [Q, N] record arrays under their PgtgEval names (rows k >= cnt[e] are zero), `cnt`, the running
    state `ret`, `disc`, `g`, `len` after the last step, `quota`, `open_envs` (after the last step) and
    `open_per_step` [T], `episodes` (per-episode arrays in (end_step, env) order) and `summary`."""
    rewards = np.asarray(rewards, dtype=np.float64)
    term = np.asarray(terminated) != 0
    trunc = np.asarray(truncated) != 0
    if rewards.ndim != 2 or term.shape != rewards.shape or trunc.shape != rewards.shape:
        raise ValueError("rewards, terminated, truncated: [T, N] arrays of one shape")
    if int(n_episodes) < 1:
        raise ValueError("n_episodes must be at least 1")
    T, N = rewards.shape
    gamma = np.float64(gamma)
    quota = quotas(n_episodes, N)
    Q = episode_slots(n_episodes, N)
    rec = {name: np.zeros((Q, N), dtype=dt) for name, dt in RECORD_DTYPES.items()}
    ret, disc, g = np.zeros(N), np.zeros(N), np.ones(N)
    ln, cnt = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    open_per_step = np.zeros(T, dtype=np.int64)
    for s in range(T):
        for e in np.nonzero(cnt < quota)[0]:
            r = rewards[s, e]
            ret[e] = ret[e] + r
            disc[e] = disc[e] + r * g[e]
            g[e] = g[e] * gamma
            ln[e] += 1
            if term[s, e] or trunc[s, e]:
                k = cnt[e]
                rec["rec_return"][k, e] = ret[e]
                rec["rec_discounted"][k, e] = disc[e]
                rec["rec_length"][k, e] = ln[e]
                rec["rec_last_reward"][k, e] = r
                rec["rec_end_step"][k, e] = s
                rec["rec_flags"][k, e] = (1 if term[s, e] else 0) | (2 if trunc[s, e] else 0)
                cnt[e] = k + 1
                ret[e] = disc[e] = 0.0
                g[e] = 1.0
                ln[e] = 0
        open_per_step[s] = int((cnt < quota).sum())
    out = dict(rec)
    open_envs = int((cnt < quota).sum())
    eps = _ordered(rec, cnt)
    out.update(cnt=cnt, ret=ret, disc=disc, g=g, len=ln, quota=quota, open_envs=open_envs,
               open_per_step=open_per_step, episodes=eps, summary=summarize(eps, open_envs))
    return out


class Evaluation:
    """n_episodes evaluation episodes of `env`'s batch, resident on its device (see the module text).

    Tensors (N = env.num_envs, Q = ceil(n_episodes / N), D = the flat observation's length): obs [N, D] int8
    (the observation the policy acts on) and terminal_obs [N, D]; the state ret, disc, g [N] float64, len, cnt
    [N] int32; the records rec_return, rec_discounted, rec_last_reward [Q, N] float64, rec_length,
    rec_end_step [Q, N] int32, rec_flags [Q, N] uint8 (bit 0 terminated, bit 1 truncated), rows k < cnt[e]
    valid; open [ceil(N / 256)] int32, the envs of each 256 still under their quota."""

    def __init__(self, env, n_episodes: int, gamma: float = 0.99):
        import torch
        if int(n_episodes) < 1:
            raise ValueError("n_episodes must be at least 1")
        if not 0.0 <= float(gamma) <= 1.0:
            raise ValueError("gamma must be in [0, 1]")
        if not env.autoreset:
            raise ValueError("an evaluation needs autoreset=True (a finished env restarts in the same step)")
        try:
            check_flattenable(env.spec)
        except IndexError as e:
            raise ValueError(str(e)) from None
        self.env = env
        self.n_episodes = int(n_episodes)
        self.gamma = float(gamma)
        self.num_envs = N = env.num_envs
        self.slots = Q = episode_slots(n_episodes, N)
        self.obs_dim = D = flat_dim(env.spec)
        self.device = dev = env.device
        self.quota = quotas(n_episodes, N)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.obs = z((N, D), torch.int8)
        self.terminal_obs = z((N, D), torch.int8)
        self.ret, self.disc, self.g = z(N, torch.float64), z(N, torch.float64), torch.ones(N, dtype=torch.float64, device=dev)
        self.len, self.cnt = z(N, torch.int32), z(N, torch.int32)
        self.rec_return, self.rec_discounted = z((Q, N), torch.float64), z((Q, N), torch.float64)
        self.rec_last_reward = z((Q, N), torch.float64)
        self.rec_length, self.rec_end_step = z((Q, N), torch.int32), z((Q, N), torch.int32)
        self.rec_flags = z((Q, N), torch.uint8)
        rows = (N + BLOCK - 1) // BLOCK
        self.open = z(rows, torch.int32)
        under = np.zeros(rows * BLOCK, dtype=np.int32)
        under[:N] = self.quota > 0
        self._open0 = torch.as_tensor(under.reshape(rows, BLOCK).sum(axis=1, dtype=np.int32))  # (before any step)
        self._summary = z(C.sizeof(_abi.PgtgEvalSummary) // 8, torch.int64)
        nbytes = C.c_uint64()
        if env._lib.pgtg_eval_workspace_bytes(N, self.n_episodes, C.byref(nbytes)) != _abi.PGTG_OK:
            raise ValueError("pgtg_eval_workspace_bytes failed")
        self._workspace = z((nbytes.value + 7) // 8, torch.int64)
        self._actions = z(N, torch.uint8)
        self._values, self._log_probs = z(N, torch.float32), z(N, torch.float32)
        p = lambda t: t.data_ptr()  # noqa: E731
        self._args = _abi.PgtgEval(
            n=N, n_episodes=self.n_episodes, step=0, gamma=self.gamma, reward=p(env.reward), terminated=p(env.terminated),
            truncated=p(env.truncated), ret=p(self.ret), disc=p(self.disc), g=p(self.g), len=p(self.len), cnt=p(self.cnt),
            rec_return=p(self.rec_return), rec_discounted=p(self.rec_discounted), rec_length=p(self.rec_length),
            rec_last_reward=p(self.rec_last_reward), rec_end_step=p(self.rec_end_step), rec_flags=p(self.rec_flags),
            open_rows=p(self.open))
        self._own = (p(env.reward), p(env.terminated), p(env.truncated))
        self._keep = ()
        self.t = 0               # evaluation steps recorded so far
        self._started = False

    @property
    def max_steps(self):
        """Steps within which every quota is met whatever the policy does: Q episodes of at most
        max_episode_steps steps each (None for an env without a time limit)."""
        return self.slots * int(self.env.max_episode_steps) if self.env.max_episode_steps else None

    # -- recording -------------------------------------------------------------------------------
    def _zero(self) -> None:
        for t in (self.ret, self.disc, self.len, self.cnt, self.rec_return, self.rec_discounted, self.rec_length,
                  self.rec_last_reward, self.rec_end_step, self.rec_flags):
            t.zero_()  # (the records too: rows k >= cnt[e] read as zero, whatever an earlier evaluation left)
        self.g.fill_(1.0)
        self.open.copy_(self._open0)
        self.t = 0

    def begin(self, seed=None):
        """Start an evaluation: reset the env (seeded: env i gets seed + i; the same seed gives every policy
        the same episodes) with its observation written into obs, and zero the state.  Returns obs."""
        env = self.env
        env.set_flat_scalars(None, None, None)
        env.set_flat_outputs(self.obs, self.terminal_obs)
        env.reset(seed=seed)
        self._zero()
        self._started = True
        return self.obs

    def clear(self) -> None:
        """Zero the state without touching the env or its bindings (record_from on chosen streams)."""
        self._zero()

    def _record(self, reward_ptr: int, term_ptr: int, trunc_ptr: int) -> None:
        a, env = self._args, self.env
        a.reward, a.terminated, a.truncated, a.step = reward_ptr, term_ptr, trunc_ptr, self.t
        env._bind_stream()
        rc = env._lib.pgtg_eval_step(env._h, C.byref(a))
        if rc != _abi.PGTG_OK:
            from .vector import _check
            _check(rc, env._h)
        self.t += 1

    def step(self, actions):
        """One tick of every env from `actions` ([N] uint8 device tensor) and one launch of k_eval on the
        step's reward, terminated and truncated outputs, as evaluation step t.  Returns obs."""
        if not self._started:
            raise RuntimeError("begin() first")
        self.env.step_actions(actions)
        self._record(*self._own)
        return self.obs

    def record_from(self, reward, terminated, truncated) -> None:
        """k_eval alone, as evaluation step t, on chosen [N] device tensors (float64; bool or uint8; bool or
        uint8) in place of the env's outputs (tests: records from chosen streams, without a tick)."""
        import torch
        N = self.num_envs
        for t, dts, name in ((reward, (torch.float64,), "reward"), (terminated, (torch.bool, torch.uint8), "terminated"),
                             (truncated, (torch.bool, torch.uint8), "truncated")):
            if t.dtype not in dts or tuple(t.shape) != (N,) or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{name}: a contiguous [{N}] tensor of {' or '.join(str(d) for d in dts)} on {self.device}")
        self._keep = (reward, terminated, truncated)  # (the launch reads them)
        self._record(reward.data_ptr(), terminated.data_ptr(), truncated.data_ptr())

    def open_envs(self) -> int:
        """Envs still under their quota after the last recorded step: one device-to-host copy of the
        ceil(N / 256) int32 rows k_eval wrote, summed.  Host-synchronising."""
        return int(self.open.cpu().sum())

    def run(self, policy, deterministic: bool = True, seed=None, max_steps=None, poll_every: int = 16) -> int:
        """The whole evaluation with a DevicePolicy: begin(seed), then per step one launch of k_policy on obs
        (deterministic: the argmax), the tick and k_eval -- no torch kernel -- and every poll_every steps one
        host synchronisation to read open_envs(); it stops at 0 open envs or after max_steps steps (default
        Q * max_episode_steps, within which every quota is met; an env without a time limit needs max_steps:
        ValueError otherwise, the loop being unbounded).  Episodes unfinished at the cap are not recorded;
        summary()["open_envs"] says how many envs fell short.  Returns the steps taken."""
        if getattr(policy, "obs_dim", None) != self.obs_dim:
            raise ValueError(f"the policy acts on rows of {getattr(policy, 'obs_dim', None)} values, "
                             f"the env's have {self.obs_dim}")
        if getattr(policy, "device", None) != self.device:
            raise ValueError(f"the policy is on {getattr(policy, 'device', None)}, the env on {self.device}")
        cap = self.max_steps if max_steps is None else int(max_steps)
        if cap is None:
            raise ValueError("the env has no time limit (max_episode_steps): give run() a max_steps")
        if cap < 0 or int(poll_every) < 1:
            raise ValueError("max_steps must be at least 0 and poll_every at least 1")
        obs = self.begin(seed)
        a, v, lp = self._actions, self._values, self._log_probs
        while self.t < cap:
            policy.act(obs, a, v, lp, deterministic=deterministic)
            self.step(a)
            if self.t % int(poll_every) == 0 and self.open_envs() == 0:
                break
        return self.t

    # -- results ---------------------------------------------------------------------------------
    def summary(self) -> dict:
        """The recorded episodes reduced on the device (k_eval_reduce, fixed order: two calls on the same
        records give the same bits) and read back as one struct: the fields of PgtgEvalSummary; the means
        and stds are None when no episode was recorded.  Host-synchronising."""
        env = self.env
        env._bind_stream()
        rc = env._lib.pgtg_eval_summary(env._h, C.byref(self._args), C.c_void_p(self._summary.data_ptr()),
                                        C.c_void_p(self._workspace.data_ptr()))
        if rc != _abi.PGTG_OK:
            from .vector import _check
            _check(rc, env._h)
        raw = self._summary.cpu().numpy().tobytes()
        s = _abi.PgtgEvalSummary.from_buffer_copy(raw)
        d = {f: getattr(s, f) for f in SUMMARY_FIELDS}
        if not d["episodes"]:
            for f in _MOMENTS:
                d[f] = None
        return d

    def records(self) -> dict:
        """Host copies of the six record arrays, cnt and the running state (numpy; host-synchronising)."""
        names = tuple(RECORD_DTYPES) + _abi.EVAL_STATE_FIELDS
        return {n: getattr(self, n).cpu().numpy() for n in names}

    def episodes(self) -> dict:
        """The recorded episodes as host arrays in SB3's completion order, sorted by (end_step, env): env,
        returns, discounted, lengths, last_reward, end_step, terminated, truncated."""
        r = self.records()
        return _ordered(r, r["cnt"])

    def close(self) -> None:
        """Unbind the flat rows from the handle (the tensors stay valid)."""
        env = self.env
        if env is not None and getattr(env, "_h", None) and self._started:
            env.set_flat_outputs(None, None)
            env.set_flat_scalars(None, None, None)
        self._started = False


def evaluate_policy(policy, env, n_eval_episodes: int = 10, deterministic: bool = True,
                    return_episode_rewards: bool = False):
    """SB3's evaluate_policy for a DevicePolicy and a PGTGVecEnv: n_eval_episodes episodes under SB3's per-env
    quotas, by Evaluation.run.  Returns (mean, std) of the undiscounted episode returns (the population std),
    or with return_episode_rewards the lists (returns, lengths) in SB3's completion order."""
    ev = Evaluation(env, n_eval_episodes, gamma=1.0)
    try:
        ev.run(policy, deterministic=deterministic)
        if return_episode_rewards:
            eps = ev.episodes()
            return [float(x) for x in eps["returns"]], [int(x) for x in eps["lengths"]]
        s = ev.summary()
        return s["return_mean"], s["return_std"]
    finally:
        ev.close()
