"""Device-resident PPO rollout buffer: SB3's `RolloutBuffer` for the batch (the PPO of pgtg/train.py:61-74).

`PGTGVecEnv.rollout(n_steps, gamma, gae_lambda, obs_dtype)` gives a `Rollout`: the storage of one rollout
of T = n_steps steps of all N envs, on the env's GPU.  Recording costs nothing beyond the step: every
step's flattened observation, float32 reward, done and truncated-only flags are written by the step's own
k_flatten pass straight into the rollout's rows (the handle's flat outputs are rebound to row t before each
launch), and the terminal observations of the finished envs into `terminal_obs`.  `finish()` is one launch
of the HIP kernel k_gae (include/pgtg.h pgtg_gae): the time-limit bootstrap and the backward GAE scan of
`RolloutBuffer.compute_returns_and_advantage`.  `get()` hands out minibatches in SB3's sample order.

    ro = env.rollout(128)
    obs = ro.begin()
    for t in range(128):
        actions, values, log_probs = policy(obs)
        obs, rewards, dones = ro.step(actions, values, log_probs)
        ro.set_terminal_values(value_net(ro.terminal_obs))      # valid on the truncated rows
    ro.finish(value_net(obs))
    for obs_b, act_b, val_b, logp_b, adv_b, ret_b in ro.get(batch_size=4096): ...

With the library's own policy (pgtg_amd.policy.DevicePolicy: SB3's MlpPolicy as the HIP kernel k_policy,
which reads obs[t] and writes the action, value and log-probability rows) the loop is the library's:

    policy = DevicePolicy(env); policy.load_state_dict(module.state_dict())
    ro.collect(policy)                                           # T x (k_policy, the tick, V(terminal_obs)), k_gae
    ro.update(policy, module, optimizer)                         # SB3's PPO.train: per minibatch k_ppo_loss, k_ppo_dw1,
                                                                 # k_ppo_reduce into module's .grad, then clip, step, repack
    ro.train_log()                                               # its train/ log (k_ppo_expl_var, k_ppo_log)

On an env with separate_reward_cost, `env.rollout(128, cost_limit=d)` also records the step's cost
(info["cost"]) into `costs`, and finish() first runs k_cost_scan / k_cost_dual (include/pgtg.h pgtg_cost_scan):
the cost summed per episode, `penalised_rewards = rewards - lambda * costs` (RCPO, Tessler et al. 2018), which
k_gae then takes as its rewards, and the multiplier's dual ascent on the mean episode cost against the budget d.
Rollout k is penalised with the multiplier rollouts 0 .. k-1 produced.  `cost_log()` reads the summary.

`env.rollout(128, norm_reward=True)` is SB3's `VecNormalize(norm_reward=True)` around the env, reward half:
finish() first runs k_ret_scan / k_ret_stats / k_ret_apply (include/pgtg.h pgtg_reward_norm), which carry each env's
discounted return and the running mean, variance and count of those returns across rollouts and write
`normalised_rewards = clip(rewards / sqrt(var + epsilon), +-clip_reward)`; the cost scan and k_gae then take those
(`rewards` keeps the raw reward).  `reward_norm_state()` / `load_reward_norm_state()` are its checkpoint,
`norm_training = False` freezes the statistics, `norm_log()` reads them.  `reward_norm_reference` restates the
kernels in numpy.  Observations are not normalised: the rows are int8 flags.

While a Rollout records, it owns the handle's flat bindings (set_flat_outputs / set_flat_scalars /
set_flat_cost): bind nothing else to them until `close()`.

`gae_reference` restates SB3's numpy loop (SB3 is not a dependency; the restatement is the yardstick of the
tests, as the flatten layout's and the episode statistics' are).
"""
from __future__ import annotations

import ctypes as C

from . import _abi
from .flat import check_flattenable, flat_dim


def sample_index(s, n_steps: int):
    """(env, step) of flat sample index s: SB3's swap_and_flatten turns [T, N] into [N * T] with the
    step running fastest, so s = env * T + step.  Works on ints, numpy arrays and tensors."""
    return s // n_steps, s % n_steps


def gae_reference(rewards, values, dones, truncated_only, terminal_values, last_values, gamma, gae_lambda):
    """SB3's arithmetic in numpy float32 on host arrays: the time-limit bootstrap of collect_rollouts,
    rewards[mask] += gamma * terminal_values[mask], then compute_returns_and_advantage.  rewards, values
    [T, N]; dones [T + 1, N] (row t = episode_starts of step t, row T = dones after the last step);
    truncated_only, terminal_values [T, N] or both None; last_values [N].  Returns (advantages, returns)."""
    import numpy as np
    rewards = np.array(rewards, dtype=np.float32)  # (a copy: the bootstrap is applied in place)
    values = np.asarray(values, dtype=np.float32)
    dones = np.asarray(dones)
    last_values = np.asarray(last_values, dtype=np.float32)
    gamma, gae_lambda = float(gamma), float(gae_lambda)
    T = rewards.shape[0]
    if truncated_only is not None:
        mask = np.asarray(truncated_only) != 0
        rewards[mask] += gamma * np.asarray(terminal_values, dtype=np.float32)[mask]
    advantages = np.zeros_like(rewards)
    last_gae_lam = 0
    for step in reversed(range(T)):
        next_non_terminal = 1.0 - (dones[step + 1] != 0).astype(np.float32)
        next_values = last_values if step == T - 1 else values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        advantages[step] = last_gae_lam
    return advantages, advantages + values


COST_BLOCK = 256  # envs per workgroup of k_cost_scan (pgtg_cost.h kCostBlock)
COST_AHEAD = 8    # rows it keeps in flight ahead of the row it consumes (kCostAhead)


def _cost_tree(s, k, m):
    """cost_block_reduce of pgtg_cost.h over lane values (numpy arrays, any length): 256 lanes per workgroup
    (the identity in the lanes past the end), each wave of 64 by the shuffle tree -- lane i takes lane i + o for
    o = 32, 16, .. 1 -- then the four waves in wave order.  Returns one (s, k, m) row per workgroup."""
    import numpy as np
    rows = -(-len(s) // COST_BLOCK)
    pad = rows * COST_BLOCK - len(s)
    s = np.concatenate([np.asarray(s, np.float64), np.zeros(pad)]).reshape(rows, 4, 64)
    k = np.concatenate([np.asarray(k, np.uint64), np.zeros(pad, np.uint64)]).reshape(rows, 4, 64)
    m = np.concatenate([np.asarray(m, np.float64), np.full(pad, -np.inf)]).reshape(rows, 4, 64)
    o = 32
    while o:
        s[..., :o] = s[..., :o] + s[..., o:2 * o]
        k[..., :o] = k[..., :o] + k[..., o:2 * o]
        m[..., :o] = np.maximum(m[..., :o], m[..., o:2 * o])
        o >>= 1
    rs, rk, rm = s[:, 0, 0].copy(), k[:, 0, 0].copy(), m[:, 0, 0].copy()
    for w in range(1, 4):
        rs = rs + s[:, w, 0]
        rk = rk + k[:, w, 0]
        rm = np.maximum(rm, m[:, w, 0])
    return rs, rk, rm


def cost_reference(rewards, costs, dones, carry, lam, cost_limit, lambda_lr, lambda_max):
    """k_cost_scan and k_cost_dual (pgtg_cost.h; include/pgtg.h pgtg_cost_scan) in numpy, statement for
    statement.  rewards, costs [T, N] float32; dones [T + 1, N] (row t + 1: the episode ended in step t); carry
    [N] float64, the cost of each env's episode under way; lam the multiplier (float32).  Returns
    (penalised [T, N] float32, new carry [N] float64, the finished episodes' costs in (env, step) order
    (float64), summary, next multiplier (numpy float32)); summary has the fields of PgtgCostSummary.  The
    sums run in the kernels' order: per env in step order, 256 envs per workgroup by _cost_tree, the
    workgroups' rows by lane t taking rows t, t + 256, ... and the same tree."""
    import numpy as np
    rewards = np.asarray(rewards, dtype=np.float32)
    costs = np.asarray(costs, dtype=np.float32)
    dones = np.asarray(dones) != 0
    lam = np.float32(lam)
    T, N = rewards.shape
    penalised = np.empty((T, N), np.float32)
    acc = np.array(carry, dtype=np.float64).reshape(N)  # (a copy)
    s, k, m = np.zeros(N), np.zeros(N, np.uint64), np.full(N, -np.inf)
    ends = np.zeros((T, N), bool)
    sums = np.zeros((T, N))
    for t in range(T):
        penalised[t] = rewards[t] - (lam * costs[t]).astype(np.float32)
        acc = acc + costs[t].astype(np.float64)
        d = dones[t + 1]
        s = np.where(d, s + acc, s)
        k = np.where(d, k + np.uint64(1), k)
        m = np.where(d, np.maximum(m, acc), m)
        ends[t], sums[t] = d, acc
        acc = np.where(d, 0.0, acc)
    episode_costs = sums.T[ends.T]  # (env, step) order
    rs, rk, rm = _cost_tree(s, k, m)  # k_cost_scan's rows
    ls, lk, lm = np.zeros(COST_BLOCK), np.zeros(COST_BLOCK, np.uint64), np.full(COST_BLOCK, -np.inf)
    for r in range(len(rs)):  # k_cost_dual: lane r % 256 takes the rows in order
        ln = r % COST_BLOCK
        ls[ln], lk[ln], lm[ln] = ls[ln] + rs[r], lk[ln] + rk[r], max(lm[ln], rm[r])
    fs, fk, fm = _cost_tree(ls, lk, lm)
    total, episodes, worst = float(fs[0]), int(fk[0]), float(fm[0])
    mean, nxt = 0.0, lam
    if episodes:
        mean = total / float(episodes)
        l = float(lam) + float(lambda_lr) * (mean - float(cost_limit))
        l = 0.0 if l < 0.0 else l
        l = float(lambda_max) if l > float(lambda_max) else l
        nxt = np.float32(l)
    summary = dict(episodes=episodes, cost_sum=total, cost_mean=mean, cost_max=worst if episodes else 0.0,
                   lambda_before=lam, lambda_after=nxt)
    return penalised, acc, episode_costs, summary, nxt


NORM_BLOCK = 256   # lanes per workgroup of k_ret_scan and k_ret_stats (pgtg_norm.h kNormBlock)
NORM_PARTIAL = 64  # envs per partial of a step: one wave (kNormPartial)
NORM_AHEAD = 8     # rows k_ret_scan keeps in flight, and steps whose trees it reduces side by side (kNormAhead)
NORM_RMS_INIT = (0.0, 1.0, 1e-4)  # RunningMeanStd's (mean, var, count) before any sample


def _ret_merge(a, b):
    """ret_merge of pgtg_norm.h on (n, mean, m2) triples of equal-shaped float64 arrays: Chan's count-aware merge,
    a then b, an empty operand returning the other unchanged."""
    import numpy as np
    (na, ma, sa), (nb, mb, sb) = a, b
    with np.errstate(divide="ignore", invalid="ignore"):
        n = na + nb
        d = mb - ma
        mean = ma + d * (nb / n)
        m2 = sa + sb + d * d * (na * nb / n)
    ea, eb = na == 0, nb == 0
    pick = lambda x, xa, xb: np.where(eb, xa, np.where(ea, xb, x))  # noqa: E731
    return pick(n, na, nb), pick(mean, ma, mb), pick(m2, sa, sb)


def _ret_tree(n, mean, m2):
    """The shuffle tree over the last axis (64 lanes): lane i merges lane i + o into itself for o = 32, 16, .. 1;
    returns lane 0's triple."""
    n, mean, m2 = n.copy(), mean.copy(), m2.copy()
    o = 32
    while o:
        r = _ret_merge((n[..., :o], mean[..., :o], m2[..., :o]), (n[..., o:2 * o], mean[..., o:2 * o], m2[..., o:2 * o]))
        n[..., :o], mean[..., :o], m2[..., :o] = r
        o >>= 1
    return n[..., 0], mean[..., 0], m2[..., 0]


def _ret_pad(x, width):
    """x [T, K] padded with zeros (empty partials) to a multiple of `width` columns, as [T, K / width, width]."""
    import numpy as np
    T, K = x.shape
    rows = -(-K // width)
    return np.concatenate([x, np.zeros((T, rows * width - K))], axis=1).reshape(T, rows, width)


def reward_norm_reference(rewards, dones, ret, rms, gamma, epsilon=1e-8, clip=10.0, training=True):
    """k_ret_scan, k_ret_stats and k_ret_apply (pgtg_norm.h; include/pgtg.h pgtg_reward_norm) in numpy float64,
    statement for statement and merge for merge: the reward half of SB3's VecNormalize.  rewards [T, N] float32;
    dones [T + 1, N] (row t + 1: the episode ended in step t); ret [N] float64, the discounted return of each
    env's episode under way; rms = (mean, var, count) of the returns seen so far.  Returns (normalised [T, N]
    float32, new ret [N], new rms float64 [3], row_var float64 [T]: the variance row t was divided with).
    training=False: ret and rms come back as they were and every row is divided by sqrt(rms[1] + epsilon).
    The moments of a step are merged in the kernels' order: 64 envs per wave by _ret_tree, the waves' partials
    by lane l taking partials l, l + 256, ... in order, those 256 by the same tree per wave and the four waves
    in wave order; then update_from_moments step by step."""
    import numpy as np
    rewards = np.asarray(rewards, dtype=np.float32)
    dones = np.asarray(dones) != 0
    T, N = rewards.shape
    gamma, epsilon, clip = float(gamma), float(epsilon), float(clip)
    ret = np.array(ret, dtype=np.float64).reshape(N)  # (a copy)
    mean, var, count = (float(x) for x in np.asarray(rms, dtype=np.float64).reshape(3))
    r64 = rewards.astype(np.float64)
    if training:
        # k_ret_scan: the returns of every step, then each wave's tree
        rets = np.empty((T, N))
        for t in range(T):
            ret = ret * gamma + r64[t]
            rets[t] = ret
            ret = np.where(dones[t + 1], 0.0, ret)
        leaves_n = _ret_pad(np.ones((T, N)), NORM_PARTIAL)
        pn, pm, ps = _ret_tree(leaves_n, _ret_pad(rets, NORM_PARTIAL), np.zeros_like(leaves_n))  # [T, W]
        # k_ret_stats, the merge: lane l takes the partials l, l + 256, ... in order
        ln, lm, ls = (_ret_pad(x, NORM_BLOCK) for x in (pn, pm, ps))  # [T, rounds, 256]
        acc = tuple(np.zeros((T, NORM_BLOCK)) for _ in range(3))
        for k in range(ln.shape[1]):
            acc = _ret_merge(acc, (ln[:, k], lm[:, k], ls[:, k]))
        wn, wm, ws = _ret_tree(*(x.reshape(T, NORM_BLOCK // 64, 64) for x in acc))  # [T, 4]
        b = (wn[:, 0], wm[:, 0], ws[:, 0])
        for w in range(1, NORM_BLOCK // 64):
            b = _ret_merge(b, (wn[:, w], wm[:, w], ws[:, w]))
        # k_ret_stats, the walk: RunningMeanStd.update_from_moments
        row_var = np.empty(T)
        for t in range(T):
            nb, mb = float(b[0][t]), float(b[1][t])
            vb = float(b[2][t]) / nb
            delta = mb - mean
            tot = count + nb
            nxt = mean + delta * nb / tot
            var = (var * count + vb * nb + delta * delta * count * nb / tot) / tot
            mean, count = nxt, tot
            row_var[t] = var
    else:
        row_var = np.full(T, var)
    # k_ret_apply
    with np.errstate(divide="ignore", invalid="ignore"):
        q = r64 / np.sqrt(row_var + epsilon)[:, None]
    q = np.where(q < -clip, -clip, q)
    q = np.where(q > clip, clip, q)
    with np.errstate(over="ignore"):
        normalised = q.astype(np.float32)
    return normalised, ret, np.array([mean, var, count]), row_var


PERM_ROUNDS = 6     # Feistel rounds of k_ppo_perm (pgtg_ppo_log.h kPermRounds)
PERM_WALK_CAP = 64  # cycle-walk steps of an element at most (kPermWalkCap)


def permutation_reference(total: int, seed: int, counter: int, return_walk: bool = False):
    """The permutation of [0, total) k_ppo_perm writes for (seed, counter), int64 [total], restated in numpy,
    bit-equal with the kernel: an alternating Feistel network over bits = ceil(log2 total) bits (the low
    bits // 2 and the high bits - bits // 2 take turns being xored with the round function of the other:
    policy_uniform's splitmix64 finaliser of (seed, counter, round, half) in a domain of its own), walked until
    the value falls below total.  Every element is computed on its own.  return_walk: also the longest walk."""
    import numpy as np
    total = int(total)
    if total < 1:
        raise ValueError("total must be at least 1")
    M = (1 << 64) - 1
    bits = (total - 1).bit_length()
    a, b = bits // 2, bits - bits // 2
    mask_a, mask_b = np.uint64((1 << a) - 1), np.uint64((1 << b) - 1)
    key = np.uint64((int(seed) & M) ^ ((int(counter) * 0x9E3779B97F4A7C15) & M) ^ 0x70706F5F7065726D)

    def f(half, rnd):
        with np.errstate(over="ignore"):
            z = key ^ (half * np.uint64(0xD1B54A32D192ED03)) ^ np.uint64(((rnd + 1) * 0xA0761D6478BD642F) & M)
            z = z + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))

    def feistel(x):
        lo, hi = x & mask_a, x >> np.uint64(a)
        for rnd in range(PERM_ROUNDS):
            if rnd & 1:
                hi = hi ^ (f(lo, rnd) & mask_b)
            else:
                lo = lo ^ (f(hi, rnd) & mask_a)
        return (hi << np.uint64(a)) | lo

    x = feistel(np.arange(total, dtype=np.uint64))
    walk = 1
    while True:
        out = x >= np.uint64(total)
        if not out.any():
            break
        if walk >= PERM_WALK_CAP:  # (the kernel flags these elements and writes their own index)
            x[out] = np.nonzero(out)[0].astype(np.uint64)
            break
        x[out] = feistel(x[out])
        walk += 1
    perm = x.astype(np.int64)
    return (perm, walk) if return_walk else perm


class Rollout:
    """One rollout of `n_steps` steps of every env of `env`, resident on its device (see the module text).

    Tensors (T = n_steps, N = env.num_envs, D = the flat observation's length):
      obs [T+1, N, D] int8 or float32 (row t: the observation step t acted on; row T: the next rollout's
      first; rows are padded to 16 bytes, so obs[t] is contiguous and obs as a whole need not be),
      actions [T, N] uint8, rewards [T, N] float32, dones [T+1, N] bool (row t = episode_starts of step t),
      truncated_only [T, N] bool, values / log_probs / terminal_values / advantages / returns [T, N]
      float32, terminal_obs [N, D] (the last step's terminal observations, valid on its finished envs).
    With cost_limit (an env with separate_reward_cost; None: nothing of this exists): costs, penalised_rewards
    [T, N] float32 and ep_cost [N] float64 (the cost of each env's episode under way); lambda_lr, lambda_init and
    lambda_max are the multiplier's step, start and upper clamp (include/pgtg.h pgtg_cost_scan).
    With norm_reward (False: nothing of this exists): normalised_rewards [T, N] float32, ret [N] float64 (the
    discounted return of each env's episode under way), ret_rms [3] float64 (mean, var, count of the returns seen
    so far) and row_var [T] float64; clip_reward, norm_epsilon and norm_gamma (None: gamma) are VecNormalize's
    clip_reward, epsilon and gamma (include/pgtg.h pgtg_reward_norm); norm_training (True) as its `training`."""

    def __init__(self, env, n_steps: int, gamma: float = 0.99, gae_lambda: float = 0.95, obs_dtype=None,
                 cost_limit=None, lambda_lr: float = 0.05, lambda_init: float = 0.0, lambda_max: float = 100.0,
                 norm_reward: bool = False, clip_reward: float = 10.0, norm_epsilon: float = 1e-8, norm_gamma=None):
        import math

        import torch
        obs_dtype = torch.int8 if obs_dtype is None else obs_dtype
        if isinstance(obs_dtype, str):
            obs_dtype = getattr(torch, obs_dtype)
        if int(n_steps) < 1:
            raise ValueError("n_steps must be at least 1")
        if not env.autoreset:
            raise ValueError("a rollout needs autoreset=True (a finished env restarts in the same step)")
        if obs_dtype not in (torch.int8, torch.float32):
            raise ValueError("obs_dtype: torch.int8 or torch.float32")
        try:
            check_flattenable(env.spec)
        except IndexError as e:
            raise ValueError(str(e)) from None
        self.env = env
        self.n_steps = T = int(n_steps)
        self.num_envs = N = env.num_envs
        self.obs_dim = D = flat_dim(env.spec)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.device = dev = env.device
        self._dtype_code = 0 if obs_dtype == torch.float32 else 1
        # k_flatten wants 16-byte aligned [N, D] buffers: each obs row starts on a multiple of 16 bytes
        item = torch.empty((), dtype=obs_dtype).element_size()
        pitch = (N * D * item + 15) // 16 * 16 // item
        self._obs_store = torch.zeros((T + 1) * pitch, dtype=obs_dtype, device=dev)
        self.obs = self._obs_store.as_strided((T + 1, N, D), (pitch, D, 1))
        self.terminal_obs = torch.zeros((N, D), dtype=obs_dtype, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.actions = torch.zeros((T, N), dtype=torch.uint8, device=dev)
        self.rewards = torch.zeros((T, N), **f32)
        self.dones = torch.zeros((T + 1, N), dtype=torch.bool, device=dev)
        self.truncated_only = torch.zeros((T, N), dtype=torch.bool, device=dev)
        self.values = torch.zeros((T, N), **f32)
        self.log_probs = torch.zeros((T, N), **f32)
        self.terminal_values = torch.zeros((T, N), **f32)
        self.advantages = torch.zeros((T, N), **f32)
        self.returns = torch.zeros((T, N), **f32)
        self.t = 0
        self._started = False  # the env has been reset into obs[0]
        self._finished = False
        self._last_values = None
        self._last_buf = None  # collect()'s V(obs[T])
        self.n_updates = 0      # epochs counted by every update() so far: SB3's _n_updates
        self._updates = 0       # update() calls so far: the counter of perm_seed's permutations
        self._train = None      # the last update's statistics buffer, shape and log
        self._stop_word = None  # target_kl's device word
        self._ev_ws = None      # k_ppo_expl_var's workspace
        self.cost_limit = None if cost_limit is None else float(cost_limit)
        self._cost_ts = ()
        if cost_limit is not None:
            if env.cost is None:
                raise ValueError("cost_limit needs an env with separate_reward_cost=True (it has no cost channel)")
            self.lambda_lr, self.lambda_max = float(lambda_lr), float(lambda_max)
            if not (math.isfinite(self.cost_limit) and math.isfinite(self.lambda_lr) and self.lambda_max >= 0.0
                    and 0.0 <= float(lambda_init) <= self.lambda_max):
                raise ValueError("cost_limit and lambda_lr must be finite, and 0 <= lambda_init <= lambda_max")
            nbytes = C.c_uint64()
            self._call(env._lib.pgtg_cost_workspace_bytes(N, C.byref(nbytes)))
            self.costs = torch.zeros((T, N), **f32)
            self.penalised_rewards = torch.zeros((T, N), **f32)
            self.ep_cost = torch.zeros(N, dtype=torch.float64, device=dev)
            self._lambda = torch.full((1,), float(lambda_init), **f32)
            self._cost_summary = torch.zeros(C.sizeof(_abi.PgtgCostSummary) // 8, dtype=torch.int64, device=dev)
            self._cost_ws = torch.empty(max(nbytes.value // 8, 1), dtype=torch.float64, device=dev)
            self._cost_ts = (self.costs, self.penalised_rewards, self.ep_cost, self._lambda, self._cost_summary,
                             self._cost_ws)
        self.norm_reward = bool(norm_reward)
        self._norm_ts = ()
        if self.norm_reward:
            self.clip_reward, self.norm_epsilon = float(clip_reward), float(norm_epsilon)
            self.norm_gamma = self.gamma if norm_gamma is None else float(norm_gamma)
            if not (math.isfinite(self.clip_reward) and self.clip_reward >= 0.0 and math.isfinite(self.norm_epsilon)
                    and self.norm_epsilon >= 0.0 and 0.0 <= self.norm_gamma <= 1.0):
                raise ValueError("clip_reward and norm_epsilon must be finite and at least 0, norm_gamma in [0, 1]")
            nbytes = C.c_uint64()
            self._call(env._lib.pgtg_reward_norm_workspace_bytes(N, T, C.byref(nbytes)))
            self.norm_training = True
            self.normalised_rewards = torch.zeros((T, N), **f32)
            self.ret = torch.zeros(N, dtype=torch.float64, device=dev)
            self.ret_rms = torch.tensor(NORM_RMS_INIT, dtype=torch.float64, device=dev)
            self.row_var = torch.zeros(T, dtype=torch.float64, device=dev)
            self._norm_ws = torch.empty(max(nbytes.value // 8, 1), dtype=torch.float64, device=dev)
            self._norm_ts = (self.normalised_rewards, self.ret, self.ret_rms, self.row_var, self._norm_ws)

    @property
    def nbytes(self) -> int:
        """Device bytes the rollout holds."""
        ts = (self._obs_store, self.terminal_obs, self.actions, self.rewards, self.dones, self.truncated_only,
              self.values, self.log_probs, self.terminal_values, self.advantages, self.returns) + self._cost_ts
        ts += self._norm_ts
        return sum(t.numel() * t.element_size() for t in ts)

    # -- recording -------------------------------------------------------------------------------
    def reset(self) -> None:
        """Have the next begin() reset the env again (a new run, not the continuation of the last rollout)."""
        self._started = False

    def begin(self, seed=None):
        """Start a rollout and return obs[0].  The first call (and the first after reset(), and any call
        with a seed) resets the env with its observation written into obs[0], and sets dones[0] = 1: every
        env starts an episode, SB3's _last_episode_starts.  A later call continues where the last rollout
        ended: row T of obs and dones becomes row 0."""
        env, T = self.env, self.n_steps
        if not self._started or seed is not None:
            env.set_flat_scalars(None, None, None)  # (the reset's observation pass writes no step scalars)
            env.set_flat_outputs(self.obs[0], self.terminal_obs)
            env.reset(seed=seed)
            self.dones[0].fill_(True)
            if self.cost_limit is not None:
                self.ep_cost.zero_()  # (every env starts an episode)
            if self.norm_reward:
                self.ret.zero_()  # (VecNormalize.reset: the returns restart, the statistics stay)
            self._started = True
        else:
            self.obs[0].copy_(self.obs[T])
            self.dones[0].copy_(self.dones[T])
        self.terminal_values.zero_()  # (rows set_terminal_values is not called for stay zero)
        self.t = 0
        self._finished = False
        return self.obs[0]

    @staticmethod
    def _into(row, src) -> None:
        if src is not None and not (src.data_ptr() == row.data_ptr() and src.dtype == row.dtype
                                    and src.shape == row.shape and src.is_contiguous()):
            row.copy_(src.reshape(row.shape))

    def step(self, actions, values=None, log_probs=None):
        """One tick of every env from `actions` ([N] device tensor), recorded as step t: the step's
        kernels write obs[t+1], rewards[t], dones[t+1], truncated_only[t] and terminal_obs themselves.
        Launch-free beyond the tick only for uint8 actions that ARE the row (ro.actions[t]); another uint8
        tensor costs one copy into the row, and any other integer dtype a few torch kernels more (every
        value outside Discrete(9) becomes the invalid code 255, as in PGTGSB3VecEnv.step_async; the step
        kernel records it per env, see PGTGVecEnv.error_count).  values / log_probs ([N]) are copied into
        their rows unless they are the rows (ro.values[t], ro.log_probs[t]): a policy that writes into the
        rows adds nothing.  Returns views (obs[t+1], rewards[t], dones[t+1])."""
        import torch
        t, env = self.t, self.env
        if not self._started:
            raise RuntimeError("begin() first")
        if t >= self.n_steps:
            raise RuntimeError(f"the rollout is full ({self.n_steps} steps): finish() and begin() again")
        a = self.actions[t]
        if actions.dtype != torch.uint8:  # every value outside Discrete(9) becomes the invalid code 255
            actions = actions.to(torch.int64)
            actions = torch.where((actions < 0) | (actions > 8), torch.full_like(actions, 255), actions)
        self._into(a, actions)
        self._into(self.values[t], values)
        self._into(self.log_probs[t], log_probs)
        env._bind_flat_ptrs(self.obs[t + 1], self.terminal_obs, self._dtype_code)
        env._bind_flat_scalar_ptrs(self.rewards[t], self.dones[t + 1], self.truncated_only[t])
        if self.cost_limit is not None:
            env._bind_flat_cost_ptr(self.costs[t])
        env.step_actions(a)
        self.t = t + 1
        return self.obs[t + 1], self.rewards[t], self.dones[t + 1]

    def set_terminal_values(self, v) -> None:
        """V(terminal_obs) of the step just taken, all N rows (used on the truncated-only ones):
        terminal_values[t-1].  Not called: the row stays zero (no bootstrap)."""
        if self.t < 1:
            raise RuntimeError("no step has been taken")
        self._into(self.terminal_values[self.t - 1], v)

    def act(self, policy):
        """Step t with a DevicePolicy: one launch of k_policy on obs[t] into actions[t], values[t] and
        log_probs[t], then step() with those rows (which copies nothing), and, when the env has a time limit,
        V(terminal_obs) into terminal_values[t] by the kernel's value-only mode.  No torch kernel."""
        t = self.t
        if self._dtype_code != 1:
            raise ValueError("a policy acts on int8 rows: build the rollout with obs_dtype=torch.int8 "
                             "(step() takes a float32 rollout's actions)")
        if not self._started:
            raise RuntimeError("begin() first")
        if t >= self.n_steps:
            raise RuntimeError(f"the rollout is full ({self.n_steps} steps): finish() and begin() again")
        a, v, lp = policy.act(self.obs[t], self.actions[t], self.values[t], self.log_probs[t])
        out = self.step(a, v, lp)
        if self.env.max_episode_steps:
            policy.value(self.terminal_obs, out=self.terminal_values[t])
        return out

    def collect(self, policy) -> None:
        """A whole rollout with a DevicePolicy: begin() unless one is under way, T times act(), then
        finish() on V(obs[T]) written into a buffer the rollout keeps.  Only this library's kernels are
        launched by the steps and by finish() (the policy, the tick, the terminal values; k_gae), and nothing
        synchronises with the host; begin() continuing a rollout copies row T to row 0 as it always did."""
        import torch
        if self._dtype_code != 1:
            raise ValueError("a policy acts on int8 rows: build the rollout with obs_dtype=torch.int8")
        if not self._started or self._finished or self.t >= self.n_steps:
            self.begin()
        while self.t < self.n_steps:
            self.act(policy)
        if self._last_buf is None:
            self._last_buf = torch.zeros(self.num_envs, dtype=torch.float32, device=self.device)
        self.finish(policy.value(self.obs[self.n_steps], out=self._last_buf))

    def finish(self, last_values) -> None:
        """advantages and returns of the whole rollout in one launch of k_gae; last_values = V(obs[T]).
        With cost_limit, k_cost_scan and k_cost_dual run first and k_gae takes penalised_rewards as its rewards
        (`rewards` keeps the raw reward).  With norm_reward, k_ret_scan, k_ret_stats and k_ret_apply run before
        either (only k_ret_apply when norm_training is False), and what follows takes normalised_rewards: the
        normalisation wraps the env, so the penalty and the advantages act on what the agent sees."""
        import torch
        env, T, N = self.env, self.n_steps, self.num_envs
        if self.t != T:
            raise RuntimeError(f"finish() after {self.t} of {T} steps")
        lv = last_values.to(device=self.device, dtype=torch.float32).reshape(N).contiguous()
        self._last_values = lv  # (the launch reads it)
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        rewards = self.rewards
        env._bind_stream()
        if self.norm_reward:
            r = _abi.PgtgRewardNorm(n=N, steps=T, gamma=self.norm_gamma, epsilon=self.norm_epsilon, clip=self.clip_reward,
                                    training=int(bool(self.norm_training)), rewards=p(rewards), dones=p(self.dones),
                                    returns=p(self.ret), rms=p(self.ret_rms), row_var=p(self.row_var),
                                    normalised=p(self.normalised_rewards), workspace=p(self._norm_ws))
            self._call(env._lib.pgtg_reward_norm(env._h, C.byref(r)))
            rewards = self.normalised_rewards
        if self.cost_limit is not None:
            c = _abi.PgtgCost(n=N, steps=T, rewards=p(rewards), costs=p(self.costs), dones=p(self.dones),
                              ep_cost=p(self.ep_cost), penalised=p(self.penalised_rewards), lambda_=p(self._lambda),
                              cost_limit=self.cost_limit, lambda_lr=self.lambda_lr, lambda_max=self.lambda_max,
                              summary=p(self._cost_summary), workspace=p(self._cost_ws))
            self._call(env._lib.pgtg_cost_scan(env._h, C.byref(c)))
            rewards = self.penalised_rewards
        g = _abi.PgtgGae(n=N, steps=T, gamma=self.gamma, gae_lambda=self.gae_lambda, rewards=p(rewards),
                         values=p(self.values), dones=p(self.dones), truncated_only=p(self.truncated_only),
                         terminal_values=p(self.terminal_values), last_values=p(lv), advantages=p(self.advantages),
                         returns=p(self.returns))
        rc = env._lib.pgtg_gae(env._h, C.byref(g))
        if rc != _abi.PGTG_OK:
            from .vector import _check
            _check(rc, env._h)
        self._finished = True

    # -- the cost channel ----------------------------------------------------------------------
    def _need_cost(self) -> None:
        if self.cost_limit is None:
            raise RuntimeError("the rollout was built without cost_limit")

    def cost_log(self) -> dict:
        """The cost summary of the last finish(): cost/ep_cost_mean and cost/ep_cost_max over the episodes that
        ended inside the rollout (cost/episodes of them; 0.0 without any), cost/lambda the multiplier the
        rollout was penalised with and cost/lambda_next the one the next will be.  One synchronisation."""
        self._need_cost()
        if not self._finished:
            raise RuntimeError("finish() first")
        s = _abi.PgtgCostSummary.from_buffer_copy(self._cost_summary.cpu().numpy().tobytes())
        return {"cost/ep_cost_mean": s.cost_mean, "cost/ep_cost_max": s.cost_max, "cost/episodes": int(s.episodes),
                "cost/lambda": s.lambda_before, "cost/lambda_next": s.lambda_after}

    @property
    def lagrange_multiplier(self) -> float:
        """The multiplier the next finish() penalises with (float32).  Reading synchronises; setting writes
        the device word from the host (checkpoints)."""
        self._need_cost()
        return float(self._lambda.item())

    @lagrange_multiplier.setter
    def lagrange_multiplier(self, value) -> None:
        self._need_cost()
        if not 0.0 <= float(value) <= self.lambda_max:
            raise ValueError("the multiplier lies in [0, lambda_max]")
        self._lambda.fill_(float(value))

    # -- reward normalisation ------------------------------------------------------------------
    def _need_norm(self) -> None:
        if not self.norm_reward:
            raise RuntimeError("the rollout was built without norm_reward")

    def reward_norm_state(self) -> dict:
        """Host copies of the running statistics and the returns under way: {"mean", "var", "count"} (floats)
        and "ret" (float64 numpy [N]) -- what VecNormalize.save keeps of the reward half.  Synchronises."""
        self._need_norm()
        mean, var, count = self.ret_rms.cpu().tolist()
        return {"mean": mean, "var": var, "count": count, "ret": self.ret.cpu().numpy().copy()}

    def load_reward_norm_state(self, state: dict) -> None:
        """Restore what reward_norm_state() returned (a checkpoint's): the device words are written from the host."""
        import numpy as np
        import torch
        self._need_norm()
        ret = np.asarray(state["ret"], dtype=np.float64)
        if ret.shape != (self.num_envs,):
            raise ValueError(f"ret: a float64 array of shape ({self.num_envs},)")
        rms = [float(state["mean"]), float(state["var"]), float(state["count"])]
        self.ret_rms.copy_(torch.tensor(rms, dtype=torch.float64))
        self.ret.copy_(torch.from_numpy(np.ascontiguousarray(ret)))

    def norm_log(self) -> dict:
        """The running statistics of the discounted return as they stand.  One synchronisation."""
        self._need_norm()
        mean, var, count = self.ret_rms.cpu().tolist()
        return {"norm/ret_mean": mean, "norm/ret_var": var, "norm/count": count}

    # -- minibatches ---------------------------------------------------------------------------
    def get(self, batch_size: int | None = None, indices=None):
        """Minibatches (obs float32 [B, D], actions int64 [B], values, log_probs, advantages, returns [B])
        of the finished rollout.  Sample s is (env, step) = sample_index(s, T), SB3's swap_and_flatten
        order, so SB3's permutation gives SB3's minibatches; indices=None draws torch.randperm on the
        device; batch_size=None gives one batch of everything.  Torch indexing, no kernel of this library."""
        import torch
        if not self._finished:
            raise RuntimeError("finish() first")
        T, total = self.n_steps, self.n_steps * self.num_envs
        if indices is None:
            indices = torch.randperm(total, device=self.device)
        idx = torch.as_tensor(indices, device=self.device).to(torch.int64).reshape(-1)
        bs = idx.numel() if batch_size is None else int(batch_size)
        if bs < 1:
            raise ValueError("batch_size must be at least 1")
        for lo in range(0, idx.numel(), bs):
            e, t = sample_index(idx[lo:lo + bs], T)
            yield (self.obs[t, e].to(torch.float32), self.actions[t, e].to(torch.int64), self.values[t, e],
                   self.log_probs[t, e], self.advantages[t, e], self.returns[t, e])

    # -- the PPO update ---------------------------------------------------------------------------
    def _call(self, rc: int) -> None:
        if rc != _abi.PGTG_OK:
            from .vector import _check
            _check(rc, self.env._h)

    def permutation(self, seed: int, counter: int, out=None):
        """The permutation of [0, T * N) of (seed, counter) as an int64 device tensor: one launch of k_ppo_perm
        (include/pgtg.h pgtg_ppo_perm; permutation_reference restates it), no torch kernel."""
        import torch
        total = self.n_steps * self.num_envs
        if out is None:
            out = torch.empty(total, dtype=torch.int64, device=self.device)
        m = (1 << 64) - 1
        self.env._bind_stream()
        self._call(self.env._lib.pgtg_ppo_perm(self.env._h, total, int(seed) & m, int(counter) & m,
                                               C.c_void_p(out.data_ptr())))
        return out

    def explained_variance(self, out=None):
        """{1 - r, r}, r = var(returns - values) / var(returns), of the finished rollout as a float32 [2] device
        tensor: SB3's explained_variance and the ratio it is one minus (three launches of k_ppo_expl_var,
        include/pgtg.h pgtg_ppo_expl_var; nothing synchronises)."""
        import torch
        if not self._finished:
            raise ValueError("the rollout is not finished: collect() or finish() first")
        if self._ev_ws is None:
            nbytes = C.c_uint64()
            self._call(self.env._lib.pgtg_ppo_expl_var_workspace_bytes(C.byref(nbytes)))
            self._ev_ws = torch.empty(nbytes.value // 8, dtype=torch.float64, device=self.device)
        if out is None:
            out = torch.empty(2, dtype=torch.float32, device=self.device)
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        self.env._bind_stream()
        self._call(self.env._lib.pgtg_ppo_expl_var(self.env._h, p(self.values), p(self.returns),
                                                   self.n_steps * self.num_envs, p(self._ev_ws), p(out)))
        return out

    def _read_log(self) -> dict:
        """Launch the explained variance and k_ppo_log over the last update's statistics, read the struct back
        (the one host synchronisation) and keep the dict."""
        import torch
        st = self._train
        ev = self.explained_variance()
        raw = torch.empty(C.sizeof(_abi.PgtgPpoLog), dtype=torch.uint8, device=self.device)
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        self.env._bind_stream()
        self._call(self.env._lib.pgtg_ppo_log(self.env._h, p(st["stats"]), st["M"], st["per_epoch"], p(st["stop"]), p(ev),
                                              p(raw)))
        log = _abi.PgtgPpoLog.from_buffer_copy(raw.cpu().numpy().tobytes())
        st["log"] = dict(entropy_loss=log.entropy_loss, policy_gradient_loss=log.policy_gradient_loss,
                         value_loss=log.value_loss, approx_kl=log.approx_kl, clip_fraction=log.clip_fraction,
                         loss=log.loss, explained_variance=log.explained_variance, n_updates=None,
                         early_stop=bool(log.early_stop), minibatches=int(log.minibatches), epochs=int(log.epochs),
                         variance_ratio=log.variance_ratio)
        return st["log"]

    def train_log(self) -> dict:
        """SB3's train/ log of the last update(): entropy_loss, policy_gradient_loss, value_loss and
        clip_fraction (means over the minibatches run), approx_kl (mean over the last run epoch), loss (the last
        run minibatch's), explained_variance (of the rollout's values against its returns, as they stand now),
        n_updates (the epochs counted by every update() of this rollout so far, SB3's _n_updates), early_stop
        and minibatches (target_kl), plus epochs and variance_ratio (1 - explained_variance before its
        rounding).  Reduced on the device (k_ppo_expl_var, k_ppo_log: four launches); this call synchronises
        the host, once; after an update with target_kl it returns what that update already read."""
        st = self._train
        if st is None:
            raise RuntimeError("update() first")
        if st["M"] == 0:
            nan = float("nan")
            log = dict(entropy_loss=nan, policy_gradient_loss=nan, value_loss=nan, approx_kl=nan, clip_fraction=nan,
                       loss=nan, explained_variance=nan, early_stop=False, minibatches=0, epochs=0, variance_ratio=nan)
        else:
            log = dict(st["log"] if st["log"] is not None else self._read_log())
        log["n_updates"] = self.n_updates
        return log

    def update(self, policy, module, optimizer, n_epochs: int = 10, batch_size: int = 64, clip_range: float = 0.2,
               ent_coef: float = 0.0, vf_coef: float = 0.5, max_grad_norm: float = 0.5,
               normalize_advantage: bool = True, generator=None, clip_range_vf=None, target_kl=None,
               perm_seed=None) -> list:
        """SB3's PPO.train loop over the finished rollout with the library's gradient: per epoch one
        torch.randperm(T * N) on the device (from `generator` if given), per minibatch of batch_size samples
        policy.ppo_grad (k_ppo_loss, k_ppo_dw1, k_ppo_reduce on the int8 rows) straight into the .grad tensors
        of `module` (an MlpPolicyReference on the env's device whose weights `policy` holds), then torch's
        clip_grad_norm_, optimizer.step() and policy.load_state_dict(module.state_dict()).  Returns the
        per-minibatch stats tensors (policy.STAT_NAMES), still on the device (rows of one [M, 8] buffer);
        nothing synchronises.
        With a policy.DeviceAdam over (policy, module) as the optimizer a minibatch is this library's launches
        alone: policy.adv_stats (k_ppo_adv_stats; when normalising more than one sample), policy.ppo_grad with
        those statistics, and optimizer.step(max_grad_norm=...) (k_ppo_gnorm, k_ppo_adam: clip, Adam and the
        repack) -- no clip_grad_norm_ and no load_state_dict.
        clip_range_vf: SB3's value-function clipping against the rollout's values (None: none).
        perm_seed: None keeps torch.randperm and `generator`; an int draws epoch k of this rollout's u-th update
        (u = 0, 1, ...) as permutation(perm_seed, u * n_epochs + k) by k_ppo_perm, a function of those numbers
        alone on any build, and then a DeviceAdam update launches no torch kernel at all.
        target_kl: SB3's early stop, approx_kl > 1.5 * target_kl before a minibatch's optimiser step ends the
        update.  With a DeviceAdam nothing synchronises per minibatch: a device word stop_at (zeroed on the
        stream as the update starts) is set by the stopping minibatch's own k_ppo_reduce, every later launch
        returns at its gate, and the host reads the word once, at the end, with the log (train_log() then costs
        nothing more): the one synchronisation of the update.  optimizer.step_count is set from that read, and
        the returned list is cut to the minibatches run.  With a torch.optim optimizer, approx_kl is read on the
        host per minibatch and the loop breaks, as SB3's does.
        ValueError for a negative or non-finite clip_range_vf or target_kl, with nothing launched."""
        import torch
        from .policy import DeviceAdam, check_clip_range_vf, check_target_kl
        if not self._finished:
            raise ValueError("the rollout is not finished: collect() or finish() first")
        if int(batch_size) < 1 or int(n_epochs) < 0:
            raise ValueError("batch_size must be at least 1 and n_epochs at least 0")
        clip_range_vf, target_kl = check_clip_range_vf(clip_range_vf), check_target_kl(target_kl)
        params = dict(module.named_parameters())
        grads = {}
        for key, p in params.items():
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            grads[key] = p.grad
        n_epochs, bs = int(n_epochs), int(batch_size)
        total = self.n_steps * self.num_envs
        per_epoch = (total + bs - 1) // bs
        M = n_epochs * per_epoch
        device_adam = isinstance(optimizer, DeviceAdam)
        if device_adam and (optimizer.policy is not policy or optimizer.module is not module):
            raise ValueError("the DeviceAdam was built over another policy or module")
        stats = torch.empty((max(M, 1), 8), dtype=torch.float32, device=self.device)
        stop = None
        if target_kl is not None:
            if self._stop_word is None:
                self._stop_word = torch.zeros(1, dtype=torch.int32, device=self.device)
            stop = self._stop_word
            stop.zero_()
        self._train = dict(stats=stats, M=M, per_epoch=per_epoch, stop=stop, log=None)
        u = self._updates
        self._updates += 1

        def epoch_perm(k):
            if perm_seed is None:
                return torch.randperm(total, device=self.device, generator=generator)
            return self.permutation(perm_seed, u * n_epochs + k)

        common = dict(grads=grads, clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef,
                      normalize_advantage=normalize_advantage, clip_range_vf=clip_range_vf)
        run = M
        if device_adam:
            count_before = optimizer.step_count
            gate = {} if stop is None else dict(stop_at=stop)
            m = 0
            for k in range(n_epochs):
                perm = epoch_perm(k)
                for lo in range(0, total, bs):
                    m += 1
                    if stop is not None:
                        gate["ordinal"] = m
                    idx = perm[lo:lo + bs]
                    st = policy.adv_stats(self, idx, **gate) if normalize_advantage and idx.numel() > 1 else None
                    policy.ppo_grad(self, idx, adv_stats=st, stats_out=stats[m - 1], target_kl=target_kl, **gate, **common)
                    optimizer.step(grads=grads, max_grad_norm=max_grad_norm, **gate)
            if stop is not None and M:
                log = self._read_log()  # (the one synchronisation: stop_at and the log together)
                run = log["minibatches"]
                optimizer.step_count = count_before + (run - 1 if log["early_stop"] else M)
                self.n_updates += log["epochs"]
            else:
                self.n_updates += n_epochs
            return [stats[i] for i in range(run)]
        m, stopped = 0, False
        for k in range(n_epochs):
            perm = epoch_perm(k)
            for lo in range(0, total, bs):
                m += 1
                policy.ppo_grad(self, perm[lo:lo + bs], stats_out=stats[m - 1], **common)
                if target_kl is not None and bool(stats[m - 1, 4] > 1.5 * target_kl):  # (a host read, as SB3's)
                    stopped = True
                    break
                torch.nn.utils.clip_grad_norm_(params.values(), max_grad_norm)
                optimizer.step()
                policy.load_state_dict(module.state_dict())
            self.n_updates += 1
            if stopped:
                stop.fill_(m)  # (k_ppo_log reads the word)
                run = m
                break
        return [stats[i] for i in range(run)]

    def close(self) -> None:
        """Unbind the flat rows and scalars from the handle (the tensors stay valid)."""
        env = self.env
        if env is not None and getattr(env, "_h", None):
            env.set_flat_outputs(None, None)
            env.set_flat_scalars(None, None, None)  # (and with them the cost row)
        self._started = False
