"""SB3's MlpPolicy for acting, on the device: the policy of the PPO of pgtg/train.py:61-74.

`PPO("MlpPolicy", env)` builds an `ActorCriticPolicy` with two separate 64-64 tanh towers, a 9-way
categorical head and a scalar value head.  `DevicePolicy` runs its forward pass for acting as one launch
of the HIP kernel k_policy (include/pgtg.h pgtg_policy): it reads the int8 flat rows where k_flatten left
them and writes the action, the value and the log-probability of every env into the rows it is given --
`Rollout.collect(policy)` is a whole rollout without a torch kernel or a host synchronisation.
`MlpPolicyReference` is the module a trainer optimises (SB3's parameter names and initialisation, so a
real `policy.state_dict()` loads into it), and `DevicePolicy.load_state_dict` hands the updated weights to
the kernel by a device-side repack (k_policy_pack).  `DevicePolicy.ppo_grad` is one PPO minibatch of
SB3's `PPO.train` on the device (include/pgtg.h pgtg_ppo_grad: k_ppo_loss, k_ppo_dw1, k_ppo_reduce): the loss,
its statistics and the gradient of all twelve tensors from the rollout's int8 rows, written into the module's
`.grad` tensors; `Rollout.update` is the loop around it.  `DeviceAdam` is the optimiser step on the device
(pgtg_ppo_step: k_ppo_gnorm, k_ppo_adam): the global-norm clip, Adam and the repack of the new weights for
k_policy in two launches; with it (and `DevicePolicy.adv_stats`, k_ppo_adv_stats) a minibatch of
`Rollout.update` is six launches of this library and nothing else.  With a torch optimiser the loop keeps
torch's norm clip, `optimizer.step()` and a repack per minibatch.

    policy = DevicePolicy(env)
    policy.load_state_dict(module.state_dict())
    opt = DeviceAdam(policy, module, lr=3e-4)           # or torch.optim.Adam(module.parameters(), ...)
    ro.collect(policy)
    ro.update(policy, module, opt)                      # n_epochs x minibatches

`policy_reference` restates the whole function in numpy at a chosen precision, `ppo_reference` the PPO loss
and its hand-derived gradient, `policy_adam_reference` the clip and Adam step, and `policy_uniform` the kernel's counter-based uniform draw (SB3 is not a dependency; the restatements are the tests' yardstick,
as gae_reference is).
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import numpy as np
import torch
from torch import nn

from . import _abi

HIDDEN = 64
N_ACTIONS = 9
K_CHUNK = 256  # observation bytes of a row the kernel stages at a time (pgtg_policy_chunk())
SAMPLE, ARGMAX, VALUE_ONLY = _abi.PGTG_POLICY_SAMPLE, _abi.PGTG_POLICY_ARGMAX, _abi.PGTG_POLICY_VALUE_ONLY

# ABI field -> (state-dict key, shape with D for obs_dim)
WEIGHT_KEYS = {
    "w1p": ("mlp_extractor.policy_net.0.weight", (HIDDEN, "D")), "b1p": ("mlp_extractor.policy_net.0.bias", (HIDDEN,)),
    "w2p": ("mlp_extractor.policy_net.2.weight", (HIDDEN, HIDDEN)), "b2p": ("mlp_extractor.policy_net.2.bias", (HIDDEN,)),
    "wa": ("action_net.weight", (N_ACTIONS, HIDDEN)), "ba": ("action_net.bias", (N_ACTIONS,)),
    "w1v": ("mlp_extractor.value_net.0.weight", (HIDDEN, "D")), "b1v": ("mlp_extractor.value_net.0.bias", (HIDDEN,)),
    "w2v": ("mlp_extractor.value_net.2.weight", (HIDDEN, HIDDEN)), "b2v": ("mlp_extractor.value_net.2.bias", (HIDDEN,)),
    "wv": ("value_net.weight", (1, HIDDEN)), "bv": ("value_net.bias", (1,)),
}

PolicyOutput = collections.namedtuple("PolicyOutput", "actions values log_probs logits")


def weight_shapes(obs_dim: int) -> dict:
    """{state-dict key: shape} of SB3's MlpPolicy for a flat observation of obs_dim values."""
    return {key: tuple(obs_dim if s == "D" else s for s in shape) for key, shape in WEIGHT_KEYS.values()}


def policy_uniform(seed: int, counter: int, env):
    """The kernel's own uniform draw: float32 in [0, 1), a multiple of 2^-24, from splitmix64 of
    (seed, draw counter, global env index) -- no state anywhere.  env: an int or an array of ints."""
    M = (1 << 64) - 1
    with np.errstate(over="ignore"):
        e = np.asarray(env, dtype=np.uint64)
        z = np.uint64(seed & M) ^ np.uint64((counter * 0x9E3779B97F4A7C15) & M) ^ (e * np.uint64(0xD1B54A32D192ED03))
        z = z ^ np.uint64(0x706F6C6963795F75)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def inverse_cdf(logits, u, dtype=np.float64):
    """The kernel's sampling rule at precision dtype: p = exp(logits - max) / sum, c_a its running sum in
    action order, the action is the least a with u < c_a, and 8 where rounding leaves c_8 <= u.
    logits [N, 9], u [N]; returns (actions uint8 [N], c [N, 9])."""
    lg = np.asarray(logits, dtype=dtype)
    ex = np.exp(lg - lg.max(axis=1, keepdims=True))
    p = ex / ex.sum(axis=1, keepdims=True, dtype=dtype)
    c = np.zeros_like(p)
    run = np.zeros(len(p), dtype=dtype)
    for a in range(p.shape[1]):  # (a running sum in action order, at dtype)
        run = (run + p[:, a]).astype(dtype)
        c[:, a] = run
    below = np.asarray(u, dtype=dtype)[:, None] < c
    act = np.where(below.any(axis=1), below.argmax(axis=1), p.shape[1] - 1)
    return act.astype(np.uint8), c


def policy_reference(state_dict, obs_int8, uniforms=None, mode=SAMPLE, dtype=np.float64, *, seed=0, counter=0,
                     env_offset=0) -> PolicyOutput:
    """What k_policy computes, in numpy at precision dtype: obs_int8 [N, D] signed bytes, uniforms [N]
    (SAMPLE; None draws policy_uniform(seed, counter, env_offset + e)).  Returns PolicyOutput(actions uint8,
    values, log_probs, logits [N, 9]); VALUE_ONLY gives None for everything but values."""
    if mode not in (SAMPLE, ARGMAX, VALUE_ONLY):
        raise ValueError("mode: SAMPLE, ARGMAX or VALUE_ONLY")
    x = np.asarray(obs_int8)
    if x.dtype != np.int8 or x.ndim != 2:
        raise ValueError("obs_int8: an int8 [N, D] array")
    w = {f: np.asarray(_host(state_dict[key]), dtype=dtype) for f, (key, _) in WEIGHT_KEYS.items()}
    x = x.astype(dtype)
    tower = lambda w1, b1, w2, b2: np.tanh(np.tanh(x @ w[w1].T + w[b1]) @ w[w2].T + w[b2])  # noqa: E731
    values = (tower("w1v", "b1v", "w2v", "b2v") @ w["wv"].T + w["bv"])[:, 0]
    if mode == VALUE_ONLY:
        return PolicyOutput(None, values, None, None)
    logits = tower("w1p", "b1p", "w2p", "b2p") @ w["wa"].T + w["ba"]
    if mode == ARGMAX:
        actions = logits.argmax(axis=1).astype(np.uint8)  # (numpy: the first of the maxima)
    else:
        if uniforms is None:
            uniforms = policy_uniform(seed, counter, env_offset + np.arange(len(x), dtype=np.uint64))
        actions, _ = inverse_cdf(logits, uniforms, dtype)
    mx = logits.max(axis=1)
    lse = mx + np.log(np.exp(logits - mx[:, None]).sum(axis=1, dtype=dtype))
    log_probs = logits[np.arange(len(x)), actions] - lse
    return PolicyOutput(actions, values, log_probs, logits)


def _host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t


STAT_NAMES = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")


def check_clip_range_vf(clip_range_vf):
    """clip_range_vf as a float, or None; ValueError for a negative or non-finite one."""
    if clip_range_vf is None:
        return None
    c = float(clip_range_vf)
    if not (math.isfinite(c) and c >= 0.0):
        raise ValueError("clip_range_vf must be finite and at least 0 (None: no value clipping)")
    return c


def ppo_terms(state_dict, obs_int8, actions, old_log_probs, advantages, returns, clip_range, ent_coef, vf_coef,
              normalize, dtype=np.float64, clip_range_vf=None, old_values=None) -> dict:
    """Every intermediate of one PPO minibatch at precision dtype (ppo_reference's working; the tests take the
    accumulated magnitudes from it): the layers' inputs `x, h1p, h2p, h1v, h2v`, the derivatives of the loss
    with respect to the layers' pre-activations `dz1p, dz2p, dlogits, dz1v, dz2v, dvalue` (already divided
    by B), and the per-sample terms of the statistics `t_policy, t_value, t_entropy, ratio, log_ratio, clipped`.
    clip_range_vf with old_values [B]: SB3's value clipping, values_pred = old_values + clamp(value - old_values,
    -c, c) in the value loss; the clamp passes the gradient on the closed interval, as torch's does."""
    clip_range_vf = check_clip_range_vf(clip_range_vf)
    if clip_range_vf is not None and old_values is None:
        raise ValueError("clip_range_vf needs old_values")
    x = np.asarray(obs_int8)
    if x.dtype != np.int8 or x.ndim != 2:
        raise ValueError("obs_int8: an int8 [B, D] array")
    w = {f: np.asarray(_host(state_dict[key]), dtype=dtype) for f, (key, _) in WEIGHT_KEYS.items()}
    x = x.astype(dtype)
    B = len(x)
    act = np.asarray(_host(actions)).astype(np.int64)
    old = np.asarray(_host(old_log_probs), dtype=dtype)
    adv = np.asarray(_host(advantages), dtype=dtype)
    ret = np.asarray(_host(returns), dtype=dtype)
    if normalize and B > 1:  # (SB3: the unbiased std; skipped for a batch of one)
        adv = (adv - adv.mean(dtype=dtype)) / (adv.std(ddof=1, dtype=dtype) + dtype(1e-8))
    c, ec, vc = dtype(clip_range), dtype(ent_coef), dtype(vf_coef)
    h1p = np.tanh(x @ w["w1p"].T + w["b1p"])
    h2p = np.tanh(h1p @ w["w2p"].T + w["b2p"])
    h1v = np.tanh(x @ w["w1v"].T + w["b1v"])
    h2v = np.tanh(h1v @ w["w2v"].T + w["b2v"])
    logits = h2p @ w["wa"].T + w["ba"]
    value = (h2v @ w["wv"].T + w["bv"])[:, 0]
    mx = logits.max(axis=1, keepdims=True)
    lsm = logits - (mx + np.log(np.exp(logits - mx).sum(axis=1, keepdims=True, dtype=dtype)))
    p = np.exp(lsm)
    ar = np.arange(B)
    log_ratio = lsm[ar, act] - old
    ratio = np.exp(log_ratio)
    p1, p2 = adv * ratio, adv * np.clip(ratio, 1 - c, 1 + c)
    entropy = -(p * lsm).sum(axis=1, dtype=dtype)
    through = (p1 < p2) | ((ratio >= 1 - c) & (ratio <= 1 + c))
    g_logp = np.where(through, -adv * ratio, 0).astype(dtype)
    onehot = np.zeros_like(p)
    onehot[ar, act] = 1
    dlogits = (g_logp[:, None] * (onehot - p) + ec * (p * (lsm + entropy[:, None]))) / dtype(B)
    value_pred, v_through = value, np.ones(B, dtype=bool)
    if clip_range_vf is not None:
        cv, ov = dtype(clip_range_vf), np.asarray(_host(old_values), dtype=dtype).reshape(B)
        dd = value - ov
        v_through = (dd >= -cv) & (dd <= cv)
        value_pred = np.where(v_through, value, ov + np.clip(dd, -cv, cv))  # (inside, old + (value - old) is the value)
    dvalue = np.where(v_through, vc * (-2 * (ret - value_pred)) / dtype(B), 0).astype(dtype)
    dz2p = (dlogits @ w["wa"]) * (1 - h2p * h2p)
    dz1p = (dz2p @ w["w2p"]) * (1 - h1p * h1p)
    dz2v = (dvalue[:, None] * w["wv"]) * (1 - h2v * h2v)
    dz1v = (dz2v @ w["w2v"]) * (1 - h1v * h1v)
    return dict(x=x, h1p=h1p, h2p=h2p, h1v=h1v, h2v=h2v, dz1p=dz1p, dz2p=dz2p, dlogits=dlogits, dz1v=dz1v, dz2v=dz2v,
                dvalue=dvalue, t_policy=-np.minimum(p1, p2), t_value=(ret - value_pred) ** 2, t_entropy=-entropy, ratio=ratio,
                log_ratio=log_ratio, clipped=(np.abs(ratio - 1) > c).astype(dtype), p=p, lsm=lsm, adv=adv, value=value,
                v_through=v_through)


# state-dict key of a layer's weight -> (its pre-activation derivative, its input) in ppo_terms
PPO_LAYERS = {
    "mlp_extractor.policy_net.0": ("dz1p", "x"), "mlp_extractor.policy_net.2": ("dz2p", "h1p"), "action_net": ("dlogits", "h2p"),
    "mlp_extractor.value_net.0": ("dz1v", "x"), "mlp_extractor.value_net.2": ("dz2v", "h1v"), "value_net": ("dvalue", "h2v"),
}


def ppo_reference(state_dict, obs_int8, actions, old_log_probs, advantages, returns, clip_range, ent_coef, vf_coef,
                  normalize, dtype=np.float64, clip_range_vf=None, old_values=None):
    """SB3's PPO.train loss of one minibatch (clip_range_vf with old_values [B]: value clipping) and its gradient, derived by
    hand, in numpy at precision dtype: obs_int8 [B, D], actions, old_log_probs, advantages, returns [B].
    Returns (grads {state-dict key: array in nn.Linear layout}, stats [8]: STAT_NAMES then two zeros).  The
    min passes the advantage where its unclipped branch is the smaller or the ratio lies inside the clip
    interval, which is autograd's result off the clip edges."""
    t = ppo_terms(state_dict, obs_int8, actions, old_log_probs, advantages, returns, clip_range, ent_coef, vf_coef,
                  normalize, dtype, clip_range_vf, old_values)
    grads = {}
    for layer, (dz, inp) in PPO_LAYERS.items():
        d = t[dz] if t[dz].ndim == 2 else t[dz][:, None]
        grads[layer + ".weight"] = d.T @ t[inp]
        grads[layer + ".bias"] = d.sum(axis=0, dtype=dtype)
    m = lambda v: v.mean(dtype=dtype)  # noqa: E731
    pol, val, ent = m(t["t_policy"]), m(t["t_value"]), m(t["t_entropy"])
    stats = np.array([pol + dtype(ent_coef) * ent + dtype(vf_coef) * val, pol, val, ent,
                      m((t["ratio"] - 1) - t["log_ratio"]), m(t["clipped"]), 0, 0], dtype=dtype)
    return grads, stats


def policy_adam_reference(params, grads, m, v, step, lr, betas, eps, max_grad_norm, dtype=np.float64):
    """torch.nn.utils.clip_grad_norm_ followed by one torch.optim.Adam step (weight_decay = 0, amsgrad = False),
    which is what pgtg_ppo_step computes, in numpy at precision dtype.  params, grads, m (exp_avg), v (exp_avg_sq):
    {key: array or tensor} over the same keys; step counts from 1; max_grad_norm = inf: no clip.  Returns
    (params, m, v, total_norm): new dicts, the inputs are not written.
        total = sqrt(sum g^2)      g <- min(1, max_grad_norm / (total + 1e-6)) g
        m <- m + (1 - beta1) (g - m)      v <- beta2 v + (1 - beta2) g^2
        p <- p - (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
    The bias corrections are Python floats (double), as in torch."""
    if int(step) < 1:
        raise ValueError("step counts from 1")
    b1, b2 = (float(b) for b in betas)
    cast = lambda d: {k: np.asarray(_host(x), dtype=dtype) for k, x in d.items()}  # noqa: E731
    p, g, m, v = cast(params), cast(grads), cast(m), cast(v)
    total = np.sqrt(sum((x * x).sum(dtype=dtype) for x in g.values()), dtype=dtype)
    coef = min(dtype(1), dtype(max_grad_norm) / (total + dtype(1e-6)))
    step_size = dtype(float(lr) / (1.0 - b1 ** int(step)))
    bc2_sqrt = dtype(math.sqrt(1.0 - b2 ** int(step)))
    for k in p:
        gk = coef * g[k]
        m[k] = m[k] + dtype(1.0 - b1) * (gk - m[k])
        v[k] = dtype(b2) * v[k] + dtype(1.0 - b2) * gk * gk
        p[k] = p[k] - step_size * m[k] / (np.sqrt(v[k]) / bc2_sqrt + dtype(eps))
    return p, m, v, total


class _MlpExtractor(nn.Module):
    def __init__(self, obs_dim: int):
        super().__init__()
        self.policy_net = nn.Sequential(nn.Linear(obs_dim, HIDDEN), nn.Tanh(), nn.Linear(HIDDEN, HIDDEN), nn.Tanh())
        self.value_net = nn.Sequential(nn.Linear(obs_dim, HIDDEN), nn.Tanh(), nn.Linear(HIDDEN, HIDDEN), nn.Tanh())


class MlpPolicyReference(nn.Module):
    """SB3's ActorCriticPolicy for a flat observation and Discrete(9), restated: the same parameter names
    (mlp_extractor.policy_net.{0,2}, mlp_extractor.value_net.{0,2}, action_net, value_net), the same
    orthogonal initialisation (gain sqrt 2 for the towers, 0.01 for action_net, 1 for value_net, zero
    biases).  forward(obs_float [N, D]) -> (logits [N, 9], value [N])."""

    def __init__(self, obs_dim: int):
        super().__init__()
        self.obs_dim = int(obs_dim)
        self.mlp_extractor = _MlpExtractor(self.obs_dim)
        self.action_net = nn.Linear(HIDDEN, N_ACTIONS)
        self.value_net = nn.Linear(HIDDEN, 1)
        for module, gain in ((self.mlp_extractor, math.sqrt(2)), (self.action_net, 0.01), (self.value_net, 1.0)):
            for m in module.modules():
                if isinstance(m, nn.Linear):
                    nn.init.orthogonal_(m.weight, gain=gain)
                    m.bias.data.fill_(0.0)

    def forward(self, obs_float):
        logits = self.action_net(self.mlp_extractor.policy_net(obs_float))
        value = self.value_net(self.mlp_extractor.value_net(obs_float))
        return logits, value[:, 0]


def check_target_kl(target_kl):
    """target_kl as a float, or None; ValueError for a negative or non-finite one."""
    if target_kl is None:
        return None
    k = float(target_kl)
    if not (math.isfinite(k) and k >= 0.0):
        raise ValueError("target_kl must be finite and at least 0 (None: no early stop)")
    return k


def _ppo_extra(device, stop_at=None, ordinal=0, clip_range_vf=None, old_values=None, target_kl=None):
    """The PgtgPpoExtra of a gated or value-clipped call (include/pgtg.h), or None where nothing is asked for."""
    if stop_at is None and clip_range_vf is None and target_kl is None:
        return None
    x = _abi.PgtgPpoExtra()
    if stop_at is not None:
        if stop_at.dtype != torch.int32 or stop_at.numel() != 1 or stop_at.device != device:
            raise ValueError(f"stop_at: an int32 tensor of one word on {device}")
        if int(ordinal) < 1:
            raise ValueError("ordinal counts from 1 where stop_at is given")
        x.stop_at, x.ordinal = stop_at.data_ptr(), int(ordinal)
    if clip_range_vf is not None:
        x.flags |= _abi.PGTG_PPO_CLIP_VF
        x.clip_range_vf, x.old_values = clip_range_vf, old_values.data_ptr()
    if target_kl is not None:
        if stop_at is None:
            raise ValueError("target_kl needs stop_at")
        x.flags |= _abi.PGTG_PPO_TARGET_KL
        x.target_kl = target_kl
    return x


class DevicePolicy:
    """The fused acting pass on `env`'s device and stream (module text).  obs_dim defaults to the env's flat
    observation length; seed is the seed of the policy's own uniform draws."""

    def __init__(self, env, obs_dim: int | None = None, seed: int = 0):
        if obs_dim is None:
            from .flat import flat_dim
            obs_dim = flat_dim(env.spec)
        self.env = env
        self.obs_dim = D = int(obs_dim)
        if not 1 <= D <= _abi.PGTG_POLICY_MAX_OBS_DIM:
            raise ValueError(f"obs_dim must be in [1, {_abi.PGTG_POLICY_MAX_OBS_DIM}]")
        self.device = env.device
        self.seed = int(seed)
        self.counter = 0       # draws made so far: one per sampling act() that drew its own uniforms
        self.env_offset = 0    # global index of env 0 (a sharded run draws what one GPU would)
        nbytes = C.c_uint64()
        rc = env._lib.pgtg_policy_packed_bytes(D, C.byref(nbytes))
        if rc != _abi.PGTG_OK:
            raise ValueError(f"pgtg_policy_packed_bytes({D}) failed ({rc})")
        self._packed = torch.zeros(nbytes.value // 4, dtype=torch.float32, device=self.device)
        self._loaded = False
        self._grads = None      # ppo_grad's own gradient tensors
        self._ppo_ws = None     # the largest workspace a ppo_grad has needed so far
        self._ppo_keep = None   # what the last ppo_grad launch reads

    def _fail(self, rc: int) -> None:
        from .vector import _check
        _check(rc, self.env._h)

    def load_state_dict(self, sd) -> None:
        """Hand a state dict of MlpPolicyReference or of SB3's MlpPolicy (tensors on any device, any
        strides) to the kernel: float32 copies on the env's device where needed, then one launch of
        k_policy_pack on the env's stream.  ValueError names a missing or misshapen key."""
        shapes = weight_shapes(self.obs_dim)
        raw, keep = _abi.PgtgPolicyWeights(obs_dim=self.obs_dim), []
        for field, (key, _) in WEIGHT_KEYS.items():
            if key not in sd:
                raise ValueError(f"state dict has no {key!r}")
            t = torch.as_tensor(sd[key])
            if tuple(t.shape) != shapes[key]:
                raise ValueError(f"{key!r} has shape {tuple(t.shape)}, expected {shapes[key]}")
            t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
            keep.append(t)
            setattr(raw, field, t.data_ptr())
        self.env._bind_stream()
        rc = self.env._lib.pgtg_policy_pack(self.env._h, C.byref(raw), C.c_void_p(self._packed.data_ptr()))
        if rc != _abi.PGTG_OK:
            self._fail(rc)
        self._loaded = True

    def _out(self, t, n: int, dtype, name: str):
        if t is None:
            return torch.empty(n, dtype=dtype, device=self.device)
        if t.dtype != dtype or t.numel() != n or not t.is_contiguous() or t.device != self.device:
            raise ValueError(f"{name}: a contiguous {dtype} tensor of {n} values on {self.device}")
        return t

    def _launch(self, obs, mode, actions, values, log_probs, uniforms, counter) -> None:
        if not self._loaded:
            raise RuntimeError("load_state_dict() first")
        if obs.dtype != torch.int8 or obs.dim() != 2 or obs.shape[1] != self.obs_dim or not obs.is_contiguous() \
                or obs.device != self.device:
            raise ValueError(f"obs: a contiguous int8 [N, {self.obs_dim}] tensor on {self.device}")
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        a = _abi.PgtgPolicy(n=obs.shape[0], obs_dim=self.obs_dim, obs=p(obs), packed=p(self._packed), mode=mode,
                            seed=self.seed & ((1 << 64) - 1), counter=counter, env_offset=self.env_offset,
                            uniforms=p(uniforms), actions=p(actions), values=p(values), log_probs=p(log_probs))
        self.env._bind_stream()
        rc = self.env._lib.pgtg_policy(self.env._h, C.byref(a))
        if rc != _abi.PGTG_OK:
            self._fail(rc)

    def act(self, obs, actions=None, values=None, log_probs=None, deterministic: bool = False, uniforms=None):
        """One launch of k_policy on obs (int8 [N, D] on the device): the sampled action (deterministic:
        the argmax), the value and the action's log-probability of every env, written into the given [N]
        rows (uint8, float32, float32) or into fresh tensors.  uniforms: float32 [N] in [0, 1) to sample
        with; None draws policy_uniform(seed, counter, env_offset + e) and advances the counter."""
        n = obs.shape[0]
        actions = self._out(actions, n, torch.uint8, "actions")
        values = self._out(values, n, torch.float32, "values")
        log_probs = self._out(log_probs, n, torch.float32, "log_probs")
        if uniforms is not None:
            uniforms = self._out(uniforms, n, torch.float32, "uniforms")
        self._launch(obs, ARGMAX if deterministic else SAMPLE, actions, values, log_probs, uniforms, self.counter)
        if not deterministic and uniforms is None:
            self.counter += 1
        return actions, values, log_probs

    def value(self, obs, out=None):
        """V(obs) alone (the vf tower; one launch of k_policy in its value-only mode) into out or a fresh
        float32 [N] tensor."""
        out = self._out(out, obs.shape[0], torch.float32, "out")
        self._launch(obs, VALUE_ONLY, None, out, None, None, 0)
        return out

    def ppo_grad(self, rollout, indices, grads=None, clip_range: float = 0.2, ent_coef: float = 0.0,
                 vf_coef: float = 0.5, normalize_advantage: bool = True, adv_stats=None, clip_range_vf=None,
                 stats_out=None, target_kl=None, stop_at=None, ordinal: int = 0):
        """One PPO minibatch on the samples `indices` (int64 [B] device tensor of flat sample indices,
        rollout.sample_index's order; repeats allowed) of a finished int8 rollout: SB3's loss and its gradient
        with respect to the twelve tensors, by pgtg_ppo_grad (three launches; the [B, D] batch is never
        built).  Returns (grads, stats): grads {state-dict key: float32 device tensor}, overwritten -- the
        policy's own set, allocated once, or the dict given, e.g. a module's .grad tensors; stats the device
        tensor of eight floats (STAT_NAMES, two zeros).  The advantages' mean and 1 / (std + 1e-8) are two
        small torch reductions on the env's stream (skipped for B <= 1, as in SB3); nothing synchronises.
        An index outside the rollout is skipped by the kernel and counted (env.error_count()); in the mean and
        the std of the advantages it stands as an advantage of 0, so that no mask has to reach the host.
        adv_stats: a float32 [2] device tensor {mean, 1 / (std + 1e-8)} (self.adv_stats) to normalise with in
        place of the torch reductions; the call then launches no torch kernel (the stats tensor is allocated
        without a fill: k_ppo_reduce writes all eight).
        clip_range_vf: SB3's value clipping against rollout.values (None: none, today's bits).  stats_out: a
        contiguous float32 [8] device tensor (a row of an update's [M, 8] buffer) to write the statistics into
        in place of a fresh tensor.  stop_at (int32 device word) with ordinal m = 1, 2, ...: the gate of an
        update with target_kl (include/pgtg.h PgtgPpoExtra): the launches do nothing once stop_at holds a value
        below m, and with target_kl given this minibatch stores stop_at = m when its approx_kl exceeds
        1.5 * target_kl and nothing has stopped the update yet.  ValueError for a negative or non-finite
        clip_range_vf or target_kl, with nothing launched."""
        if not self._loaded:
            raise ValueError("load_state_dict() first")
        clip_range_vf, target_kl = check_clip_range_vf(clip_range_vf), check_target_kl(target_kl)
        ro = rollout
        if ro.env is not self.env or ro.obs_dim != self.obs_dim:
            raise ValueError("the rollout is of another env or obs_dim")
        if ro._dtype_code != 1:
            raise ValueError("ppo_grad reads int8 rows: build the rollout with obs_dtype=torch.int8")
        if not ro._finished:
            raise ValueError("the rollout is not finished: collect() or finish() first")
        idx = torch.as_tensor(indices, device=self.device).to(torch.int64).reshape(-1).contiguous()
        B, D, T, N = idx.numel(), self.obs_dim, ro.n_steps, ro.num_envs
        shapes = weight_shapes(D)
        if grads is None:
            if self._grads is None:
                self._grads = {k: torch.zeros(s, dtype=torch.float32, device=self.device) for k, s in shapes.items()}
            grads = self._grads
        raw = _abi.PgtgPpoGrads()
        for field, (key, _) in WEIGHT_KEYS.items():
            g = grads.get(key)
            if g is None or g.dtype != torch.float32 or tuple(g.shape) != shapes[key] or not g.is_contiguous() \
                    or g.device != self.device:
                raise ValueError(f"grads[{key!r}]: a contiguous float32 tensor of shape {shapes[key]} on {self.device}")
            setattr(raw, field, g.data_ptr())
        if adv_stats is not None:
            adv_stats = self._out(adv_stats, 2, torch.float32, "adv_stats")
        extra = _ppo_extra(self.device, stop_at, ordinal, clip_range_vf, ro.values, target_kl)
        if stats_out is not None:
            stats = self._out(stats_out, 8, torch.float32, "stats_out")
        elif adv_stats is not None and B > 0:
            stats = torch.empty(8, dtype=torch.float32, device=self.device)
        else:
            stats = torch.zeros(8, dtype=torch.float32, device=self.device)
        if B == 0:
            return grads, stats
        nbytes = C.c_uint64()
        rc = self.env._lib.pgtg_ppo_workspace_bytes(D, B, C.byref(nbytes))
        if rc != _abi.PGTG_OK:
            raise ValueError(f"pgtg_ppo_workspace_bytes({D}, {B}) failed ({rc})")
        ws = self._ppo_ws  # (one buffer, grown to the largest batch seen: its contents do not matter)
        if ws is None or ws.numel() * 4 < nbytes.value:
            ws = self._ppo_ws = torch.empty(max(4, nbytes.value // 4), dtype=torch.float32, device=self.device)
        if adv_stats is None and normalize_advantage and B > 1:
            e, t = idx // T, idx % T
            inside = (idx >= 0) & (idx < T * N)
            adv = ro.advantages[t.clamp(0, T - 1), e.clamp(0, N - 1)] * inside  # (a skipped sample counts as 0)
            adv_stats = torch.stack((adv.mean(), 1.0 / (adv.std() + 1e-8)))
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        a = _abi.PgtgPpoGrad(batch=B, obs_dim=D, steps=T, n=N, obs_pitch=ro.obs.stride(0), obs=p(ro.obs),
                             indices=p(idx), actions=p(ro.actions), log_probs=p(ro.log_probs),
                             advantages=p(ro.advantages), returns=p(ro.returns), packed=p(self._packed),
                             adv_stats=p(adv_stats), clip_range=float(clip_range), ent_coef=float(ent_coef),
                             vf_coef=float(vf_coef), workspace=p(ws), grads=raw, stats=p(stats))
        self._ppo_keep = (idx, adv_stats, stats, grads, stop_at)
        self.env._bind_stream()
        if extra is None:
            rc = self.env._lib.pgtg_ppo_grad(self.env._h, C.byref(a))
        else:
            rc = self.env._lib.pgtg_ppo_grad_ex(self.env._h, C.byref(a), C.byref(extra))
        if rc != _abi.PGTG_OK:
            self._fail(rc)
        return grads, stats

    def adv_stats(self, rollout, indices, out=None, stop_at=None, ordinal: int = 0):
        """{mean, 1 / (std + 1e-8)} of the advantages of the samples `indices` (as ppo_grad takes them; at least
        two) into out or a fresh float32 [2] device tensor: one launch of k_ppo_adv_stats on the env's stream
        (include/pgtg.h pgtg_ppo_adv_stats), for ppo_grad's adv_stats.  The unbiased std; an index outside the
        rollout stands as an advantage of 0, as in ppo_grad's own reductions.  stop_at, ordinal: ppo_grad's gate."""
        ro = rollout
        if ro.env is not self.env:
            raise ValueError("the rollout is of another env")
        if not ro._finished:
            raise ValueError("the rollout is not finished: collect() or finish() first")
        idx = torch.as_tensor(indices, device=self.device).to(torch.int64).reshape(-1).contiguous()
        if idx.numel() < 2:
            raise ValueError("adv_stats needs at least two samples (SB3 does not normalise a batch of one)")
        out = self._out(out, 2, torch.float32, "out")
        extra = _ppo_extra(self.device, stop_at, ordinal)
        self._adv_keep = (idx, out, stop_at)
        self.env._bind_stream()
        args = (self.env._h, C.c_void_p(ro.advantages.data_ptr()), C.c_void_p(idx.data_ptr()), idx.numel(), ro.n_steps,
                ro.num_envs, C.c_void_p(out.data_ptr()))
        if extra is None:
            rc = self.env._lib.pgtg_ppo_adv_stats(*args)
        else:
            rc = self.env._lib.pgtg_ppo_adv_stats_ex(*args, C.byref(extra))
        if rc != _abi.PGTG_OK:
            self._fail(rc)
        return out


class DeviceAdam:
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam (weight_decay 0, no amsgrad) + the repack for k_policy
    as one call of pgtg_ppo_step (k_ppo_gnorm, k_ppo_adam: two launches on the env's stream, no torch kernel, no
    host synchronisation).  module: an MlpPolicyReference on the policy's device whose parameters are contiguous
    float32; they are updated in place, so module.state_dict() stays the truth, and the policy's packed buffer
    is rewritten by the same launch (no policy.load_state_dict follows).  The moments and the step count live
    here; `lr` is read at every step (a schedule is an assignment); `last_grad_norm` is the device tensor [1] of
    the last step's total norm before clipping.  state_dict() / load_state_dict() speak torch.optim.Adam's format
    over module.parameters()' order, so a run can move between the two optimisers."""

    def __init__(self, policy: DevicePolicy, module, lr: float = 3e-4, betas=(0.9, 0.999), eps: float = 1e-5):
        self.policy, self.module = policy, module
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.step_count = 0
        named = dict(module.named_parameters())
        shapes = weight_shapes(policy.obs_dim)
        for key, shape in shapes.items():
            p = named.get(key)
            if p is None:
                raise ValueError(f"the module has no parameter {key!r}")
            if p.dtype != torch.float32 or tuple(p.shape) != shape or not p.is_contiguous() or p.device != policy.device:
                raise ValueError(f"{key!r}: a contiguous float32 parameter of shape {shape} on {policy.device}")
        self._keys = [k for k in named if k in shapes]  # module.parameters()' order
        if len(self._keys) != len(named):
            raise ValueError(f"the module has parameters beyond MlpPolicy's twelve: {sorted(set(named) - set(shapes))}")
        self._params = {k: named[k] for k in self._keys}
        self.exp_avg = {k: torch.zeros_like(p, requires_grad=False) for k, p in self._params.items()}
        self.exp_avg_sq = {k: torch.zeros_like(p, requires_grad=False) for k, p in self._params.items()}
        self.last_grad_norm = torch.zeros(1, dtype=torch.float32, device=policy.device)
        nbytes = C.c_uint64()
        rc = policy.env._lib.pgtg_ppo_step_workspace_bytes(policy.obs_dim, C.byref(nbytes))
        if rc != _abi.PGTG_OK:
            raise ValueError(f"pgtg_ppo_step_workspace_bytes({policy.obs_dim}) failed ({rc})")
        self._ws = torch.empty(nbytes.value // 4, dtype=torch.float32, device=policy.device)
        self._raw = _abi.PgtgPpoStep(obs_dim=policy.obs_dim, packed=policy._packed.data_ptr(), workspace=self._ws.data_ptr(),
                                     grad_norm=self.last_grad_norm.data_ptr())
        for field, (key, _) in WEIGHT_KEYS.items():
            setattr(self._raw.params, field, self._params[key].data_ptr())
            setattr(self._raw.exp_avg, field, self.exp_avg[key].data_ptr())
            setattr(self._raw.exp_avg_sq, field, self.exp_avg_sq[key].data_ptr())

    def step(self, grads=None, max_grad_norm: float | None = 0.5, stop_at=None, ordinal: int = 0) -> None:
        """One optimiser step from grads {state-dict key: contiguous float32 device tensor} (default: the
        module's .grad tensors; they are read, not written): the global norm over all twelve, the clip to
        max_grad_norm (None or inf: none), Adam, and the policy's packed buffer rewritten.  stop_at, ordinal:
        ppo_grad's gate; the step of ordinal m does nothing once stop_at holds a value up to m.  step_count
        counts the call either way: Rollout.update sets it right after its one read of stop_at."""
        pol, shapes = self.policy, weight_shapes(self.policy.obs_dim)
        raw = self._raw
        for field, (key, _) in WEIGHT_KEYS.items():
            p = self._params[key]
            g = p.grad if grads is None else grads.get(key)
            if g is None or g.dtype != torch.float32 or tuple(g.shape) != shapes[key] or not g.is_contiguous() \
                    or g.device != pol.device:
                raise ValueError(f"gradient of {key!r}: a contiguous float32 tensor of shape {shapes[key]} on {pol.device}")
            if p.data_ptr() != getattr(raw.params, field):
                raise ValueError(f"{key!r}: the module's parameter storage was replaced; build a new DeviceAdam")
            setattr(raw.grads, field, g.data_ptr())
        raw.step = self.step_count + 1
        raw.lr, (raw.beta1, raw.beta2), raw.eps = float(self.lr), self.betas, self.eps
        raw.max_grad_norm = math.inf if max_grad_norm is None else float(max_grad_norm)
        extra = _ppo_extra(pol.device, stop_at, ordinal)
        self._keep = (grads, stop_at)
        pol.env._bind_stream()
        if extra is None:
            rc = pol.env._lib.pgtg_ppo_step(pol.env._h, C.byref(raw))
        else:
            rc = pol.env._lib.pgtg_ppo_step_ex(pol.env._h, C.byref(raw), C.byref(extra))
        if rc != _abi.PGTG_OK:
            pol._fail(rc)
        self.step_count += 1
        pol._loaded = True

    def zero_grad(self, set_to_none: bool = False) -> None:
        """Nothing to do for pgtg_ppo_grad, which overwrites; here for loops written for torch.optim."""
        for p in self._params.values():
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def state_dict(self) -> dict:
        """torch.optim.Adam's state dict over module.parameters()' order (clones; `step` a host int)."""
        state = {}
        if self.step_count:
            state = {i: {"step": int(self.step_count), "exp_avg": self.exp_avg[k].clone(), "exp_avg_sq": self.exp_avg_sq[k].clone()}
                     for i, k in enumerate(self._keys)}
        group = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                     capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                     params=list(range(len(self._keys))))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd) -> None:
        """Take a torch.optim.Adam (or DeviceAdam) state dict over the same parameters: lr, betas, eps, the
        moments (copied into this optimiser's own tensors) and the step count (an int or a tensor; one count
        for all parameters).  ValueError for another shape of state, weight decay or amsgrad."""
        groups = sd["param_groups"]
        if len(groups) != 1 or list(groups[0]["params"]) != list(range(len(self._keys))):
            raise ValueError(f"one parameter group over {len(self._keys)} parameters is expected")
        g = groups[0]
        if g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("weight_decay, amsgrad and maximize are not supported")
        state = sd["state"]
        if state and sorted(state) != list(range(len(self._keys))):
            raise ValueError("the state must hold every parameter or none")
        steps = {int(float(s["step"])) for s in state.values()}
        if len(steps) > 1:
            raise ValueError(f"one step count for all parameters is expected, got {sorted(steps)}")
        for i, k in enumerate(self._keys):
            for mine, name in ((self.exp_avg, "exp_avg"), (self.exp_avg_sq, "exp_avg_sq")):
                if state:
                    t = torch.as_tensor(state[i][name])
                    if tuple(t.shape) != tuple(mine[k].shape):
                        raise ValueError(f"{name} of parameter {i} ({k}) has shape {tuple(t.shape)}")
                    mine[k].copy_(t)
                else:
                    mine[k].zero_()
        self.lr, self.betas, self.eps = float(g["lr"]), (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
        self.step_count = steps.pop() if steps else 0
