"""Inputs, references and the measured tolerance shared by test_ppo_cpu.py and test_gpu_ppo.py, built like
policy_cases.py.

One input set per D: the "scaled" weights of policy_cases, a made-up finished rollout of T = 3 steps of
N = 96 envs (int8 rows from policy_cases' row generator; 96 D is a multiple of 16 for every D, so the GPU
tests pad the row pitch themselves: `pitch(D)`), uniform actions, normal advantages and returns, and old
log-probabilities that are the float64 reference's under a perturbed copy of the weights, so that the ratios spread around 1.  The set is
redrawn until the float64 reference alone satisfies: no ratio within 1e-3 of 1 +- clip_range, a clip fraction
in [0.1, 0.9] and no two logits of a sample closer than 1e-6.

Tolerance.  Truth is `ppo_reference` at float64.  A quantity's deviation is measured in units of its
accumulated magnitude, the float64 sum over the samples of the absolute per-sample contributions:
    weight gradient  |dZ|^T |input|  (one abs-matmul),  bias gradient  sum |dZ|,
    policy / value / entropy loss  mean |term|  (entropy: mean sum_c |p_c log p_c|),
    approx_kl  mean (|ratio - 1| + |log ratio|)  (the two parts the sample's term is the difference of),
    clip fraction  its own value,  loss  the three magnitudes combined with the coefficients;
a quantity whose magnitude is zero must be exactly zero.  E_torch is, per tensor and per statistic, the
largest such deviation of torch-CPU float32 autograd through MlpPolicyReference (what SB3 would compute)
over the set's batches (every B of the set with and without normalisation, ent_coef 0 and 0.01), computed
once per set as policy_cases does; the kernel may deviate by MARGIN = 4 of it ("another summation order over
the same float32 products").
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import policy_cases as pc
from pgtg_amd import policy as P

T, N = 3, 96
TOTAL = T * N
CLIP, VF = 0.2, 0.5
BS = (1, 63, 64, 65, 257)
FULL_DS = (29, 1239)
EDGE_DS = (1, 17, P.K_CHUNK + 1)
# batches long enough for k_ppo_dw1 to take several 64-sample stages per segment, the last segment short
# (pgtg_ppo.h ppo_plan at D = 1239: B = 3333 gives 53 blocks in 27 segments of 2 with a last one of 1 and a last
# block of 5 samples; B = 7000 gives 110 blocks in 37 segments of 3 with a last one of 2); indices repeat past T * N
BIG_D, BIG_BS = 1239, (3333, 7000)
SHAPES = [(b, d) for d in FULL_DS for b in BS] + [(65, d) for d in EDGE_DS] + [(b, BIG_D) for b in BIG_BS]
CONFIGS = [(norm, ent) for norm in (True, False) for ent in (0.0, 0.01)]
MARGIN = pc.MARGIN
KEYS = [key for key, _ in P.WEIGHT_KEYS.values()]


def pitch(D: int) -> int:
    """Bytes from obs[t] to obs[t + 1] in the GPU tests' storage: N * D rounded up to 16 as a Rollout's is,
    and one more 16 so that the rows are not contiguous."""
    return (N * D + 15) // 16 * 16 + 16


def batches(D: int):
    return (BS if D in FULL_DS else (65,)) + (BIG_BS if D == BIG_D else ())


def torch_ppo(module, obs, actions, old_log_probs, advantages, returns, clip_range, ent_coef, vf_coef, normalize):
    """SB3's PPO.train loss of one minibatch in torch, at the module's dtype and device.  Returns (loss,
    stats [6] detached: P.STAT_NAMES)."""
    logits, values = module(obs)
    lsm = torch.log_softmax(logits, dim=1)
    log_prob = lsm.gather(1, actions.to(torch.int64)[:, None])[:, 0]
    entropy = -(lsm.exp() * lsm).sum(dim=1)
    adv = advantages
    if normalize and len(adv) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(log_prob - old_log_probs)
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    value_loss = torch.nn.functional.mse_loss(returns, values)
    entropy_loss = -entropy.mean()
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    with torch.no_grad():
        lr = log_prob - old_log_probs
        kl = ((torch.exp(lr) - 1) - lr).mean()
        cf = (torch.abs(ratio - 1) > clip_range).to(ratio.dtype).mean()
    return loss, torch.stack([loss.detach(), policy_loss.detach(), value_loss.detach(), entropy_loss.detach(), kl, cf])


def torch_grads(sd, obs_int8, actions, old, adv, ret, clip_range, ent_coef, vf_coef, normalize, dtype=torch.float32,
                device="cpu"):
    """(grads {key: numpy}, stats numpy [6]) of torch autograd through MlpPolicyReference."""
    m = P.MlpPolicyReference(obs_int8.shape[1]).to(dtype=dtype, device=device)
    m.load_state_dict({k: torch.as_tensor(v).to(dtype=dtype, device=device) for k, v in sd.items()})
    t = lambda x: torch.as_tensor(x).to(dtype=dtype, device=device)  # noqa: E731
    loss, stats = torch_ppo(m, t(obs_int8), torch.as_tensor(actions).to(device), t(old), t(adv), t(ret), clip_range,
                            ent_coef, vf_coef, normalize)
    loss.backward()
    return {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}, stats.cpu().numpy()


def magnitudes(sd, obs_int8, actions, old, adv, ret, clip_range, ent_coef, vf_coef, normalize):
    """The accumulated magnitudes of the module text: ({key: array}, stats [6]), float64."""
    t = P.ppo_terms(sd, obs_int8, actions, old, adv, ret, clip_range, ent_coef, vf_coef, normalize)
    g = {}
    for layer, (dz, inp) in P.PPO_LAYERS.items():
        d = np.abs(t[dz] if t[dz].ndim == 2 else t[dz][:, None])
        g[layer + ".weight"] = d.T @ np.abs(t[inp])
        g[layer + ".bias"] = d.sum(axis=0)
    pol, val = np.abs(t["t_policy"]).mean(), t["t_value"].mean()
    ent = np.abs(t["p"] * t["lsm"]).sum(axis=1).mean()
    kl = (np.abs(t["ratio"] - 1) + np.abs(t["log_ratio"])).mean()
    return g, np.array([pol + ent_coef * ent + vf_coef * val, pol, val, ent, kl, t["clipped"].mean()])


def _dev(got, want, mag):
    """Largest |got - want| / mag; where mag is zero the value must be exactly zero."""
    got, want, mag = (np.asarray(a, dtype=np.float64) for a in (got, want, mag))
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(mag > 0, err / mag, np.where(err == 0, 0.0, np.inf))
    return float(d.max())


def deviations(grads, stats, ref_grads, ref_stats, mag_grads, mag_stats) -> dict:
    d = {k: _dev(grads[k], ref_grads[k], mag_grads[k]) for k in KEYS}
    for i, name in enumerate(P.STAT_NAMES):
        d[name] = _dev(stats[i], ref_stats[i], mag_stats[i])
    return d


class Case:
    def __init__(self, D: int):
        self.D = D
        self.sd = pc.make_state_dict(D, "scaled")
        for seed in range(200):
            rng = np.random.default_rng(977 * D + seed)
            self.obs = pc._draw_rows(rng, np.arange(TOTAL), D).reshape(T, N, D)
            self.actions = rng.integers(0, P.N_ACTIONS, size=(T, N)).astype(np.uint8)
            g = torch.Generator().manual_seed(41 * D + seed)
            old_sd = {k: v + 0.05 * v.abs().mean() * torch.randn(v.shape, generator=g) for k, v in self.sd.items()}
            flat = self.obs.reshape(TOTAL, D)
            lsm = pc.log_softmax64(P.policy_reference(old_sd, flat, mode=P.ARGMAX).logits)
            self.old_log_probs = lsm[np.arange(TOTAL), self.actions.reshape(-1)].reshape(T, N).astype(np.float32)
            self.advantages = rng.standard_normal((T, N)).astype(np.float32)
            self.returns = rng.standard_normal((T, N)).astype(np.float32)
            self.conditions = self._conditions()
            if all(self.conditions.values()):
                break
        self.seed = seed
        self.perm = np.random.default_rng(5 + D).permutation(TOTAL).astype(np.int64)

    def _conditions(self) -> dict:
        flat = self.obs.reshape(TOTAL, self.D)
        lg = P.policy_reference(self.sd, flat, mode=P.ARGMAX).logits
        lsm = pc.log_softmax64(lg)
        ratio = np.exp(lsm[np.arange(TOTAL), self.actions.reshape(-1)] - self.old_log_probs.reshape(-1).astype(np.float64))
        edge = np.minimum(np.abs(ratio - (1 - CLIP)), np.abs(ratio - (1 + CLIP))).min()
        frac = float((np.abs(ratio - 1) > CLIP).mean())
        gaps = np.diff(np.sort(lg, axis=1), axis=1).min()
        return dict(off_the_edges=bool(edge > 1e-3), both_branches=bool(0.1 <= frac <= 0.9), no_ties=bool(gaps > 1e-6))

    def indices(self, B: int) -> np.ndarray:
        """B sample indices: the first B of a fixed permutation (past T * N they repeat)."""
        return self.perm[np.arange(B) % TOTAL].copy()

    def batch(self, idx):
        """(obs [B, D], actions, old_log_probs, advantages, returns [B]) of sample indices idx (s = env * T + step)."""
        e, t = np.asarray(idx) // T, np.asarray(idx) % T
        return self.obs[t, e], self.actions[t, e], self.old_log_probs[t, e], self.advantages[t, e], self.returns[t, e]

    @functools.lru_cache(maxsize=None)
    def reference(self, B: int, norm: bool, ent: float):
        """(float64 grads, stats, magnitudes of both) of the batch indices(B)."""
        b = self.batch(self.indices(B))
        g, s = P.ppo_reference(self.sd, *b, CLIP, ent, VF, norm)
        mg, ms = magnitudes(self.sd, *b, CLIP, ent, VF, norm)
        return g, s, mg, ms

    @functools.cached_property
    def e_torch(self) -> dict:
        """Per tensor and statistic: torch-CPU float32 autograd's largest deviation over the set's batches."""
        worst = {}
        for B in batches(self.D):
            for norm, ent in CONFIGS:
                g, s, mg, ms = self.reference(B, norm, ent)
                tg, ts = torch_grads(self.sd, *self.batch(self.indices(B)), CLIP, ent, VF, norm)
                for k, v in deviations(tg, ts, g, s, mg, ms).items():
                    worst[k] = max(worst.get(k, 0.0), v)
        return worst

    def check(self, grads, stats, ref, label="", e_torch=None) -> dict:
        """grads {key: array}, stats [>= 6] against ref = (grads, stats, magnitudes of both): every tensor and
        statistic within MARGIN x E_torch.  Prints the figures before asserting; returns them."""
        e = self.e_torch if e_torch is None else e_torch
        d = deviations(grads, stats, *ref)
        fig = {k: (d[k], e[k]) for k in d}
        print("ppo-tolerance", label, {k: f"{a:.2e}/{b:.2e}={a / b if b else float('nan'):.2f}" for k, (a, b) in fig.items()})
        bad = {k: v for k, v in fig.items() if not v[0] <= MARGIN * v[1]}
        assert not bad, (label, bad)
        return fig


@functools.lru_cache(maxsize=None)
def case(D: int) -> Case:
    return Case(D)
