"""Inputs and references shared by test_ppo_train_cpu.py and test_gpu_ppo_train.py, on top of ppo_cases.py: old
values that put both sides of SB3's value clip into every set, torch autograd of SB3's clipped expression, and
the accumulated magnitudes and E_torch of ppo_cases' tolerance re-measured for the clipped loss."""
from __future__ import annotations

import functools

import numpy as np
import torch

import ppo_cases as ppc
from pgtg_amd import policy as P

CLIP_VF = 0.3
BS = (1, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def old_values(D: int, clip_vf: float = CLIP_VF):
    """[T, N] float32 old values for ppc.case(D), redrawn until the float64 reference alone has no |value - old|
    within 1e-3 of clip_vf and a clipped share in [0.1, 0.9] (ppo_cases' conditioning of the ratio)."""
    c = ppc.case(D)
    v = P.policy_reference(c.sd, c.obs.reshape(ppc.TOTAL, D), mode=P.VALUE_ONLY).values.reshape(ppc.T, ppc.N)
    for seed in range(200):
        rng = np.random.default_rng(31 * D + seed)
        old = (v + clip_vf * 1.5 * rng.standard_normal(v.shape)).astype(np.float32)
        dd = np.abs(v - old.astype(np.float64))
        if np.abs(dd - clip_vf).min() > 1e-3 and 0.1 <= float((dd > clip_vf).mean()) <= 0.9:
            return old
    raise AssertionError("no conditioned old values found")


def batch(D: int, B: int):
    """(ppc's batch tuple, old values [B]) of ppc.case(D).indices(B)."""
    c = ppc.case(D)
    idx = c.indices(B)
    return c.batch(idx), old_values(D)[idx % ppc.T, idx // ppc.T]


def torch_clipped(sd, obs_int8, actions, old, adv, ret, ov, clip_vf, ent, norm, dtype):
    """(grads {key: numpy}, stats [6]) of torch-CPU autograd through MlpPolicyReference with SB3's value clipping:
    values_pred = old_values + clamp(values - old_values, -c, c)."""
    m = P.MlpPolicyReference(obs_int8.shape[1]).to(dtype)
    m.load_state_dict({k: torch.as_tensor(v).to(dtype) for k, v in sd.items()})
    t = lambda x: torch.as_tensor(x).to(dtype)  # noqa: E731
    ovt = t(ov)

    def clipped(x):
        logits, values = m(x)
        return logits, ovt + torch.clamp(values - ovt, -clip_vf, clip_vf)

    loss, stats = ppc.torch_ppo(clipped, t(obs_int8), torch.as_tensor(actions), t(old), t(adv), t(ret), ppc.CLIP, ent, ppc.VF,
                                norm)
    loss.backward()
    return {k: p.grad.numpy() for k, p in m.named_parameters()}, stats.numpy()


def magnitudes(sd, b, ov, clip_vf, ent, norm):
    """ppc.magnitudes for the clipped loss: ({key: array}, stats [6]), float64."""
    t = P.ppo_terms(sd, *b, ppc.CLIP, ent, ppc.VF, norm, clip_range_vf=clip_vf, old_values=ov)
    g = {}
    for layer, (dz, inp) in P.PPO_LAYERS.items():
        d = np.abs(t[dz] if t[dz].ndim == 2 else t[dz][:, None])
        g[layer + ".weight"] = d.T @ np.abs(t[inp])
        g[layer + ".bias"] = d.sum(axis=0)
    pol, val = np.abs(t["t_policy"]).mean(), t["t_value"].mean()
    ent_m = np.abs(t["p"] * t["lsm"]).sum(axis=1).mean()
    kl = (np.abs(t["ratio"] - 1) + np.abs(t["log_ratio"])).mean()
    return g, np.array([pol + ent * ent_m + ppc.VF * val, pol, val, ent_m, kl, t["clipped"].mean()])


@functools.lru_cache(maxsize=None)
def reference(D: int, B: int, norm: bool, ent: float):
    """(float64 grads, stats, magnitudes of both) of the clipped loss on batch(D, B)."""
    c = ppc.case(D)
    b, ov = batch(D, B)
    g, s = P.ppo_reference(c.sd, *b, ppc.CLIP, ent, ppc.VF, norm, clip_range_vf=CLIP_VF, old_values=ov)
    return (g, s) + magnitudes(c.sd, b, ov, CLIP_VF, ent, norm)


@functools.lru_cache(maxsize=None)
def e_torch(D: int) -> dict:
    """Per tensor and statistic: torch-CPU float32 autograd's largest deviation (ppc.deviations) from the float64
    reference of the clipped loss over BS x ppc.CONFIGS."""
    c = ppc.case(D)
    worst = {}
    for B in BS:
        b, ov = batch(D, B)
        for norm, ent in ppc.CONFIGS:
            tg, ts = torch_clipped(c.sd, *b, ov, CLIP_VF, ent, norm, torch.float32)
            for k, v in ppc.deviations(tg, ts, *reference(D, B, norm, ent)).items():
                worst[k] = max(worst.get(k, 0.0), v)
    return worst
