"""Inputs, references and the measured tolerance shared by test_policy_cpu.py and test_gpu_policy.py.

One input set per (D, weights): `rows(D)` envs of made-up int8 rows and an MlpPolicyReference's weights.
A test at N envs uses the set's first N rows, so the float64 reference, the torch float32 forward and the
tolerance are computed once per set and never changed.

Tolerance (per set, per output kind): with the float64 policy_reference as the truth, E_torch is the
largest deviation of the torch-CPU float32 forward of MlpPolicyReference -- what SB3 itself would compute
-- per element, in units of the magnitude that output's last layer accumulates,
    value:     s = sum_k |wv[k] h2v[k]| + |bv|
    log_prob:  s = max_a (sum_k |wa[a][k] h2p[k]| + |ba[a]|)   (a log-probability involves every logit)
and the kernel may deviate by 4 E_torch in the same units: the margin for another summation order over
the same float32 products.  Rounding the weights once to bfloat16 must exceed it (test_policy_cpu.py).
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from pgtg_amd import policy as P

NS = (1, 63, 64, 65, 257, 1000)
KC = P.K_CHUNK
DS = (1, 3, 15, 16, 17, 29, 63, 64, 65, 1239, KC - 1, KC, KC + 1, 2 * KC + 1)
BIG_D = 4099
FULL_N_DS = (29, 1239)  # every N at these; every other D at N = 65
SHAPES = sorted({(65, d) for d in DS} | {(n, d) for n in NS for d in FULL_N_DS} | {(65, BIG_D)})
WEIGHTS = ("init", "scaled")
MARGIN = 4.0


def rows(D: int) -> int:
    return max(NS) if D in FULL_N_DS else 65


def _draw_rows(rng, idx, D):
    """Rows for the env indices idx: 0/1 bytes at density 0, 0.1, 0.5, 1 by env % 4; every third env has a
    few bytes of the whole int8 range, with -128 and 127 at positions 0 and D - 1 on every sixth."""
    dens = np.array([0.0, 0.1, 0.5, 1.0])[idx % 4]
    x = (rng.random((len(idx), D)) < dens[:, None]).astype(np.int8)
    for j, e in enumerate(idx):
        if e % 3 == 0:
            pos = rng.integers(0, D, size=3)
            x[j, pos] = rng.integers(-128, 128, size=3).astype(np.int8)
        if e % 6 == 0:
            x[j, 0], x[j, D - 1] = -128, 127
        elif e % 6 == 3:
            x[j, D - 1], x[j, 0] = -128, 127
    return x


def make_state_dict(D: int, weights: str, seed: int = 0) -> dict:
    """SB3's initialisation with small random biases in place of its zero ones (an all-zero row would
    otherwise tie every logit); "scaled": the same with larger biases, first layers x3 and the action head
    x150 (logits span about +-5, the towers saturate for some envs)."""
    torch.manual_seed(1000 + 7 * D + seed)
    sd = {k: v.detach().clone() for k, v in P.MlpPolicyReference(D).state_dict().items()}
    g = torch.Generator().manual_seed(5 + D + seed)
    for k in sd:
        if k.endswith("bias"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * (0.1 if weights == "scaled" else 0.05)
    if weights == "scaled":
        sd["mlp_extractor.policy_net.0.weight"] *= 3.0
        sd["mlp_extractor.value_net.0.weight"] *= 3.0
        sd["action_net.weight"] *= 150.0
    elif weights != "init":
        raise ValueError(weights)
    return sd


def _hidden64(sd, x):
    w = {f: np.asarray(sd[k].numpy(), dtype=np.float64) for f, (k, _) in P.WEIGHT_KEYS.items()}
    x = x.astype(np.float64)
    h2p = np.tanh(np.tanh(x @ w["w1p"].T + w["b1p"]) @ w["w2p"].T + w["b2p"])
    h2v = np.tanh(np.tanh(x @ w["w1v"].T + w["b1v"]) @ w["w2v"].T + w["b2v"])
    return w, h2p, h2v


def scales(sd, x):
    """(s_value [N], s_log_prob [N]) of the module text, from the float64 hidden activations."""
    w, h2p, h2v = _hidden64(sd, x)
    s_v = (np.abs(w["wv"][0]) * np.abs(h2v)).sum(axis=1) + abs(w["bv"][0])
    s_lp = (np.abs(h2p) @ np.abs(w["wa"]).T + np.abs(w["ba"])).max(axis=1)
    return s_v, s_lp


def log_softmax64(logits):
    lg = np.asarray(logits, dtype=np.float64)
    mx = lg.max(axis=1, keepdims=True)
    return lg - (mx + np.log(np.exp(lg - mx).sum(axis=1, keepdims=True)))


def deviations(values, logp_matrix, ref, s_v, s_lp):
    """Largest deviation of values [N] and of a log-softmax matrix [N, 9] from the float64 reference, in
    units of the scales."""
    dv = np.abs(np.asarray(values, dtype=np.float64) - ref.values) / s_v
    dl = np.abs(np.asarray(logp_matrix, dtype=np.float64) - log_softmax64(ref.logits)) / s_lp[:, None]
    return float(dv.max()), float(dl.max())


def torch_forward32(sd, x):
    """The torch-CPU float32 forward of MlpPolicyReference: (logits [N, 9], values [N], log-softmax)."""
    m = P.MlpPolicyReference(x.shape[1])
    m.load_state_dict(sd)
    with torch.no_grad():
        logits, value = m(torch.as_tensor(x).to(torch.float32))
        lsm = torch.log_softmax(logits, dim=1)
    return logits.numpy(), value.numpy(), lsm.numpy()


class Case:
    """One input set: obs [rows(D), D] int8, sd, uniforms [rows] (moved off the CDF boundaries), the
    float64 references of the three modes, the torch float32 forward and E_torch."""

    def __init__(self, D: int, weights: str):
        self.D, self.weights, n = D, weights, rows(D)
        for seed in range(50):  # (the all-zero rows cannot be redrawn: weights under which they have a margin)
            self.sd = make_state_dict(D, weights, seed)
            lg = np.sort(P.policy_reference(self.sd, np.zeros((1, D), np.int8), mode=P.ARGMAX).logits[0])
            if lg[-1] - lg[-2] > 2e-3:
                break
        rng = np.random.default_rng(31 * D + (weights == "scaled"))
        idx = np.arange(n)
        self.obs = _draw_rows(rng, idx, D)
        # ARGMAX without a tolerance: redraw a row until its top two float64 logits differ by > 1e-3
        for _ in range(200):
            lg = np.sort(P.policy_reference(self.sd, self.obs, mode=P.ARGMAX).logits, axis=1)
            bad = np.flatnonzero(lg[:, -1] - lg[:, -2] <= 1e-3)
            if not len(bad):
                break
            self.obs[bad] = _draw_rows(rng, bad, D)
        else:
            raise AssertionError(f"D={D} {weights}: rows {bad} keep top-two logit gaps under 1e-3")
        self.argmax = P.policy_reference(self.sd, self.obs, mode=P.ARGMAX)
        # SAMPLE without a tolerance: a uniform within 1e-4 of a float64 CDF boundary moves to the middle
        # of the interval it fell in
        u = (rng.integers(0, 1 << 24, size=n).astype(np.float64) * 2.0 ** -24)
        _, c = P.inverse_cdf(self.argmax.logits, u)
        edges = np.concatenate([np.zeros((n, 1)), c[:, :-1], np.ones((n, 1))], axis=1)  # interval a = [edges[a], edges[a+1])
        for e in range(n):
            if np.abs(u[e] - edges[e]).min() < 1e-4:
                a = min(int(np.searchsorted(edges[e, 1:-1], u[e], side="right")), P.N_ACTIONS - 1)
                u[e] = 0.5 * (edges[e, a] + edges[e, a + 1])
        self.uniforms = u.astype(np.float32)
        self.sample = P.policy_reference(self.sd, self.obs, self.uniforms, mode=P.SAMPLE)
        self.s_v, self.s_lp = scales(self.sd, self.obs)
        self.t_logits, self.t_values, self.t_lsm = torch_forward32(self.sd, self.obs)
        self.e_torch_v, self.e_torch_lp = deviations(self.t_values, self.t_lsm, self.sample, self.s_v, self.s_lp)

    def check(self, n, mode, actions, values, log_probs, label=""):
        """The kernel's outputs on the first n rows: actions equal to the float64 reference's, values and
        log_probs within MARGIN x E_torch.  Prints the figures before asserting.  Returns them."""
        ref = self.argmax if mode == P.ARGMAX else self.sample
        sl = slice(0, n)
        dv = float((np.abs(values.astype(np.float64) - ref.values[sl]) / self.s_v[sl]).max())
        fig = dict(D=self.D, N=n, weights=self.weights, mode=mode, e_torch_v=self.e_torch_v, kernel_v=dv)
        if mode != P.VALUE_ONLY:
            lsm = log_softmax64(ref.logits[sl])
            want_lp = lsm[np.arange(n), ref.actions[sl]]
            dl = float((np.abs(log_probs.astype(np.float64) - want_lp) / self.s_lp[sl]).max())
            fig.update(e_torch_lp=self.e_torch_lp, kernel_lp=dl)
        print("policy-tolerance", label, fig)
        if mode != P.VALUE_ONLY:
            assert np.array_equal(actions, ref.actions[sl]), np.flatnonzero(actions != ref.actions[sl])
            assert dl <= MARGIN * self.e_torch_lp, fig
        assert dv <= MARGIN * self.e_torch_v, fig
        return fig


@functools.lru_cache(maxsize=None)
def case(D: int, weights: str = "init") -> Case:
    return Case(D, weights)
