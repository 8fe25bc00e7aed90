"""pgtg_amd.policy on the CPU: MlpPolicyReference is SB3's MlpPolicy by name, shape and initialisation;
policy_reference is its forward plus the kernel's sampling rule; policy_uniform is pinned; and the inputs
and tolerance that test_gpu_policy.py holds the kernel k_policy to do discriminate (policy_cases.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import helpers
import policy_cases as pc
from pgtg_amd import policy as P

SB3_SHAPES = {
    "mlp_extractor.policy_net.0.weight": (64, "D"), "mlp_extractor.policy_net.0.bias": (64,),
    "mlp_extractor.policy_net.2.weight": (64, 64), "mlp_extractor.policy_net.2.bias": (64,),
    "mlp_extractor.value_net.0.weight": (64, "D"), "mlp_extractor.value_net.0.bias": (64,),
    "mlp_extractor.value_net.2.weight": (64, 64), "mlp_extractor.value_net.2.bias": (64,),
    "action_net.weight": (9, 64), "action_net.bias": (9,), "value_net.weight": (1, 64), "value_net.bias": (1,),
}


@pytest.mark.parametrize("D", [29, 1239])
def test_module_has_sb3s_names_shapes_and_init(D):
    torch.manual_seed(3)
    sd = P.MlpPolicyReference(D).state_dict()
    want = {k: tuple(D if s == "D" else s for s in v) for k, v in SB3_SHAPES.items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert P.weight_shapes(D) == want
    for k, v in sd.items():
        if k.endswith("bias"):
            assert not v.any()
    # orthogonal with SB3's gains: the smaller side of W is orthonormal times the gain
    for k, gain in (("mlp_extractor.policy_net.0.weight", math.sqrt(2)), ("mlp_extractor.value_net.2.weight", math.sqrt(2)),
                    ("action_net.weight", 0.01), ("value_net.weight", 1.0)):
        w = sd[k].double()
        g = w @ w.T if w.shape[0] <= w.shape[1] else w.T @ w
        assert torch.allclose(g, torch.eye(len(g), dtype=torch.float64) * gain ** 2, atol=1e-5 * gain ** 2), k


@pytest.mark.parametrize("D, weights", [(29, "init"), (29, "scaled"), (1239, "scaled")])
def test_float64_reference_is_the_modules_forward(D, weights):
    c = pc.case(D, weights)
    m = P.MlpPolicyReference(D).double()
    m.load_state_dict({k: v.double() for k, v in c.sd.items()})
    with torch.no_grad():
        logits, value = m(torch.as_tensor(c.obs).double())
    ref = c.sample
    assert np.allclose(ref.logits, logits.numpy(), rtol=0, atol=1e-12 * max(1.0, np.abs(ref.logits).max()))
    assert np.allclose(ref.values, value.numpy(), rtol=0, atol=1e-12 * max(1.0, np.abs(ref.values).max()))
    lsm = torch.log_softmax(logits, dim=1).numpy()
    assert np.allclose(ref.log_probs, lsm[np.arange(len(lsm)), ref.actions], rtol=0, atol=1e-12)
    assert np.array_equal(c.argmax.actions, logits.argmax(dim=1).numpy())
    only = P.policy_reference(c.sd, c.obs, mode=P.VALUE_ONLY)
    assert np.array_equal(only.values, ref.values) and only.actions is None and only.log_probs is None


def test_inverse_cdf_rule():
    big = np.full((1, 9), -1e4)
    for a in range(9):  # one action with all the mass, whatever u
        lg = big.copy()
        lg[0, a] = 0.0
        for u in (0.0, 0.5, 1 - 2.0 ** -24):
            assert P.inverse_cdf(lg, np.array([u]))[0][0] == a
    flat = np.zeros((1, 9))
    assert P.inverse_cdf(flat, np.array([0.0]))[0][0] == 0            # u = 0: the first action with mass
    lg = flat.copy()
    lg[0, 0] = -1e4
    assert P.inverse_cdf(lg, np.array([0.0]))[0][0] == 1              # (c_0 = 0 is not above u = 0)
    assert P.inverse_cdf(flat, np.array([1 - 2.0 ** -24]))[0][0] == 8  # the largest u
    assert P.inverse_cdf(flat, np.array([1 / 9 + 1e-9]))[0][0] == 1
    # c_8 <= u by construction: logits whose float32 running sum ends below 1, under the largest uniform
    top = np.float32(1 - 2.0 ** -24)
    lgs = np.random.default_rng(0).standard_normal((400, 9)).astype(np.float32)
    act, c = P.inverse_cdf(lgs, np.full(400, top), dtype=np.float32)
    short = c[:, 8] <= top
    assert c.dtype == np.float32 and short.any() and (~short).any()
    assert (act[short] == 8).all() and (act[~short] == 8).all()  # (by the last clause, and by u < c_8)
    act, c = P.inverse_cdf(flat, np.array([2.0]))  # any u at or above c_8: the rule's last clause
    assert c[0, 8] < 2.0 and act[0] == 8
    # the same rule inside policy_reference
    sd = pc.make_state_dict(5, "scaled")
    x = np.zeros((4, 5), np.int8)
    r = P.policy_reference(sd, x, np.array([0.0, 0.3, 0.9, 5.0], np.float32))
    want, _ = P.inverse_cdf(r.logits, [0.0, 0.3, 0.9, 5.0])
    assert np.array_equal(r.actions, want) and r.actions[0] == 0 and r.actions[3] == 8


def test_policy_uniform_properties_and_pinned_values():
    env = np.arange(5000, dtype=np.uint64)
    u = P.policy_uniform(7, 3, env)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    k = u.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(k, np.floor(k))
    assert 0.45 < u.mean() < 0.55 and len(np.unique(u)) > 4990
    for other in (P.policy_uniform(8, 3, env), P.policy_uniform(7, 4, env), P.policy_uniform(7, 3, env + np.uint64(5000))):
        assert (other != u).mean() > 0.99
    assert P.policy_uniform(7, 3, 11) == u[11]  # (a scalar env)
    # the draw a sampling reference makes on its own
    sd = pc.make_state_dict(5, "scaled")
    x = np.zeros((6, 5), np.int8)
    own = P.policy_reference(sd, x, None, seed=7, counter=3, env_offset=100)
    given = P.policy_reference(sd, x, P.policy_uniform(7, 3, 100 + np.arange(6)))
    assert np.array_equal(own.actions, given.actions)
    pins = json.load(open(os.path.join(helpers.GOLDEN, "policy_uniform.json")))
    assert len(pins) >= 12
    for p in pins:
        assert int(P.policy_uniform(p["seed"], p["counter"], p["env"]) * 2.0 ** 24) == p["u24"], p


CPU_SETS = [(d, w) for d in pc.DS + (pc.BIG_D,) for w in pc.WEIGHTS]


@pytest.mark.parametrize("D, weights", CPU_SETS)
def test_margins_and_tolerance_discriminate(D, weights):
    """On every GPU input set: the torch float32 forward alone reproduces every action of the float64
    reference (the margins are wide enough), and weights rounded once to bfloat16 miss the tolerance in
    logits and in value (the tolerance is tight enough)."""
    c = pc.case(D, weights)
    lg = np.sort(c.argmax.logits, axis=1)
    assert (lg[:, -1] - lg[:, -2] > 1e-3).all()
    assert np.array_equal(c.t_logits.argmax(axis=1), c.argmax.actions)
    a32, _ = P.inverse_cdf(c.t_logits, c.uniforms, dtype=np.float32)
    assert np.array_equal(a32, c.sample.actions)
    assert len(np.unique(c.sample.actions)) > 1 or D < 3
    assert c.e_torch_v > 0 and c.e_torch_lp > 0
    sd16 = {k: v.to(torch.bfloat16).to(torch.float32) for k, v in c.sd.items()}
    r16 = P.policy_reference(sd16, c.obs, c.uniforms)
    dv, dl = pc.deviations(r16.values, pc.log_softmax64(r16.logits), c.sample, c.s_v, c.s_lp)
    print("policy-tolerance-cpu", dict(D=D, weights=weights, e_torch_v=c.e_torch_v, e_torch_lp=c.e_torch_lp,
                                       bf16_v=dv, bf16_lp=dl))
    assert dv > pc.MARGIN * c.e_torch_v and dl > pc.MARGIN * c.e_torch_lp


def test_scaled_weights_saturate_and_spread():
    c = pc.case(1239, "scaled")
    assert np.abs(c.sample.logits).max() > 3.0
    w, h2p, _ = pc._hidden64(c.sd, c.obs)
    h1 = np.tanh(c.obs.astype(np.float64) @ w["w1p"].T + w["b1p"])
    assert (np.abs(h1) > 0.999).any()


def test_state_dict_errors_name_the_key():
    class FakeEnv:  # (load_state_dict refuses before anything touches the device)
        device = torch.device("cpu")
        _h = None

        class _lib:
            @staticmethod
            def pgtg_policy_packed_bytes(d, out):
                out._obj.value = 64
                return 0
    pol = P.DevicePolicy(FakeEnv(), obs_dim=29)
    sd = pc.make_state_dict(29, "init")
    missing = {k: v for k, v in sd.items() if k != "action_net.bias"}
    with pytest.raises(ValueError, match="action_net.bias"):
        pol.load_state_dict(missing)
    bad = dict(sd, **{"mlp_extractor.value_net.0.weight": torch.zeros(64, 30)})
    with pytest.raises(ValueError, match="mlp_extractor.value_net.0.weight"):
        pol.load_state_dict(bad)
    with pytest.raises(RuntimeError):
        pol.act(torch.zeros((2, 29), dtype=torch.int8))
