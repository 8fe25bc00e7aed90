"""The HIP kernel k_policy alone through pgtg_policy (include/pgtg.h) on the made-up input sets of
policy_cases.py -- actions equal to the float64 reference's, values and log-probabilities within four
times the torch float32 forward's own error -- and DevicePolicy / Rollout.collect against the existing
Rollout.step path."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
import policy_cases as pc
from pgtg_amd import _abi
from pgtg_amd import policy as P

pytestmark = pytest.mark.gpu

TRAIN = dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=0.2,
             random_map_percentage_of_connections=0.8, traffic_density=0.2, conservative_driver_percentage=0.15,
             normal_driver_percentage=0.50, aggressive_driver_percentage=0.20, elderly_driver_percentage=0.10,
             reckless_driver_percentage=0.05, sliding_observation_window_size=5, max_allowed_deviation=15,
             use_sliding_observation_window=True, use_next_subgoal_direction=True, final_goal_bonus=200,
             standing_still_penalty=1)
SENT_A, SENT_F = 0xEE, -777.0


def _vec(n, **kw):
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PGTGVecEnv(n, device=0, **kw)


@pytest.fixture(scope="module")
def handle():
    env = _vec(2, random_map_width=3, random_map_height=3)  # (its batch size is not the policy's)
    yield env
    env.close()


_POLICIES = {}


def _policy(handle, D, weights):
    """A DevicePolicy packed from the set's state dict (one per set and module)."""
    if (D, weights) not in _POLICIES:
        pol = P.DevicePolicy(handle, obs_dim=D, seed=9)
        pol.load_state_dict(pc.case(D, weights).sd)
        _POLICIES[(D, weights)] = pol
    return _POLICIES[(D, weights)]


def _obs(x, shift):
    """x [N, D] int8 on the device, starting `shift` bytes into a storage that ends exactly with it; the
    bytes in front of it are 0x7F."""
    n = x.size
    store = torch.full((shift + n,), 0x7F, dtype=torch.int8, device="cuda")
    assert store.untyped_storage().nbytes() == shift + n
    t = store[shift:].view(x.shape)
    t.copy_(torch.as_tensor(x))
    assert t.data_ptr() == store.data_ptr() + shift and t.is_contiguous()
    return t


def _call(handle, pol, obs, mode, uniforms=None, want=("actions", "values", "log_probs"), n=None, obs_dim=None,
          counter=0, env_offset=0, packed=True, obs_ptr=True):
    """pgtg_policy with a sentinel row before and after every output; returns (rc, outputs as host arrays
    without the guards, the guard rows intact?)."""
    N = obs.shape[0]
    outs = {"actions": torch.full((N + 2,), SENT_A, dtype=torch.uint8, device="cuda"),
            "values": torch.full((N + 2,), SENT_F, device="cuda"), "log_probs": torch.full((N + 2,), SENT_F, device="cuda")}
    p = lambda k: C.c_void_p(outs[k].data_ptr() + outs[k].element_size()) if k in want else None  # noqa: E731
    a = _abi.PgtgPolicy(n=N if n is None else n, obs_dim=obs.shape[1] if obs_dim is None else obs_dim,
                        obs=C.c_void_p(obs.data_ptr()) if obs_ptr else None,
                        packed=C.c_void_p(pol._packed.data_ptr()) if packed else None, mode=mode, seed=pol.seed,
                        counter=counter, env_offset=env_offset,
                        uniforms=None if uniforms is None else C.c_void_p(uniforms.data_ptr()),
                        actions=p("actions"), values=p("values"), log_probs=p("log_probs"))
    handle._bind_stream()
    rc = handle._lib.pgtg_policy(handle._h, C.byref(a))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    sent = {"actions": SENT_A, "values": np.float32(SENT_F), "log_probs": np.float32(SENT_F)}
    guards = all(host[k][0] == sent[k] and host[k][-1] == sent[k] for k in host)
    untouched = {k: bool((host[k] == sent[k]).all()) for k in host}
    return rc, {k: v[1:-1] for k, v in host.items()}, guards, untouched


def test_the_module_follows_the_kernels_chunk(handle):
    assert handle._lib.pgtg_policy_chunk() == P.K_CHUNK


@pytest.mark.parametrize("weights", pc.WEIGHTS)
@pytest.mark.parametrize("N, D", pc.SHAPES)
def test_k_policy_matches_the_reference(handle, N, D, weights):
    c = pc.case(D, weights)
    pol = _policy(handle, D, weights)
    shifts = (0, 1, 4, 15) if (N == 65 or D in pc.FULL_N_DS) and D != pc.BIG_D else (1,)
    uni = torch.as_tensor(c.uniforms[:N]).cuda()
    first = None
    for shift in shifts:
        obs = _obs(c.obs[:N], shift)
        rc, out, guards, _ = _call(handle, pol, obs, P.SAMPLE, uni)
        assert rc == 0 and guards, shift
        if first is None:
            first = out
            c.check(N, P.SAMPLE, out["actions"], out["values"], out["log_probs"], "sample")
        else:  # (the base alignment changes nothing: the same bits)
            for k in out:
                assert np.array_equal(out[k].view(np.uint8), first[k].view(np.uint8)), (k, shift)
    obs = _obs(c.obs[:N], shifts[-1])
    rc, arg, guards, _ = _call(handle, pol, obs, P.ARGMAX)
    assert rc == 0 and guards
    c.check(N, P.ARGMAX, arg["actions"], arg["values"], arg["log_probs"], "argmax")
    assert np.array_equal(arg["values"].view(np.int32), first["values"].view(np.int32))
    # VALUE_ONLY: the same value bits, nothing else written
    rc, vo, guards, untouched = _call(handle, pol, obs, P.VALUE_ONLY)
    assert rc == 0 and guards and untouched["actions"] and untouched["log_probs"]
    assert np.array_equal(vo["values"].view(np.int32), first["values"].view(np.int32))
    # the same call twice: the same bits
    rc, again, _, _ = _call(handle, pol, _obs(c.obs[:N], shifts[0]), P.SAMPLE, uni)
    for k in again:
        assert np.array_equal(again[k].view(np.uint8), first[k].view(np.uint8)), k


@pytest.mark.parametrize("N, D", [(65, 29), (257, 1239)])
def test_null_outputs_leave_the_others_identical(handle, N, D):
    c, pol = pc.case(D, "scaled"), _policy(handle, D, "scaled")
    obs, uni = _obs(c.obs[:N], 1), torch.as_tensor(c.uniforms[:N]).cuda()
    _, full, _, _ = _call(handle, pol, obs, P.SAMPLE, uni)
    for want in (("actions",), ("values",), ("log_probs",), ("actions", "log_probs"), ("values", "log_probs")):
        rc, out, guards, untouched = _call(handle, pol, obs, P.SAMPLE, uni, want=want)
        assert rc == 0 and guards
        for k in out:
            if k in want:
                assert np.array_equal(out[k].view(np.uint8), full[k].view(np.uint8)), (want, k)
            else:
                assert untouched[k], (want, k)


@pytest.mark.parametrize("N, D", [(65, 29), (257, 1239)])
def test_self_drawn_uniforms_are_policy_uniform(handle, N, D):
    c, pol = pc.case(D, "scaled"), _policy(handle, D, "scaled")
    obs = _obs(c.obs[:N], 4)
    seen = []
    for counter, off in ((0, 0), (5, 0), (5, 1000), ((1 << 40) + 3, (1 << 33) + 7)):
        rc, own, guards, _ = _call(handle, pol, obs, P.SAMPLE, None, counter=counter, env_offset=off)
        u = P.policy_uniform(pol.seed, counter, off + np.arange(N, dtype=np.uint64))
        rc2, given, _, _ = _call(handle, pol, obs, P.SAMPLE, torch.as_tensor(u).cuda())
        assert rc == rc2 == 0 and guards
        for k in own:
            assert np.array_equal(own[k].view(np.uint8), given[k].view(np.uint8)), (k, counter, off)
        seen.append(own["actions"])
    if N > 100:
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


def test_pack_from_views_and_cpu_tensors_and_repack(handle):
    D, N = 29, 65
    c = pc.case(D, "scaled")
    obs, uni = _obs(c.obs[:N], 0), torch.as_tensor(c.uniforms[:N]).cuda()
    base = _policy(handle, D, "scaled")
    _, want, _, _ = _call(handle, base, obs, P.SAMPLE, uni)
    # non-contiguous views on the device: every tensor the transpose of a transposed copy, or a strided slice
    views = {}
    for k, v in c.sd.items():
        if v.dim() == 2:
            views[k] = v.t().contiguous().cuda().t()
        else:
            wide = torch.zeros(2 * len(v), device="cuda")
            wide[::2] = v.cuda()
            views[k] = wide[::2]
    assert sum(not v.is_contiguous() for v in views.values()) >= 10
    for sd in (views, {k: v.cpu() for k, v in c.sd.items()}, {k: v.double() for k, v in c.sd.items()}):
        pol = P.DevicePolicy(handle, obs_dim=D, seed=9)
        pol.load_state_dict(sd)
        _, out, _, _ = _call(handle, pol, obs, P.SAMPLE, uni)
        for k in out:
            assert np.array_equal(out[k].view(np.uint8), want[k].view(np.uint8)), k
    # an in-place weight change and a repack: other outputs, and the old ones do not come back
    pol = P.DevicePolicy(handle, obs_dim=D, seed=9)
    sd = {k: v.clone().cuda() for k, v in c.sd.items()}
    pol.load_state_dict(sd)
    sd["value_net.bias"].add_(1.0)
    sd["action_net.weight"].mul_(-1.0)
    _, stale, _, _ = _call(handle, pol, obs, P.SAMPLE, uni)  # (not repacked yet: the packed copy is the kernel's)
    assert np.array_equal(stale["values"], want["values"])
    pol.load_state_dict(sd)
    for _ in range(2):
        _, out, _, _ = _call(handle, pol, obs, P.SAMPLE, uni)
        assert np.allclose(out["values"], want["values"] + 1.0, rtol=0, atol=1e-5)
        assert not np.array_equal(out["log_probs"], want["log_probs"])
    ref = P.policy_reference({k: v.cpu() for k, v in sd.items()}, c.obs[:N], c.uniforms[:N])
    assert np.allclose(out["log_probs"], ref.log_probs, rtol=0, atol=1e-4)


def test_refusals_launch_nothing(handle):
    D, N = 29, 65
    c, pol = pc.case(D, "init"), _policy(handle, D, "init")
    obs = _obs(c.obs[:N], 0)
    cases = [(dict(obs_dim=0), "obs_dim"), (dict(obs_ptr=False), "obs and packed"), (dict(packed=False), "obs and packed"),
             (dict(mode=3), "mode"), (dict(mode=-1), "mode"), (dict(n=1 << 63, obs_dim=4), "overflow"),
             (dict(obs_dim=_abi.PGTG_POLICY_MAX_OBS_DIM + 1), "PGTG_POLICY_MAX_OBS_DIM"),
             (dict(mode=P.VALUE_ONLY, want=("actions", "log_probs")), "values")]
    for kw, word in cases:
        mode = kw.pop("mode", P.SAMPLE)
        rc, _, guards, untouched = _call(handle, pol, obs, mode, **kw)
        msg = handle._lib.pgtg_last_error(handle._h).decode()
        assert rc == _abi.PGTG_E_INVALID and msg.startswith("pgtg_policy") and word in msg, (kw, msg)
        assert guards and all(untouched.values()), kw
    rc, _, guards, untouched = _call(handle, pol, obs, P.SAMPLE, n=0)  # no envs: nothing to do
    assert rc == 0 and all(untouched.values())
    nbytes = C.c_uint64()
    assert handle._lib.pgtg_policy_packed_bytes(0, C.byref(nbytes)) == _abi.PGTG_E_INVALID
    assert handle._lib.pgtg_policy_packed_bytes(_abi.PGTG_POLICY_MAX_OBS_DIM + 1, C.byref(nbytes)) == _abi.PGTG_E_INVALID
    with pytest.raises(ValueError):
        pol.act(obs.to(torch.float32))
    with pytest.raises(ValueError):
        pol.act(obs, values=torch.zeros(N, dtype=torch.float64, device="cuda"))


def test_device_policy_act_and_value(handle):
    D, N = 1239, 257
    c, pol = pc.case(D, "scaled"), _policy(handle, D, "scaled")
    obs, uni = _obs(c.obs[:N], 0), torch.as_tensor(c.uniforms[:N]).cuda()
    a, v, lp = pol.act(obs, uniforms=uni)
    assert a.dtype == torch.uint8 and v.dtype == lp.dtype == torch.float32
    c.check(N, P.SAMPLE, a.cpu().numpy(), v.cpu().numpy(), lp.cpu().numpy(), "act")
    a2, v2, _ = pol.act(obs, deterministic=True)
    assert np.array_equal(a2.cpu().numpy(), c.argmax.actions[:N]) and torch.equal(v2, v)
    rows = torch.zeros(N, device="cuda")
    assert pol.value(obs, out=rows) is rows and torch.equal(rows, v)
    k0 = pol.counter
    a3, _, _ = pol.act(obs)
    a4, _, _ = pol.act(obs)
    assert pol.counter == k0 + 2 and not torch.equal(a3, a4)
    want = P.policy_reference(c.sd, c.obs[:N], None, seed=pol.seed, counter=k0, env_offset=0)
    assert (a3.cpu().numpy() == want.actions).mean() > 0.99  # (its own uniforms are not kept off the boundaries)
    pol.act(obs, uniforms=uni)
    pol.act(obs, deterministic=True)
    assert pol.counter == k0 + 2


N_RO, T_RO, LIMIT = 96, 5, 3
KEYS = ("obs", "actions", "rewards", "dones", "truncated_only", "values", "log_probs", "terminal_values",
        "advantages", "returns")


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.bool else t.to(torch.uint8)


def test_collect_is_the_step_path_bit_for_bit():
    from pgtg_amd.flat import flat_dim
    a = _vec(N_RO, autoreset=True, max_episode_steps=LIMIT, **TRAIN)
    b = _vec(N_RO, autoreset=True, max_episode_steps=LIMIT, **TRAIN)
    D = flat_dim(a.spec)
    torch.manual_seed(4)
    sd = P.MlpPolicyReference(D).state_dict()
    sd["action_net.weight"] = sd["action_net.weight"] * 100.0
    pa, pb = P.DevicePolicy(a, seed=21), P.DevicePolicy(b, seed=21)
    assert pa.obs_dim == D
    pa.load_state_dict(sd)
    pb.load_state_dict(sd)
    ra, rb = a.rollout(T_RO), b.rollout(T_RO)
    ra.begin(seed=7)
    for k in range(2):  # the second rollout continues the episodes: row T becomes row 0
        last = {key: getattr(ra, key).clone() for key in ("obs", "dones")} if k else None
        ra.collect(pa)
        if k:
            assert torch.equal(ra.obs[0], last["obs"][T_RO]) and torch.equal(ra.dones[0], last["dones"][T_RO])
            assert not bool(ra.dones[0].all())
        # the existing path: separate act() calls with the same uniforms, fed to Rollout.step
        obs = rb.begin(seed=7) if k == 0 else rb.begin()
        for t in range(T_RO):
            u = torch.as_tensor(P.policy_uniform(21, k * T_RO + t, np.arange(N_RO, dtype=np.uint64))).cuda()
            act, val, lp = pb.act(obs, uniforms=u)
            obs, _, _ = rb.step(act, val, lp)
            rb.set_terminal_values(pb.value(rb.terminal_obs))
        rb.finish(pb.value(obs))
        torch.cuda.synchronize()
        assert pa.counter == (k + 1) * T_RO
        for key in KEYS:
            assert torch.equal(_bits(getattr(ra, key)), _bits(getattr(rb, key))), (k, key)
        # (a limit of 3 steps truncates wherever the sampled actions do not crash first: about a third of the envs)
        assert float(ra.truncated_only.any(dim=0).float().mean()) > 0.2
        assert len(torch.unique(ra.actions)) > 1 and bool(torch.isfinite(ra.advantages).all())
    # the values of the truncated rows did enter the returns
    assert bool((ra.terminal_values[ra.truncated_only] != 0).any())
    for ro, env in ((ra, a), (rb, b)):
        ro.close()
        env.close()


def test_collect_refuses_float32_rows():
    env = _vec(4, autoreset=True, max_episode_steps=3, random_map_width=3, random_map_height=3)
    pol = P.DevicePolicy(env)
    torch.manual_seed(1)
    pol.load_state_dict(P.MlpPolicyReference(pol.obs_dim).state_dict())
    ro = env.rollout(2, obs_dtype=torch.float32)
    with pytest.raises(ValueError, match="int8"):
        ro.collect(pol)
    ro.begin(seed=1)
    with pytest.raises(ValueError, match="int8"):
        ro.act(pol)
    ro.step(torch.zeros(4, dtype=torch.uint8, device="cuda"))  # (step keeps working for it)
    ro.close()
    env.close()
