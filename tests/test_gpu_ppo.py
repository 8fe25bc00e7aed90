"""The HIP kernels k_ppo_loss, k_ppo_dw1 and k_ppo_reduce through pgtg_ppo_grad (include/pgtg.h) on the made-up
rollouts of ppo_cases.py -- every gradient tensor and statistic within four times torch float32 autograd's
own error -- and DevicePolicy.ppo_grad / Rollout.update against torch autograd on a collected rollout."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
import ppo_cases as ppc
from pgtg_amd import _abi
from pgtg_amd import policy as P

pytestmark = pytest.mark.gpu

# the training caller's settings (test_gpu_policy.py's TRAIN)
TRAIN = dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=0.2,
             random_map_percentage_of_connections=0.8, traffic_density=0.2, conservative_driver_percentage=0.15,
             normal_driver_percentage=0.50, aggressive_driver_percentage=0.20, elderly_driver_percentage=0.10,
             reckless_driver_percentage=0.05, sliding_observation_window_size=5, max_allowed_deviation=15,
             use_sliding_observation_window=True, use_next_subgoal_direction=True, final_goal_bonus=200,
             standing_still_penalty=1)

SENT = -777.0
T, N, TOTAL = ppc.T, ppc.N, ppc.TOTAL


def _vec(n, **kw):
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PGTGVecEnv(n, device=0, **kw)


@pytest.fixture(scope="module")
def handle():
    env = _vec(2, random_map_width=3, random_map_height=3)  # (its batch size is not the rollout's)
    yield env
    env.close()


class _Dev:
    """A case's rollout on the device; obs(shift) starts `shift` bytes into a storage that ends exactly with
    the last row, rows ppc.pitch(D) bytes apart, every other byte 0x7F."""

    def __init__(self, handle, D):
        self.c = c = ppc.case(D)
        self.D, self.pitch = D, ppc.pitch(D)
        self.pol = P.DevicePolicy(handle, obs_dim=D, seed=9)
        self.pol.load_state_dict(c.sd)
        cu = lambda x: torch.as_tensor(x).cuda().contiguous()  # noqa: E731
        self.actions, self.old, self.adv, self.ret = cu(c.actions), cu(c.old_log_probs), cu(c.advantages), cu(c.returns)
        self._obs = {}

    def obs(self, shift):
        if shift not in self._obs:
            n = shift + (T - 1) * self.pitch + N * self.D
            store = torch.full((n,), 0x7F, dtype=torch.int8, device="cuda")
            assert store.untyped_storage().nbytes() == n
            view = store[shift:].as_strided((T, N, self.D), (self.pitch, self.D, 1))
            view.copy_(torch.as_tensor(self.c.obs))
            assert view.data_ptr() == store.data_ptr() + shift
            self._obs[shift] = (store, view)
        return self._obs[shift][1]


_DEVS = {}


def _dev(handle, D):
    if D not in _DEVS:
        _DEVS[D] = _Dev(handle, D)
    return _DEVS[D]


def _call(handle, dv, idx, norm, ent, shift=0, clip=ppc.CLIP, vf=ppc.VF, **over):
    """pgtg_ppo_grad with a sentinel word before and after every output tensor and the stats.  Returns (rc,
    grads {key: array}, stats [8], the sentinels intact?, every output untouched?).  over: struct fields to
    replace (a value of None: a NULL pointer); grads_null names one gradient field to pass as NULL."""
    D = dv.D
    idx = torch.as_tensor(idx, dtype=torch.int64).cuda()
    B = idx.numel()
    outs = {key: torch.full((int(np.prod(shape)) + 2,), SENT, device="cuda") for key, shape in P.weight_shapes(D).items()}
    outs["stats"] = torch.full((8 + 2,), SENT, device="cuda")
    raw = _abi.PgtgPpoGrads()
    for field, (key, _) in P.WEIGHT_KEYS.items():
        setattr(raw, field, None if over.get("grads_null") == field else outs[key].data_ptr() + 4)
    over.pop("grads_null", None)
    nbytes = C.c_uint64()
    assert handle._lib.pgtg_ppo_workspace_bytes(D, max(B, 1), C.byref(nbytes)) == 0
    ws = torch.full((nbytes.value // 4 + 8,), float("nan"), device="cuda")  # (the kernels need no memset)
    adv_stats = None
    if norm and B > 1:
        a = dv.adv[idx % T, idx // T]
        adv_stats = torch.stack((a.mean(), 1.0 / (a.std() + 1e-8)))
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    obs = dv.obs(shift)
    fields = dict(batch=B, obs_dim=D, steps=T, n=N, obs_pitch=dv.pitch, obs=p(obs), indices=p(idx), actions=p(dv.actions),
                  log_probs=p(over.pop("old", dv.old)), advantages=p(dv.adv), returns=p(dv.ret), packed=p(dv.pol._packed),
                  adv_stats=p(adv_stats), clip_range=clip, ent_coef=ent, vf_coef=vf, workspace=p(ws), grads=raw,
                  stats=C.c_void_p(outs["stats"].data_ptr() + 4))
    fields.update(over)
    handle._bind_stream()
    rc = handle._lib.pgtg_ppo_grad(handle._h, C.byref(_abi.PgtgPpoGrad(**fields)))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    guards = all(v[0] == np.float32(SENT) and v[-1] == np.float32(SENT) for v in host.values())
    untouched = all(bool((v == np.float32(SENT)).all()) for v in host.values())
    grads = {k: host[k][1:-1].reshape(s) for k, s in P.weight_shapes(D).items()}
    return rc, grads, host["stats"][1:-1], guards, untouched


def _same_bits(a, b):
    (ga, sa), (gb, sb) = a, b
    return all(np.array_equal(ga[k].view(np.uint32), gb[k].view(np.uint32)) for k in ga) and \
        np.array_equal(sa.view(np.uint32), sb.view(np.uint32))


@pytest.mark.parametrize("B, D", ppc.SHAPES)
def test_ppo_grad_matches_the_reference(handle, B, D):
    dv = _dev(handle, D)
    c, idx = dv.c, dv.c.indices(B)
    first = None
    for norm, ent in ppc.CONFIGS:
        rc, g, s, guards, _ = _call(handle, dv, idx, norm, ent)
        assert rc == 0 and guards, (norm, ent)
        assert s[6] == 0 and s[7] == 0
        c.check(g, s, c.reference(B, norm, ent), f"B={B} D={D} norm={norm} ent={ent}")
        if first is None:
            first = (g, s)
    norm, ent = ppc.CONFIGS[0]
    for shift in (0, 1, 4, 15):  # the same call again, and the obs base at other alignments: the same bits
        rc, g, s, guards, _ = _call(handle, dv, idx, norm, ent, shift=shift)
        assert rc == 0 and guards and _same_bits((g, s), first), shift


def test_repeats_every_sample_once_and_a_permutation(handle):
    D = 29
    dv = _dev(handle, D)
    c = dv.c
    norm, ent = True, 0.01
    # repeats: 40 samples, each three times, interleaved
    idx = np.tile(c.perm[:40], 3)
    b = c.batch(idx)
    ref = P.ppo_reference(c.sd, *b, ppc.CLIP, ent, ppc.VF, norm) + ppc.magnitudes(c.sd, *b, ppc.CLIP, ent, ppc.VF, norm)
    rc, g, s, guards, _ = _call(handle, dv, idx, norm, ent)
    assert rc == 0 and guards
    c.check(g, s, ref, "repeats")
    # every sample exactly once: also the whole rollout's reference in its own order
    rc, g, s, guards, _ = _call(handle, dv, c.perm, norm, ent)
    assert rc == 0 and guards
    c.check(g, s, c.reference(TOTAL, norm, ent), "all once")
    b = c.batch(np.arange(TOTAL))
    whole = P.ppo_reference(c.sd, *b, ppc.CLIP, ent, ppc.VF, norm) + ppc.magnitudes(c.sd, *b, ppc.CLIP, ent, ppc.VF, norm)
    c.check(g, s, whole, "all once vs the rollout's order")
    # a permutation of the batch: within tolerance (the summation order follows the batch order)
    B = 257
    idx = c.indices(B)
    rc, g1, s1, guards, _ = _call(handle, dv, idx[np.random.default_rng(3).permutation(B)], norm, ent)
    assert rc == 0 and guards
    c.check(g1, s1, c.reference(B, norm, ent), "permuted")


def test_the_forward_is_k_policys(handle):
    """old_log_probs = k_policy's own for the same weights and actions: approx_kl and the clip fraction are
    exactly 0.  (The forward is k_policy's own code, shared through pgtg_policy.h; this pins the log-probs a
    rollout stores to the ones k_ppo_loss recomputes, through the gather and the whole call.)"""
    D = 1239
    dv = _dev(handle, D)
    c = dv.c
    lp = torch.zeros((T, N), device="cuda")
    act = torch.zeros((T, N), dtype=torch.uint8, device="cuda")
    saved = dv.actions
    try:
        for t in range(T):
            dv.pol.act(dv.obs(0)[t].contiguous(), actions=act[t], log_probs=lp[t])
        dv.actions = act
        rc, g, s, guards, _ = _call(handle, dv, c.perm, False, 0.0, old=lp)
    finally:
        dv.actions = saved
    print("ppo-consistency approx_kl", float(s[4]), "clip fraction", float(s[5]))
    assert rc == 0 and guards
    assert s[4] == 0 and s[5] == 0


def test_refusals_launch_nothing(handle):
    D = 29
    dv = _dev(handle, D)
    idx = dv.c.indices(65)
    off1 = lambda t: C.c_void_p(t.data_ptr() + 4)  # noqa: E731
    cases = [(dict(obs=None), "required"), (dict(indices=None), "required"), (dict(actions=None), "required"),
             (dict(old=None), "required"), (dict(advantages=None), "required"), (dict(returns=None), "required"),
             (dict(packed=None), "required"), (dict(workspace=None), "required"), (dict(stats=None), "required"),
             (dict(grads_null="w1p"), "gradient"), (dict(grads_null="bv"), "gradient"),
             (dict(obs_dim=0), "obs_dim"), (dict(obs_dim=_abi.PGTG_POLICY_MAX_OBS_DIM + 1), "obs_dim"),
             (dict(steps=0), "steps"), (dict(n=0), "steps"), (dict(obs_pitch=N * D - 1), "obs_pitch"),
             (dict(packed=off1(dv.pol._packed)), "aligned"), (dict(workspace=off1(dv.adv)), "aligned"),
             (dict(n=1 << 62), "overflow"), (dict(steps=1 << 62), "overflow"), (dict(obs_pitch=1 << 63), "overflow"),
             (dict(batch=1 << 60), "overflow")]
    for over, word in cases:
        rc, _, _, guards, untouched = _call(handle, dv, idx, True, 0.0, **dict(over))
        msg = handle._lib.pgtg_last_error(handle._h).decode()
        assert rc == _abi.PGTG_E_INVALID and msg.startswith("pgtg_ppo_grad") and word in msg, (over, rc, msg)
        assert guards and untouched, over
    rc, _, _, guards, untouched = _call(handle, dv, idx, True, 0.0, batch=0)  # no samples: nothing to do
    assert rc == 0 and guards and untouched


def test_an_index_out_of_range_is_skipped_and_counted(handle):
    D = 29
    dv = _dev(handle, D)
    c = dv.c
    B, ent = 65, 0.01
    good = c.indices(B - 2)
    idx = np.concatenate([good[:10], [TOTAL], good[10:], [-1]])  # batch positions 10 and 64: error bytes 0 and 0
    handle.reset(seed=1)  # (a reset clears the error bytes)
    assert handle.error_count()[0] == 0
    rc, g, s, guards, _ = _call(handle, dv, idx, False, ent)
    assert rc == 0 and guards
    assert handle.error_count() == (1, _abi.PGTG_E_INVALID)
    # the other samples' sums are what they are alone; the means stay over B
    b, f = c.batch(good), (B - 2) / B
    rg, rs = P.ppo_reference(c.sd, *b, ppc.CLIP, ent, ppc.VF, False)
    mg, ms = ppc.magnitudes(c.sd, *b, ppc.CLIP, ent, ppc.VF, False)
    scale = lambda d: {k: v * f for k, v in d.items()}  # noqa: E731
    c.check(g, s, (scale(rg), rs * f, scale(mg), ms * f), "out of range")
    handle.reset(seed=1)
    assert handle.error_count()[0] == 0


N_RO, T_RO, LIMIT = 96, 5, 3


def _collected(seed_module=4):
    from pgtg_amd.flat import flat_dim
    env = _vec(N_RO, autoreset=True, max_episode_steps=LIMIT, **TRAIN)
    D = flat_dim(env.spec)
    torch.manual_seed(seed_module)
    module = P.MlpPolicyReference(D).cuda()
    with torch.no_grad():
        module.action_net.weight.mul_(100.0)
    pol = P.DevicePolicy(env, seed=21)
    pol.load_state_dict(module.state_dict())
    ro = env.rollout(T_RO)
    ro.begin(seed=7)
    ro.collect(pol)
    return env, module, pol, ro


def _truth(module, ro, idx, clip, ent, vf, norm):
    """(float64 reference, magnitudes) of the batch idx of a collected rollout under module's weights."""
    sd = {k: v.detach().cpu() for k, v in module.state_dict().items()}
    e, t = (idx // ro.n_steps).cpu().numpy(), (idx % ro.n_steps).cpu().numpy()
    h = lambda x: x.cpu().numpy()[t, e]  # noqa: E731
    b = (ro.obs.cpu().numpy()[t, e], h(ro.actions), h(ro.log_probs), h(ro.advantages), h(ro.returns))
    return sd, b, P.ppo_reference(sd, *b, clip, ent, vf, norm) + ppc.magnitudes(sd, *b, clip, ent, vf, norm)


def test_device_policy_ppo_grad_on_a_collected_rollout():
    env, module, pol, ro = _collected()
    D = pol.obs_dim
    with pytest.raises(ValueError):
        P.DevicePolicy(env).ppo_grad(ro, torch.arange(4, device="cuda"))  # no weights
    torch.manual_seed(11)
    with torch.no_grad():  # the weights move after the rollout, as in an update's second minibatch
        for p in module.parameters():
            p.add_(0.02 * p.abs().mean() * torch.randn_like(p))
    pol.load_state_dict(module.state_dict())
    idx = torch.randperm(N_RO * T_RO, device="cuda")[:200]
    clip, ent, vf, norm = 0.2, 0.01, 0.5, True
    grads, stats = pol.ppo_grad(ro, idx, clip_range=clip, ent_coef=ent, vf_coef=vf, normalize_advantage=norm)
    assert stats.shape == (8,) and stats.is_cuda and set(grads) == set(P.weight_shapes(D))
    # torch autograd on the GPU over get()'s batch
    obs_b, act_b, _, logp_b, adv_b, ret_b = next(ro.get(indices=idx))
    module.zero_grad()
    loss, tstats = ppc.torch_ppo(module, obs_b, act_b, logp_b, adv_b, ret_b, clip, ent, vf, norm)
    loss.backward()
    tg = {k: p.grad.cpu().numpy() for k, p in module.named_parameters()}
    _, _, ref = _truth(module, ro, idx, clip, ent, vf, norm)
    e_torch = ppc.deviations(tg, tstats.cpu().numpy(), *ref)
    c = ppc.case(29)
    c.check({k: v.cpu().numpy() for k, v in grads.items()}, stats.cpu().numpy(), ref, "collected", e_torch=e_torch)
    # the .grad form writes in place; the policy's own set is kept
    mine = {k: p.grad for k, p in module.named_parameters()}
    ptrs = {k: v.data_ptr() for k, v in mine.items()}
    out, stats2 = pol.ppo_grad(ro, idx, grads=mine, clip_range=clip, ent_coef=ent, vf_coef=vf, normalize_advantage=norm)
    assert out is mine and all(p.grad.data_ptr() == ptrs[k] for k, p in module.named_parameters())
    assert all(torch.equal(mine[k], grads[k]) for k in mine) and torch.equal(stats, stats2)
    again, _ = pol.ppo_grad(ro, idx[:7])
    assert again is grads
    # an index outside the rollout with normalisation on: the sample is skipped and counted, and stands as an
    # advantage of 0 in the mean and the std; the rest is the reference on pre-normalised advantages, means over B
    good = idx[:100]
    bad = torch.cat([good[:37], torch.tensor([N_RO * T_RO], device="cuda"), good[37:]])
    assert env.error_count()[0] == 0
    g2, s2 = pol.ppo_grad(ro, bad, clip_range=clip, ent_coef=ent, vf_coef=vf, normalize_advantage=True)
    assert env.error_count() == (1, _abi.PGTG_E_INVALID)
    sd, b, _ = _truth(module, ro, good, clip, ent, vf, False)
    a0 = np.concatenate([b[3].astype(np.float64), [0.0]])
    adv_n = ((b[3] - a0.mean()) / (a0.std(ddof=1) + 1e-8)).astype(np.float32)
    b, f = b[:3] + (adv_n,) + b[4:], 100 / 101
    rg, rs = P.ppo_reference(sd, *b, clip, ent, vf, False)
    mg, ms = ppc.magnitudes(sd, *b, clip, ent, vf, False)
    tg2, ts2 = ppc.torch_grads(sd, *b, clip, ent, vf, False, device="cuda")
    scale = lambda d: {k: v * f for k, v in d.items()}  # noqa: E731
    # E_torch here is one torch run on one batch, and a single float32 result can by chance lie far inside its
    # own rounding interval (1.7e-9 for the value loss at the first measurement); no float32 output can be asked
    # to be nearer the truth than float32 resolves, 2^-24 of its magnitude, so E_torch is not taken below that
    e2 = {k: max(v, 2.0 ** -24) for k, v in ppc.deviations(tg2, ts2, rg, rs, mg, ms).items()}
    c.check({k: v.cpu().numpy() for k, v in g2.items()}, s2.cpu().numpy(), (scale(rg), rs * f, scale(mg), ms * f),
            "collected, one index out of range", e_torch=e2)
    # refusals of the wrapper
    other = _vec(4, autoreset=True, max_episode_steps=3, random_map_width=3, random_map_height=3)
    for bad in (other.rollout(2), other.rollout(2, obs_dtype=torch.float32), env.rollout(2)):
        with pytest.raises(ValueError):
            pol.ppo_grad(bad, idx[:4])
    other.close()
    ro.close()
    env.close()


def _torch_loop(module, ro, dtype, n_epochs, bs, lr, seed, clip, ent, vf, max_norm):
    opt = torch.optim.Adam(module.parameters(), lr=lr, eps=1e-5)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    total = ro.n_steps * ro.num_envs
    for _ in range(n_epochs):
        perm = torch.randperm(total, device="cuda", generator=gen)
        for lo in range(0, total, bs):
            obs_b, act_b, _, logp_b, adv_b, ret_b = next(ro.get(indices=perm[lo:lo + bs]))
            loss, _ = ppc.torch_ppo(module, obs_b.to(dtype), act_b, logp_b.to(dtype), adv_b.to(dtype), ret_b.to(dtype),
                                    clip, ent, vf, True)
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(module.parameters(), max_norm)
            opt.step()


def test_rollout_update_follows_the_torch_loop():
    ea, ma, pa, ra = _collected()
    eb, mb, pb, rb = _collected()
    for key in ("obs", "actions", "log_probs", "advantages", "returns"):
        assert torch.equal(getattr(ra, key), getattr(rb, key)), key
    m64 = P.MlpPolicyReference(pa.obs_dim).cuda().double()
    m64.load_state_dict({k: v.double() for k, v in mb.state_dict().items()})
    kw = dict(n_epochs=2, bs=120, lr=1e-3, seed=3, clip=0.2, ent=0.01, vf=0.5, max_norm=0.5)  # 4 minibatches of 120

    def value_loss(m):
        obs_b, _, _, _, _, ret_b = next(ra.get(indices=torch.arange(N_RO * T_RO, device="cuda")))
        with torch.no_grad():
            return float(((ret_b - m(obs_b)[1]) ** 2).mean())

    before = value_loss(ma)
    v_old = pa.value(ra.obs[0]).clone()
    opt = torch.optim.Adam(ma.parameters(), lr=kw["lr"], eps=1e-5)
    stats = ra.update(pa, ma, opt, n_epochs=kw["n_epochs"], batch_size=kw["bs"], clip_range=kw["clip"], ent_coef=kw["ent"],
                      vf_coef=kw["vf"], max_grad_norm=kw["max_norm"], generator=torch.Generator(device="cuda").manual_seed(kw["seed"]))
    assert len(stats) == 8 and all(s.is_cuda and s.shape == (8,) for s in stats)
    _torch_loop(mb, rb, torch.float32, **kw)
    _torch_loop(m64, rb, torch.float64, **kw)
    fig = {}
    p64 = dict(m64.named_parameters())
    for (k, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        drift = float((b.detach().double() - p64[k].detach()).abs().max())
        mine = float((a.detach().double() - p64[k].detach()).abs().max())
        fig[k] = (mine, drift)
    print("ppo-update drift", {k: f"{a:.2e}/{b:.2e}" for k, (a, b) in fig.items()})
    bad = {k: v for k, v in fig.items() if not v[0] <= ppc.MARGIN * v[1]}
    assert not bad, bad
    assert value_loss(ma) < before
    # collect afterwards runs with the new weights
    ra.collect(pa)
    torch.cuda.synchronize()
    assert torch.equal(ra.values[0], pa.value(ra.obs[0]))
    assert not torch.equal(pa.value(ra.obs[0]), pb.value(ra.obs[0])) and not torch.equal(pa.value(rb.obs[0]), v_old)
    for ro, env in ((ra, ea), (rb, eb)):
        ro.close()
        env.close()
