"""The HIP kernels k_ppo_gnorm and k_ppo_adam through pgtg_ppo_step and k_ppo_adv_stats through pgtg_ppo_adv_stats
(include/pgtg.h) against policy_adam_reference / numpy at float64, within four times torch-CPU float32's own
error, and DeviceAdam / Rollout.update with it against the written-out torch loops.

Tolerance (the method of ppo_cases.py).  Truth is policy_adam_reference at float64 from the same float32 inputs; a
tensor's deviation is its largest absolute difference from truth; E_torch is that deviation of torch-CPU float32
(clip_grad_norm_ + Adam) on the same inputs, per tensor and per case, floored at half a float32 ulp of the
tensor's largest magnitude (torch may land on the rounded truth); the kernel may take ppc.MARGIN = 4 of it.  The
same holds for the two advantage statistics against tensor.mean() / .std() on CPU float32.
"""
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
import ppo_cases as ppc
from pgtg_amd import _abi
from pgtg_amd import policy as P

pytestmark = pytest.mark.gpu

SENT = -777.0
BETAS = (0.9, 0.999)
LR = 3e-4
DS = (1, 16, 17, P.K_CHUNK + 1, 1239)
T, N, TOTAL = ppc.T, ppc.N, ppc.TOTAL


def _vec(n, **kw):
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PGTGVecEnv(n, device=0, **kw)


@pytest.fixture(scope="module")
def handle():
    env = _vec(2, random_map_width=3, random_map_height=3)
    yield env
    env.close()


def _half_ulp(x):
    return 0.5 * float(np.spacing(np.float32(np.abs(x).max())))


def _made_up(sd, seed, norm):
    """Normal float32 tensors of the state dict's shapes with a total norm of `norm`."""
    g = torch.Generator().manual_seed(seed)
    out = {k: torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in sd.items()}
    total = math.sqrt(sum(float((x * x).sum()) for x in out.values()))
    return {k: (x * (norm / total)).to(torch.float32).numpy() for k, x in out.items()}


class _State:
    """One (D, step, gradient norm) input set: parameters, gradients and moments as float32 numpy arrays, the
    float64 truth and torch-CPU float32's deviation from it (both computed once)."""

    def __init__(self, D, step, norm, max_norm=0.5, eps=1e-5, zero=False):
        self.D, self.step, self.max_norm, self.eps = D, step, max_norm, eps
        sd = ppc.case(D).sd
        self.p = {k: v.numpy().astype(np.float32) for k, v in sd.items()}
        self.g = _made_up(sd, 7 * D + step, norm)
        if zero:
            self.g = {k: np.zeros_like(x) for k, x in self.g.items()}
        if step > 1:  # moments as a run would have left them: a mean of gradients, a mean of their squares
            self.m = {k: 0.5 * x for k, x in _made_up(sd, 11 * D + step, norm).items()}
            self.v = {k: x * x for k, x in _made_up(sd, 13 * D + step, 2 * norm).items()}
        else:
            self.m = {k: np.zeros_like(x) for k, x in self.p.items()}
            self.v = {k: np.zeros_like(x) for k, x in self.p.items()}
        self.truth = P.policy_adam_reference(self.p, self.g, self.m, self.v, step, LR, BETAS, eps, max_norm)
        self.e_torch = self._torch()

    def _torch(self):
        params = {k: torch.nn.Parameter(torch.as_tensor(x.copy())) for k, x in self.p.items()}
        opt = torch.optim.Adam(params.values(), lr=LR, betas=BETAS, eps=self.eps)
        if self.step > 1:
            sd = opt.state_dict()
            sd["state"] = {i: {"step": torch.tensor(float(self.step - 1)), "exp_avg": torch.as_tensor(self.m[k].copy()),
                               "exp_avg_sq": torch.as_tensor(self.v[k].copy())} for i, k in enumerate(params)}
            opt.load_state_dict(sd)
        for k, p in params.items():
            p.grad = torch.as_tensor(self.g[k].copy())
        total = torch.nn.utils.clip_grad_norm_(params.values(), self.max_norm)
        opt.step()
        st = opt.state_dict()["state"]
        got = ({k: p.detach().numpy() for k, p in params.items()}, {k: st[i]["exp_avg"].numpy() for i, k in enumerate(params)},
               {k: st[i]["exp_avg_sq"].numpy() for i, k in enumerate(params)}, np.float32(total))
        return self.deviations(*got, floor=True)

    def deviations(self, p, m, v, total, floor=False):
        tp, tm, tv, tt = self.truth
        d = {}
        for name, got, want in (("p", p, tp), ("m", m, tm), ("v", v, tv)):
            for k in want:
                e = float(np.abs(got[k].astype(np.float64) - want[k]).max())
                d[f"{name}:{k}"] = max(e, _half_ulp(want[k])) if floor else e
        e = abs(float(total) - float(tt))
        d["grad_norm"] = max(e, _half_ulp(np.float64(tt))) if floor else e
        return d

    def check(self, p, m, v, total, label):
        d = self.deviations(p, m, v, total)
        ratio = {k: d[k] / self.e_torch[k] for k in d}
        worst = sorted(ratio, key=ratio.get)[-3:][::-1]
        print("ppo-step-tolerance", f"D={self.D} step={self.step} {label}",
              {k: f"{d[k]:.2e}/{self.e_torch[k]:.2e}={ratio[k]:.2f}" for k in worst})
        bad = {k: (d[k], self.e_torch[k]) for k in d if not d[k] <= ppc.MARGIN * self.e_torch[k]}
        assert not bad, (label, bad)


def _guarded(arr, pad=1):
    """arr on the device with `pad` sentinel words before and after."""
    t = torch.full((arr.size + 2 * pad,), SENT, dtype=torch.float32, device="cuda")
    t[pad:pad + arr.size] = torch.as_tensor(arr.reshape(-1)).cuda()
    return t


def _call(handle, s, **over):
    """pgtg_ppo_step on the state s with a sentinel word before and after every tensor, the packed buffer (four
    words, for its alignment) and grad_norm, a workspace of NaNs and a packed buffer of 0x7F bytes.  Returns a
    dict: rc, p, m, v, g (after the call), packed (uint32), total, guards intact?, every output untouched?
    over: struct fields to replace; null=(group, field) passes one tensor pointer as NULL."""
    D = s.D
    dev = {name: {k: _guarded(x) for k, x in arrs.items()} for name, arrs in (("p", s.p), ("g", s.g), ("m", s.m), ("v", s.v))}
    nbytes = C.c_uint64()
    assert handle._lib.pgtg_policy_packed_bytes(D, C.byref(nbytes)) == 0
    words = nbytes.value // 4
    packed = torch.full((words + 8,), SENT, dtype=torch.float32, device="cuda")
    packed[4:4 + words].view(torch.uint8).fill_(0x7F)
    packed0 = packed.clone()
    assert handle._lib.pgtg_ppo_step_workspace_bytes(D, C.byref(nbytes)) == 0
    ws = torch.full((nbytes.value // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")
    norm = torch.full((3,), SENT, dtype=torch.float32, device="cuda")
    null = over.pop("null", None)
    raws = {}
    for name, field_name in (("p", "params"), ("g", "grads"), ("m", "exp_avg"), ("v", "exp_avg_sq")):
        raw = _abi.PgtgPpoGrads()
        for field, (key, _) in P.WEIGHT_KEYS.items():
            setattr(raw, field, None if null == (field_name, field) else dev[name][key].data_ptr() + 4)
        raws[field_name] = raw
    fields = dict(obs_dim=D, packed=packed.data_ptr() + 16, workspace=ws.data_ptr(), step=s.step, lr=LR, beta1=BETAS[0],
                  beta2=BETAS[1], eps=s.eps, max_grad_norm=s.max_norm, grad_norm=norm.data_ptr() + 4, **raws)
    fields.update(over)
    handle._bind_stream()
    rc = handle._lib.pgtg_ppo_step(handle._h, C.byref(_abi.PgtgPpoStep(**fields)))
    torch.cuda.synchronize()
    host = {name: {k: t.cpu().numpy() for k, t in d.items()} for name, d in dev.items()}
    ph, nh = packed.cpu().numpy(), norm.cpu().numpy()
    sent = np.float32(SENT)
    guards = all(x[0] == sent and x[-1] == sent for d in host.values() for x in d.values()) \
        and bool((ph[:4] == sent).all() and (ph[-4:] == sent).all()) and nh[0] == sent and nh[2] == sent
    body = lambda name: {k: host[name][k][1:-1].reshape(s.p[k].shape) for k in s.p}  # noqa: E731
    out = dict(rc=rc, p=body("p"), m=body("m"), v=body("v"), g=body("g"), packed=ph[4:-4].view(np.uint32).copy(), total=nh[1],
               guards=guards)
    same = lambda a, b: all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)  # noqa: E731
    out["untouched"] = same(out["p"], s.p) and same(out["m"], s.m) and same(out["v"], s.v) and nh[1] == sent \
        and np.array_equal(ph.view(np.uint32), packed0.cpu().numpy().view(np.uint32))
    out["grads_unchanged"] = same(out["g"], s.g)
    return out


def _repacked(handle, D, params):
    """What pgtg_policy_pack writes from params into a fresh buffer (uint32 words)."""
    pol = P.DevicePolicy(handle, obs_dim=D)
    pol._packed.view(torch.uint8).fill_(0x55)
    pol.load_state_dict({k: torch.as_tensor(x) for k, x in params.items()})
    torch.cuda.synchronize()
    return pol._packed.cpu().numpy().view(np.uint32)


_STATES = {}


def _state(*key, **kw):
    k = key + tuple(sorted(kw.items()))
    if k not in _STATES:
        _STATES[k] = _State(*key, **kw)
    return _STATES[k]


@pytest.mark.parametrize("D", DS)
def test_ppo_step_matches_the_reference(handle, D):
    """Step 1 from zero moments and step 7 from filled ones, each with a total norm above max_grad_norm (3.0: the
    clip scales by about 1/6) and below it (0.2); the packed buffer is the repack of the new parameters bit for
    bit, padding included; the same call again gives the same bits."""
    for step, norm in ((1, 3.0), (1, 0.2), (7, 3.0), (7, 0.2)):
        s = _state(D, step, norm)
        assert (float(s.truth[3]) > s.max_norm) == (norm > s.max_norm)
        r = _call(handle, s)
        assert r["rc"] == 0 and r["guards"] and r["grads_unchanged"], (step, norm)
        s.check(r["p"], r["m"], r["v"], r["total"], f"norm={norm}")
        assert np.array_equal(r["packed"], _repacked(handle, D, r["p"])), (step, norm)
        again = _call(handle, s)
        for name in ("p", "m", "v"):
            assert all(np.array_equal(r[name][k].view(np.uint32), again[name][k].view(np.uint32)) for k in s.p), name
        assert np.array_equal(r["packed"], again["packed"]) and r["total"].tobytes() == again["total"].tobytes()


def test_edges(handle):
    D = 17
    # all-zero gradients and zero moments: nothing moves, nothing is NaN, the packed buffer is the repack
    s = _state(D, 1, 1.0, zero=True)
    r = _call(handle, s)
    assert r["rc"] == 0 and r["guards"] and r["total"] == 0
    for k in s.p:
        assert np.array_equal(r["p"][k].view(np.uint32), s.p[k].view(np.uint32)), k
        assert not r["m"][k].any() and not r["v"][k].any()
    assert np.array_equal(r["packed"], _repacked(handle, D, s.p))
    # max_grad_norm = inf: the unclipped reference
    s = _state(D, 7, 3.0, max_norm=math.inf)
    r = _call(handle, s)
    assert r["rc"] == 0 and r["guards"]
    s.check(r["p"], r["m"], r["v"], r["total"], "max_grad_norm=inf")
    clipped = _state(D, 7, 3.0)
    assert not np.array_equal(r["p"]["action_net.weight"], _call(handle, clipped)["p"]["action_net.weight"])
    # grad_norm is optional, and eps = 1e-8 (torch's default) is another divisor
    r0 = _call(handle, clipped, grad_norm=None)
    assert r0["rc"] == 0 and r0["guards"] and r0["total"] == np.float32(SENT)
    s8 = _state(D, 7, 0.2, eps=1e-8)
    r8 = _call(handle, s8)
    assert r8["rc"] == 0 and r8["guards"]
    s8.check(r8["p"], r8["m"], r8["v"], r8["total"], "eps=1e-8")


def test_refusals_launch_nothing(handle):
    s = _state(17, 7, 3.0)
    dummy = torch.zeros(64, device="cuda")
    cases = [(dict(null=("params", "w1p")), "twelve"), (dict(null=("grads", "bv")), "twelve"),
             (dict(null=("exp_avg", "wa")), "twelve"), (dict(null=("exp_avg_sq", "b2v")), "twelve"),
             (dict(packed=None), "required"), (dict(workspace=None), "required"),
             (dict(packed=dummy.data_ptr() + 4), "aligned"), (dict(workspace=dummy.data_ptr() + 4), "aligned"),
             (dict(obs_dim=0), "obs_dim"), (dict(obs_dim=_abi.PGTG_POLICY_MAX_OBS_DIM + 1), "obs_dim"),
             (dict(step=0), "step"), (dict(lr=math.nan), "finite"), (dict(lr=math.inf), "finite"), (dict(eps=math.nan), "finite"),
             (dict(beta1=math.nan), "finite"), (dict(beta2=math.inf), "finite"), (dict(beta1=1.0), "[0, 1)"),
             (dict(beta2=-0.5), "[0, 1)"), (dict(max_grad_norm=math.nan), "max_grad_norm"),
             (dict(max_grad_norm=0.0), "max_grad_norm"), (dict(max_grad_norm=-1.0), "max_grad_norm")]
    for over, word in cases:
        r = _call(handle, s, **dict(over))
        msg = handle._lib.pgtg_last_error(handle._h).decode()
        assert r["rc"] == _abi.PGTG_E_INVALID and msg.startswith("pgtg_ppo_step") and word in msg, (over, r["rc"], msg)
        assert r["guards"] and r["untouched"] and r["grads_unchanged"], over
    assert not dummy.any()


# ---- pgtg_ppo_adv_stats ------------------------------------------------------------------------------

def _adv_call(handle, adv_dev, idx, batch=None, **over):
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64).cuda()
    out = torch.full((4,), SENT, dtype=torch.float32, device="cuda")
    args = dict(advantages=adv_dev.data_ptr(), indices=idx.data_ptr(), batch=idx.numel() if batch is None else batch, steps=T, n=N,
                out=out.data_ptr() + 4)
    args.update(over)
    handle._bind_stream()
    rc = handle._lib.pgtg_ppo_adv_stats(handle._h, *(args[k] for k in ("advantages", "indices", "batch", "steps", "n", "out")))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return rc, o[1:3], o[0] == np.float32(SENT) and o[3] == np.float32(SENT)


def _adv_check(got, a32, label):
    """got {mean, 1 / (std + 1e-8)} against numpy float64 over the gathered float32 advantages a32."""
    a = a32.astype(np.float64)
    want = np.array([a.mean(), 1.0 / (a.std(ddof=1) + 1e-8)])
    t = torch.as_tensor(a32)
    tor = np.array([float(t.mean()), float(1.0 / (t.std() + 1e-8))])
    e = np.maximum(np.abs(tor - want), [_half_ulp(want[0]), _half_ulp(want[1])])
    d = np.abs(got.astype(np.float64) - want)
    print("ppo-step-tolerance adv_stats", label, {n: f"{d[i]:.2e}/{e[i]:.2e}={d[i] / e[i]:.2f}" for i, n in enumerate(("mean", "inv_std"))})
    assert (d <= ppc.MARGIN * e).all(), (label, d, e)


def test_adv_stats(handle):
    c = ppc.case(29)
    adv = torch.as_tensor(c.advantages).cuda().contiguous()
    gather = lambda idx: c.advantages[np.asarray(idx) % T, np.asarray(idx) // T]  # noqa: E731
    for B in (2, 63, 64, 65, 257, 3333):  # (3 333: past T * N the indices repeat; more than one round of the workgroup)
        idx = c.indices(B)
        rc, got, guards = _adv_call(handle, adv, idx)
        assert rc == 0 and guards, B
        _adv_check(got, gather(idx), f"B={B}")
        rc, again, _ = _adv_call(handle, adv, idx)
        assert got.tobytes() == again.tobytes(), B
    idx = np.tile(c.perm[:40], 3)  # repeats
    rc, got, guards = _adv_call(handle, adv, idx)
    assert rc == 0 and guards
    _adv_check(got, gather(idx), "repeats")
    good = c.indices(64)  # one index out of range (and one negative): advantages of 0
    idx = np.concatenate([good[:10], [TOTAL], good[10:], [-1]])
    rc, got, guards = _adv_call(handle, adv, idx)
    assert rc == 0 and guards
    a = np.concatenate([gather(good[:10]), [0.0], gather(good[10:]), [0.0]]).astype(np.float32)
    _adv_check(got, a, "out of range")
    # refusals: a batch of one (SB3 does not normalise it), NULL pointers, empty or overflowing shapes
    for over, word in ((dict(batch=1), "batch"), (dict(batch=0), "batch"), (dict(advantages=None), "required"),
                       (dict(indices=None), "required"), (dict(out=None), "required"), (dict(steps=0), "steps"), (dict(n=0), "steps"),
                       (dict(steps=1 << 62, n=1 << 62), "overflow")):
        rc, got, guards = _adv_call(handle, adv, good, **over)
        msg = handle._lib.pgtg_last_error(handle._h).decode()
        assert rc == _abi.PGTG_E_INVALID and msg.startswith("pgtg_ppo_adv_stats") and word in msg, (over, rc, msg)
        assert guards and (got == np.float32(SENT)).all(), over


# ---- DeviceAdam and Rollout.update ----------------------------------------------------------------------

TRAIN = dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=0.2,
             random_map_percentage_of_connections=0.8, traffic_density=0.2, conservative_driver_percentage=0.15,
             normal_driver_percentage=0.50, aggressive_driver_percentage=0.20, elderly_driver_percentage=0.10,
             reckless_driver_percentage=0.05, sliding_observation_window_size=5, max_allowed_deviation=15,
             use_sliding_observation_window=True, use_next_subgoal_direction=True, final_goal_bonus=200,
             standing_still_penalty=1)
N_RO, T_RO, LIMIT = 96, 5, 3


def _collected(seed_module=4):
    """test_gpu_ppo.py's fixture: a collected rollout of 96 envs x 5 steps under a module with sharpened logits."""
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


def test_device_adam_state_round_trip(handle):
    D = 29
    sd = ppc.case(D).sd
    module = P.MlpPolicyReference(D).cuda()
    module.load_state_dict(sd)
    pol = P.DevicePolicy(handle, obs_dim=D)
    pol.load_state_dict(module.state_dict())
    opt = P.DeviceAdam(pol, module, lr=1e-3)
    gs = [{k: torch.as_tensor(x).cuda() for k, x in _made_up(sd, 50 + i, n).items()} for i, n in enumerate((3.0, 0.2, 1.0))]
    for g in gs[:2]:
        opt.step(grads=g, max_grad_norm=0.5)
    assert opt.step_count == 2 and opt.last_grad_norm.is_cuda
    assert abs(float(opt.last_grad_norm) - 0.2) < 1e-6
    state = opt.state_dict()
    assert all(isinstance(s["step"], int) and s["step"] == 2 for s in state["state"].values())
    # the third step by torch from the exported state, by the kernel, and at float64
    twin = P.MlpPolicyReference(D).cuda()
    twin.load_state_dict(module.state_dict())
    topt = torch.optim.Adam(twin.parameters(), lr=5.0, eps=1e-3)  # (the loaded state overrides these)
    topt.load_state_dict(state)
    assert topt.param_groups[0]["lr"] == 1e-3 and topt.param_groups[0]["eps"] == 1e-5
    host = lambda d: {k: v.detach().cpu().numpy() for k, v in d.items()}  # noqa: E731
    truth = P.policy_adam_reference(host(dict(module.named_parameters())), host(gs[2]), host(opt.exp_avg), host(opt.exp_avg_sq),
                                    3, 1e-3, BETAS, 1e-5, 0.5)
    for k, p in twin.named_parameters():
        p.grad = gs[2][k].clone()
    torch.nn.utils.clip_grad_norm_(twin.parameters(), 0.5)
    topt.step()
    opt.step(grads=gs[2], max_grad_norm=0.5)
    torch.cuda.synchronize()
    tst = topt.state_dict()["state"]
    keys = [k for k, _ in module.named_parameters()]
    for name, mine, theirs, want in (("p", host(dict(module.named_parameters())), host(dict(twin.named_parameters())), truth[0]),
                                     ("m", host(opt.exp_avg), {k: tst[i]["exp_avg"].cpu().numpy() for i, k in enumerate(keys)}, truth[1]),
                                     ("v", host(opt.exp_avg_sq), {k: tst[i]["exp_avg_sq"].cpu().numpy() for i, k in enumerate(keys)}, truth[2])):
        for k in keys:
            e = max(float(np.abs(theirs[k] - want[k]).max()), _half_ulp(want[k]))
            d = float(np.abs(mine[k] - want[k]).max())
            assert d <= ppc.MARGIN * e, (name, k, d, e)
    # and back: the torch optimiser's state (step a tensor) into a fresh DeviceAdam
    back = P.DeviceAdam(pol, module)
    back.load_state_dict(topt.state_dict())
    assert back.step_count == 3 and back.lr == 1e-3 and back.eps == 1e-5
    assert all(torch.equal(back.exp_avg[k], tst[i]["exp_avg"]) for i, k in enumerate(keys))
    # the packed buffer follows the module without a load_state_dict
    assert np.array_equal(pol._packed.cpu().numpy().view(np.uint32), _repacked(handle, D, host(dict(module.named_parameters()))))
    with pytest.raises(ValueError, match="mlp_extractor.policy_net.0.weight"):
        P.DeviceAdam(pol, P.MlpPolicyReference(D).cuda().double())
    with pytest.raises(ValueError):
        P.DeviceAdam(pol, P.MlpPolicyReference(D))  # on the host


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


def test_rollout_update_with_device_adam(monkeypatch):
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
    opt = P.DeviceAdam(pa, ma, lr=kw["lr"], eps=1e-5)
    calls = []
    real_load = pa.load_state_dict
    monkeypatch.setattr(pa, "load_state_dict", lambda sd: (calls.append(1), real_load(sd))[1])
    made = []
    real_init = torch.optim.Optimizer.__init__
    monkeypatch.setattr(torch.optim.Optimizer, "__init__", lambda self, *a, **k: (made.append(type(self)), real_init(self, *a, **k))[1])
    clips = []
    real_clip = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: (clips.append(1), real_clip(*a, **k))[1])
    stats = ra.update(pa, ma, opt, n_epochs=kw["n_epochs"], batch_size=kw["bs"], clip_range=kw["clip"], ent_coef=kw["ent"],
                      vf_coef=kw["vf"], max_grad_norm=kw["max_norm"], generator=torch.Generator(device="cuda").manual_seed(kw["seed"]))
    monkeypatch.undo()
    assert not calls and not made and not clips  # no repack by load_state_dict, no torch optimiser, no torch clip
    assert opt.step_count == 8
    assert len(stats) == 8 and all(s.is_cuda and s.shape == (8,) for s in stats)
    _torch_loop(mb, rb, torch.float32, **kw)
    _torch_loop(m64, rb, torch.float64, **kw)
    fig = {}
    p64 = dict(m64.named_parameters())
    for (k, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        drift = float((b.detach().double() - p64[k].detach()).abs().max())
        mine = float((a.detach().double() - p64[k].detach()).abs().max())
        fig[k] = (mine, drift)
    print("ppo-step-tolerance update drift", {k: f"{a:.2e}/{b:.2e}={a / b if b else float('nan'):.2f}" for k, (a, b) in fig.items()})
    bad = {k: v for k, v in fig.items() if not v[0] <= ppc.MARGIN * v[1]}
    assert not bad, bad
    assert value_loss(ma) < before
    # collect afterwards runs with the new weights, which reached the packed buffer without a load_state_dict
    ra.collect(pa)
    torch.cuda.synchronize()
    assert torch.equal(ra.values[0], pa.value(ra.obs[0]))
    assert not torch.equal(pa.value(ra.obs[0]), pb.value(ra.obs[0])) and not torch.equal(pa.value(rb.obs[0]), v_old)
    # a DeviceAdam of another policy is refused
    with pytest.raises(ValueError):
        rb.update(pb, mb, opt, n_epochs=1, batch_size=120)
    for ro, env in ((ra, ea), (rb, eb)):
        ro.close()
        env.close()
