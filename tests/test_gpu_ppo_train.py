"""PPO.train in full on the device: value clipping in k_ppo_loss (pgtg_ppo_grad_ex), the target_kl gate through
every kernel of a minibatch, the log (k_ppo_expl_var, k_ppo_log) and the permutation (k_ppo_perm), through the C
ABI on ppo_cases' made-up rollouts and through Rollout.update / train_log on a collected rollout of 48 envs x 5
steps (240 samples in minibatches of 100, 100 and 40: the last 64-sample block is partial).

Tolerance of the clipped gradient: ppo_cases' (deviations in units of the accumulated magnitudes, MARGIN = 4 x
E_torch), with E_torch re-measured for the clipped loss from torch-CPU float32 autograd (ppo_train_cases.e_torch).
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
import ppo_cases as ppc
import ppo_train_cases as ptc
from pgtg_amd import _abi
from pgtg_amd import policy as P
from pgtg_amd import rollout as R

pytestmark = pytest.mark.gpu

SENT = -777.0
T, N, TOTAL = ppc.T, ppc.N, ppc.TOTAL
TOTALS = (1, 2, 3, 240, 255, 256, 257, 4099, 65537)


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


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


# ---- value clipping through pgtg_ppo_grad_ex ----------------------------------------------------------------

class _Dev:
    """ppc.case(D)'s rollout and the old values of ppo_train_cases on the device (rows ppc.pitch(D) apart)."""

    def __init__(self, handle, D):
        self.c = c = ppc.case(D)
        self.D, self.pitch = D, ppc.pitch(D)
        self.pol = P.DevicePolicy(handle, obs_dim=D, seed=9)
        self.pol.load_state_dict(c.sd)
        cu = lambda x: torch.as_tensor(x).cuda().contiguous()  # noqa: E731
        self.actions, self.old, self.adv, self.ret = cu(c.actions), cu(c.old_log_probs), cu(c.advantages), cu(c.returns)
        self.old_values = cu(ptc.old_values(D))
        n = (T - 1) * self.pitch + N * D
        self.store = torch.full((n,), 0x7F, dtype=torch.int8, device="cuda")
        self.obs = self.store.as_strided((T, N, D), (self.pitch, D, 1))
        self.obs.copy_(torch.as_tensor(c.obs))


_DEVS = {}


def _dev(handle, D):
    if D not in _DEVS:
        _DEVS[D] = _Dev(handle, D)
    return _DEVS[D]


def _grad(handle, dv, idx, norm, ent, extra="none", **over):
    """pgtg_ppo_grad (extra="none") or pgtg_ppo_grad_ex with the PgtgPpoExtra given (None: a NULL pointer), a
    sentinel word before and after every output.  Returns (rc, grads, stats [8], guards intact?, all untouched?)."""
    D = dv.D
    idx = torch.as_tensor(idx, dtype=torch.int64).cuda()
    B = idx.numel()
    outs = {key: torch.full((int(np.prod(shape)) + 2,), SENT, device="cuda") for key, shape in P.weight_shapes(D).items()}
    outs["stats"] = torch.full((8 + 2,), SENT, device="cuda")
    raw = _abi.PgtgPpoGrads()
    for field, (key, _) in P.WEIGHT_KEYS.items():
        setattr(raw, field, outs[key].data_ptr() + 4)
    nbytes = C.c_uint64()
    assert handle._lib.pgtg_ppo_workspace_bytes(D, max(B, 1), C.byref(nbytes)) == 0
    ws = torch.full((nbytes.value // 4 + 8,), float("nan"), device="cuda")
    adv_stats = None
    if norm and B > 1:
        a = dv.adv[idx % T, idx // T]
        adv_stats = torch.stack((a.mean(), 1.0 / (a.std() + 1e-8)))
    fields = dict(batch=B, obs_dim=D, steps=T, n=N, obs_pitch=dv.pitch, obs=_ptr(dv.obs), indices=_ptr(idx),
                  actions=_ptr(dv.actions), log_probs=_ptr(dv.old), advantages=_ptr(dv.adv), returns=_ptr(dv.ret),
                  packed=_ptr(dv.pol._packed), adv_stats=_ptr(adv_stats), clip_range=ppc.CLIP, ent_coef=ent, vf_coef=ppc.VF,
                  workspace=_ptr(ws), grads=raw, stats=C.c_void_p(outs["stats"].data_ptr() + 4))
    fields.update(over)
    a = _abi.PgtgPpoGrad(**fields)
    handle._bind_stream()
    if isinstance(extra, str):
        rc = handle._lib.pgtg_ppo_grad(handle._h, C.byref(a))
    else:
        rc = handle._lib.pgtg_ppo_grad_ex(handle._h, C.byref(a), None if extra is None else C.byref(extra))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    guards = all(v[0] == np.float32(SENT) and v[-1] == np.float32(SENT) for v in host.values())
    untouched = all(bool((v == np.float32(SENT)).all()) for v in host.values())
    grads = {k: host[k][1:-1].reshape(s) for k, s in P.weight_shapes(D).items()}
    return rc, grads, host["stats"][1:-1], guards, untouched


def _clip_extra(dv, c=ptc.CLIP_VF, **kw):
    return _abi.PgtgPpoExtra(flags=_abi.PGTG_PPO_CLIP_VF, old_values=dv.old_values.data_ptr(), clip_range_vf=c, **kw)


def _same_bits(a, b):
    (ga, sa), (gb, sb) = a, b
    bad = [k for k in ga if not np.array_equal(ga[k].view(np.uint32), gb[k].view(np.uint32))]
    if not np.array_equal(sa.view(np.uint32), sb.view(np.uint32)):
        bad.append(("stats", sa.tolist(), sb.tolist()))
    if bad:
        print("differing bits:", bad)
    return not bad


@pytest.mark.parametrize("D", ppc.FULL_DS)
def test_value_clip_matches_the_reference(handle, D):
    """Every gradient and statistic of the clipped loss within MARGIN x E_torch of ppo_reference at float64."""
    dv = _dev(handle, D)
    e = ptc.e_torch(D)
    print("ppo-train E_torch (clipped loss)", D, {k: f"{v:.2e}" for k, v in e.items()})
    for B in ptc.BS:
        idx = dv.c.indices(B)
        for norm, ent in ppc.CONFIGS:
            rc, g, s, guards, _ = _grad(handle, dv, idx, norm, ent, extra=_clip_extra(dv))
            assert rc == 0 and guards, (B, norm, ent)
            dv.c.check(g, s, ptc.reference(D, B, norm, ent), f"clip_vf B={B} D={D} norm={norm} ent={ent}", e_torch=e)
    # the clip changes the value tower alone, and a second call gives the same bits
    idx = dv.c.indices(257)
    _, g0, s0, _, _ = _grad(handle, dv, idx, True, 0.01)
    _, g1, s1, _, _ = _grad(handle, dv, idx, True, 0.01, extra=_clip_extra(dv))
    _, g2, s2, _, _ = _grad(handle, dv, idx, True, 0.01, extra=_clip_extra(dv))
    assert _same_bits((g1, s1), (g2, s2))
    for k in ppc.KEYS:
        assert np.array_equal(g0[k].view(np.uint32), g1[k].view(np.uint32)) == ("value_net" not in k), k
    assert all(s0[i] == s1[i] for i in (1, 3, 4, 5)) and s0[2] != s1[2] and s0[0] != s1[0]
    # a clip range nothing reaches computes the unclipped loss (same statistics bit for bit; the value tower's
    # gradients come from the kernel's other branch, whose compilation may round a product the other way, so
    # they are held to the unclipped reference at the tolerance, not to the unclipped call's bits: on an MI355X
    # they differ from it by one float32 ulp), and one of zero leaves no value gradient
    _, g3, s3, _, _ = _grad(handle, dv, idx, True, 0.01, extra=_clip_extra(dv, c=1e30))
    assert np.array_equal(s0.view(np.uint32), s3.view(np.uint32))
    dv.c.check(g3, s3, dv.c.reference(257, True, 0.01), f"clip_vf=1e30 D={D} against the unclipped reference", e_torch=e)
    _, g4, _, _, _ = _grad(handle, dv, idx, True, 0.01, extra=_clip_extra(dv, c=0.0))
    assert all(not g4[k].any() for k in ppc.KEYS if "value_net" in k)


@pytest.mark.parametrize("D", ppc.FULL_DS)
def test_an_empty_extra_is_pgtg_ppo_grad(handle, D):
    dv = _dev(handle, D)
    for B in (65, 257):
        idx = dv.c.indices(B)
        rc, g, s, guards, _ = _grad(handle, dv, idx, True, 0.01)
        assert rc == 0 and guards
        stop = torch.zeros(1, dtype=torch.int32, device="cuda")
        for extra in (None, _abi.PgtgPpoExtra(), _abi.PgtgPpoExtra(old_values=dv.old_values.data_ptr(), clip_range_vf=0.1),
                      _abi.PgtgPpoExtra(stop_at=stop.data_ptr(), ordinal=1)):
            rc, ge, se, guards, _ = _grad(handle, dv, idx, True, 0.01, extra=extra)
            assert rc == 0 and guards and _same_bits((g, s), (ge, se)), B
        assert int(stop) == 0


def test_refusals_launch_nothing(handle):
    dv = _dev(handle, 29)
    idx = dv.c.indices(65)
    stop = torch.zeros(2, dtype=torch.int32, device="cuda")
    ov, sp = dv.old_values.data_ptr(), stop.data_ptr()
    X, CV, KL = _abi.PgtgPpoExtra, _abi.PGTG_PPO_CLIP_VF, _abi.PGTG_PPO_TARGET_KL
    cases = [(X(flags=CV, old_values=ov, clip_range_vf=-0.1), "clip_range_vf"), (X(flags=CV, old_values=ov, clip_range_vf=float("nan")), "clip_range_vf"),
             (X(flags=CV, old_values=ov, clip_range_vf=float("inf")), "clip_range_vf"), (X(flags=CV, clip_range_vf=0.2), "old_values"),
             (X(flags=KL, stop_at=sp, ordinal=1, target_kl=-1.0), "target_kl"), (X(flags=KL, stop_at=sp, ordinal=1, target_kl=float("nan")), "target_kl"),
             (X(flags=KL, stop_at=sp, ordinal=1, target_kl=float("inf")), "target_kl"), (X(flags=KL, ordinal=1, target_kl=0.01), "stop_at"),
             (X(stop_at=sp, ordinal=0), "ordinal"), (X(stop_at=sp + 2, ordinal=1), "aligned"), (X(flags=4), "flags")]
    for extra, word in cases:
        rc, _, _, guards, untouched = _grad(handle, dv, idx, True, 0.0, extra=extra)
        msg = handle._lib.pgtg_last_error(handle._h).decode()
        assert rc == _abi.PGTG_E_INVALID and msg.startswith("pgtg_ppo_grad_ex") and word in msg, (word, rc, msg)
        assert guards and untouched, word
    assert not stop.any()
    # pgtg_ppo_log: a statistics buffer off its 16-byte alignment, no per_epoch, NULL pointers
    stats = torch.zeros(4 * 8 + 4, device="cuda")
    out = torch.full((C.sizeof(_abi.PgtgPpoLog) // 4,), SENT, device="cuda")
    for args, word in (((stats.data_ptr() + 4, 4, 2, None, None, out.data_ptr()), "16-byte"),
                       ((stats.data_ptr(), 4, 0, None, None, out.data_ptr()), "per_epoch"),
                       ((None, 4, 2, None, None, out.data_ptr()), "required"), ((stats.data_ptr(), 4, 2, None, None, None), "required"),
                       ((stats.data_ptr(), 4, 2, sp + 1, None, out.data_ptr()), "4-byte")):
        rc = handle._lib.pgtg_ppo_log(handle._h, *args)
        msg = handle._lib.pgtg_last_error(handle._h).decode()
        assert rc == _abi.PGTG_E_INVALID and msg.startswith("pgtg_ppo_log") and word in msg, (word, rc, msg)
    perm = torch.full((8,), -5, dtype=torch.int64, device="cuda")
    assert handle._lib.pgtg_ppo_perm(handle._h, 0, 1, 0, perm.data_ptr()) == _abi.PGTG_E_INVALID
    assert handle._lib.pgtg_ppo_perm(handle._h, 4, 1, 0, perm.data_ptr() + 4) == _abi.PGTG_E_INVALID
    assert handle._lib.pgtg_ppo_perm(handle._h, 4, 1, 0, None) == _abi.PGTG_E_INVALID
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((perm == -5).all())


# ---- the explained variance and the permutation through the C ABI ----------------------------------------------

def _expl_var(handle, values, returns):
    v, r = torch.as_tensor(values).cuda().contiguous(), torch.as_tensor(returns).cuda().contiguous()
    nbytes = C.c_uint64()
    assert handle._lib.pgtg_ppo_expl_var_workspace_bytes(C.byref(nbytes)) == 0
    ws = torch.full((nbytes.value // 8,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((4,), SENT, device="cuda")
    handle._bind_stream()
    rc = handle._lib.pgtg_ppo_expl_var(handle._h, _ptr(v), _ptr(r), v.numel(), _ptr(ws), C.c_void_p(out.data_ptr() + 4))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert rc == 0 and o[0] == np.float32(SENT) and o[3] == np.float32(SENT)
    return o[1:3].copy()


@pytest.mark.parametrize("shape", [(1, 1), (3, 96), (5, 48), (7, 1000)])
def test_explained_variance(handle, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    y = (3.0 + 2.0 * rng.standard_normal(shape)).astype(np.float32)
    p = (y + 0.5 * rng.standard_normal(shape)).astype(np.float32)
    got = _expl_var(handle, p, y)
    if y.size == 1:
        assert np.isnan(got).all()  # (one return: var(returns) == 0)
    else:
        y64, p64 = y.astype(np.float64), p.astype(np.float64)
        want = np.var(y64 - p64) / np.var(y64)
        print("ppo-train expl_var", shape, float(got[1]), want, abs(float(got[1]) - want) / want)
        assert abs(float(got[1]) - want) <= 5e-7 * want
        assert abs(float(got[0]) - (1.0 - want)) <= 5e-7 * want + float(np.spacing(np.float32(abs(1.0 - want))))
        assert _expl_var(handle, p, y).tobytes() == got.tobytes()
    same = _expl_var(handle, y, y)
    if y.size == 1:
        assert np.isnan(same).all()
    else:
        assert same[0] == 1.0 and same[1] == 0.0
    assert np.isnan(_expl_var(handle, p, np.full(shape, 2.5, dtype=np.float32))).all()


@pytest.mark.parametrize("total", TOTALS)
def test_the_permutation_kernel_is_the_reference(handle, total):
    for seed, counter in ((7, 0), (7, 5), ((1 << 63) + 12345, (1 << 40) + 3)):
        perm = torch.full((total + 2,), -5, dtype=torch.int64, device="cuda")
        handle._bind_stream()
        rc = handle._lib.pgtg_ppo_perm(handle._h, total, seed, counter, C.c_void_p(perm.data_ptr() + 8))
        torch.cuda.synchronize()
        got = perm.cpu().numpy()
        assert rc == 0 and got[0] == -5 and got[-1] == -5
        assert np.array_equal(got[1:-1], R.permutation_reference(total, seed, counter)), (seed, counter)
    assert handle.error_count()[0] == 0


# ---- the gate, target_kl, the log and perm_seed through DevicePolicy, DeviceAdam and Rollout.update ------------

N_RO, T_RO, BATCH, EPOCHS, LR, SEED = 48, 5, 100, 3, 2e-3, 11
PER_EPOCH = 3
M_ALL = EPOCHS * PER_EPOCH
KW = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5)


class _Run:
    """A collected rollout of 48 envs x 5 steps on a 3 x 3 map, its module, policy and DeviceAdam, and the state to
    return to between updates."""

    def __init__(self):
        from pgtg_amd.flat import flat_dim
        self.env = _vec(N_RO, autoreset=True, max_episode_steps=3, random_map_width=3, random_map_height=3)
        self.D = flat_dim(self.env.spec)
        torch.manual_seed(4)
        self.module = P.MlpPolicyReference(self.D).cuda()
        with torch.no_grad():
            self.module.action_net.weight.mul_(100.0)
        self.pol = P.DevicePolicy(self.env, seed=21)
        self.pol.load_state_dict(self.module.state_dict())
        self.ro = self.env.rollout(T_RO)
        self.ro.begin(seed=7)
        self.ro.collect(self.pol)
        self.opt = P.DeviceAdam(self.pol, self.module, lr=LR, eps=1e-5)
        torch.cuda.synchronize()
        self.sd0 = {k: v.clone() for k, v in self.module.state_dict().items()}
        self.packed0 = self.pol._packed.clone()

    def restore(self):
        with torch.no_grad():
            for k, p in self.module.named_parameters():
                p.copy_(self.sd0[k])
                self.opt.exp_avg[k].zero_()
                self.opt.exp_avg_sq[k].zero_()
        self.pol._packed.copy_(self.packed0)
        self.opt.step_count = 0
        self.ro._updates = 0
        self.ro.n_updates = 0

    def state(self):
        """Every byte an update may change: parameters, both moments, the packed buffer; and the step count."""
        torch.cuda.synchronize()
        out = {f"p:{k}": p.detach().cpu().numpy().copy() for k, p in self.module.named_parameters()}
        out.update({f"m:{k}": v.cpu().numpy().copy() for k, v in self.opt.exp_avg.items()})
        out.update({f"v:{k}": v.cpu().numpy().copy() for k, v in self.opt.exp_avg_sq.items()})
        out["packed"] = self.pol._packed.cpu().numpy().copy()
        return out, self.opt.step_count

    def minibatches(self):
        """(ordinal m, index tensor) of the update's minibatches under perm_seed = SEED, first update."""
        m = 0
        for k in range(EPOCHS):
            perm = torch.as_tensor(R.permutation_reference(N_RO * T_RO, SEED, k)).cuda()
            for lo in range(0, N_RO * T_RO, BATCH):
                m += 1
                yield m, perm[lo:lo + BATCH]

    def first(self, count):
        """The update written out, ungated, over the first `count` minibatches."""
        grads = {k: torch.zeros_like(p) for k, p in self.module.named_parameters()}
        for m, idx in self.minibatches():
            if m > count:
                break
            st = self.pol.adv_stats(self.ro, idx)
            self.pol.ppo_grad(self.ro, idx, grads=grads, adv_stats=st, clip_range=KW["clip_range"], ent_coef=KW["ent_coef"],
                              vf_coef=KW["vf_coef"])
            self.opt.step(grads=grads, max_grad_norm=KW["max_grad_norm"])

    def host_loop(self, dtype):
        """SB3's loop on the host at dtype over the same permutations: every minibatch's approx_kl."""
        ro = self.ro
        m = P.MlpPolicyReference(self.D).to(dtype)
        m.load_state_dict({k: v.cpu().to(dtype) for k, v in self.sd0.items()})
        opt = torch.optim.Adam(m.parameters(), lr=LR, eps=1e-5)
        h = lambda x: x.cpu()  # noqa: E731
        obs, act, lp, adv, ret = h(ro.obs[:T_RO]), h(ro.actions), h(ro.log_probs), h(ro.advantages), h(ro.returns)
        kls = []
        for _, idx in self.minibatches():
            idx = idx.cpu()
            e, t = idx // T_RO, idx % T_RO
            loss, stats = ppc.torch_ppo(m, obs[t, e].to(dtype), act[t, e], lp[t, e].to(dtype), adv[t, e].to(dtype),
                                        ret[t, e].to(dtype), KW["clip_range"], KW["ent_coef"], KW["vf_coef"], True)
            kls.append(float(stats[4]))
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), KW["max_grad_norm"])
            opt.step()
        return np.array(kls)


@pytest.fixture(scope="module")
def run():
    r = _Run()
    yield r
    r.ro.close()
    r.env.close()


def _equal_states(a, b):
    (sa, ca), (sb, cb) = a, b
    bad = [k for k in sa if sa[k].tobytes() != sb[k].tobytes()]
    return not bad and ca == cb, (bad, ca, cb)


def test_the_gate_directed(run):
    """stop_at = m preset: ordinal m - 1 runs everything, ordinal m writes its gradients and stats and takes no
    step, ordinal m + 1 changes no byte anywhere."""
    r = run
    r.restore()
    idx = next(iter(r.minibatches()))[1]
    m = 5
    stop = torch.full((1,), m, dtype=torch.int32, device="cuda")
    sent = lambda: {k: torch.full_like(p, SENT) for k, p in r.module.named_parameters()}  # noqa: E731

    def launch(ordinal, gated=True):
        gate = dict(stop_at=stop, ordinal=ordinal) if gated else {}
        grads, stats, adv, norm0 = sent(), torch.full((8,), SENT, device="cuda"), torch.full((2,), SENT, device="cuda"), None
        r.opt.last_grad_norm.fill_(SENT)
        r.pol.adv_stats(r.ro, idx, out=adv, **gate)
        r.pol.ppo_grad(r.ro, idx, grads=grads, adv_stats=adv, stats_out=stats, ent_coef=0.01, **gate)
        r.opt.step(grads=grads, max_grad_norm=0.5, **gate)
        torch.cuda.synchronize()
        return ({k: g.cpu().numpy() for k, g in grads.items()}, stats.cpu().numpy(), adv.cpu().numpy(),
                float(r.opt.last_grad_norm))

    before = r.state()[0]
    plain = launch(1, gated=False)          # the ungated minibatch from the same state
    after_plain = r.state()[0]
    assert any(before[k].tobytes() != after_plain[k].tobytes() for k in before)
    r.restore()
    low = launch(m - 1)                     # everything runs
    after_low = r.state()[0]
    assert all(after_low[k].tobytes() == after_plain[k].tobytes() for k in before)
    assert all(low[0][k].tobytes() == plain[0][k].tobytes() for k in plain[0]) and low[1].tobytes() == plain[1].tobytes()
    assert low[3] == plain[3] != SENT
    r.restore()
    at = launch(m)                          # gradients and stats, no step
    after_at = r.state()[0]
    assert all(after_at[k].tobytes() == before[k].tobytes() for k in before)
    assert all(at[0][k].tobytes() == plain[0][k].tobytes() for k in plain[0]) and at[1].tobytes() == plain[1].tobytes()
    assert at[2].tobytes() == plain[2].tobytes() and at[3] == SENT
    above = launch(m + 1)                   # nothing at all
    after_above = r.state()[0]
    assert all(after_above[k].tobytes() == before[k].tobytes() for k in before)
    assert all(bool((g == np.float32(SENT)).all()) for g in above[0].values())
    assert bool((above[1] == np.float32(SENT)).all()) and bool((above[2] == np.float32(SENT)).all()) and above[3] == SENT
    assert int(stop) == m
    r.opt.step_count = 0


@pytest.fixture(scope="module")
def kls(run):
    """approx_kl of every minibatch from the float64 host loop, and torch float32's largest deviation from it."""
    k64, k32 = run.host_loop(torch.float64), run.host_loop(torch.float32)
    e = max(float(np.abs(k64 - k32).max()), float(np.spacing(np.float32(k64.max()))))
    print("ppo-train approx_kl per minibatch (float64)", [f"{x:.3e}" for x in k64], "E_torch", f"{e:.2e}")
    return k64, e


def _target(k64, e, stop_at):
    """A target_kl under which the update stops at minibatch stop_at (None: never), with 1.5 target_kl at least
    10 E_torch away from every approx_kl it is compared with."""
    if stop_at is None:
        limit = 2.0 * k64.max() + 20 * e
        seen = k64
    else:
        below, seen = k64[:stop_at - 1].max(), k64[:stop_at]
        assert k64[stop_at - 1] > below, ("the float64 loop sets no record at minibatch", stop_at, k64)
        limit = 0.5 * (below + k64[stop_at - 1])
    assert np.abs(seen - limit).min() >= 10 * e, (stop_at, limit, k64, e)
    return limit / 1.5


@pytest.mark.parametrize("stop_at", [PER_EPOCH, PER_EPOCH + 1, PER_EPOCH + 2, None],
                         ids=["last-of-epoch-0", "first-of-epoch-1", "mid-epoch", "never"])
def test_target_kl_through_update(run, kls, stop_at):
    r = run
    k64, e = kls
    target = _target(k64, e, stop_at)
    r.restore()
    stats = r.ro.update(r.pol, r.module, r.opt, n_epochs=EPOCHS, batch_size=BATCH, target_kl=target, perm_seed=SEED, **KW)
    got = r.state()
    log = r.ro.train_log()
    rows = np.stack([s.cpu().numpy() for s in stats])
    print("ppo-train target_kl", stop_at, target, "approx_kl rows", [f"{x:.3e}" for x in rows[:, 4]], log)
    run_m = M_ALL if stop_at is None else stop_at
    assert len(stats) == run_m and log["minibatches"] == run_m and log["early_stop"] == (stop_at is not None)
    assert log["n_updates"] == (EPOCHS if stop_at is None else (stop_at - 1) // PER_EPOCH + 1)
    r.restore()
    r.first(M_ALL if stop_at is None else stop_at - 1)
    ok, why = _equal_states(got, r.state())
    assert ok, why
    assert got[1] == (M_ALL if stop_at is None else stop_at - 1)
    # the log: every mean within one float32 ulp of numpy's over the rows read back
    r64 = rows.astype(np.float64)
    first = (run_m - 1) // PER_EPOCH * PER_EPOCH
    want = dict(entropy_loss=r64[:, 3].mean(), policy_gradient_loss=r64[:, 1].mean(), value_loss=r64[:, 2].mean(),
                clip_fraction=r64[:, 5].mean(), approx_kl=r64[first:, 4].mean())
    for k, w in want.items():
        w32 = np.float32(w)
        assert abs(np.float32(log[k]) - w32) <= np.spacing(np.abs(w32)), (k, log[k], w)
    assert np.float32(log["loss"]) == rows[-1, 0]
    if first > 0 and run_m - first < run_m:  # (the last run epoch's mean is not the mean over all epochs)
        assert np.float32(r64[:, 4].mean()) != np.float32(want["approx_kl"])
        assert np.float32(log["approx_kl"]) != np.float32(r64[:, 4].mean())
    y, p = r.ro.returns.cpu().numpy().astype(np.float64), r.ro.values.cpu().numpy().astype(np.float64)
    ratio = np.var(y - p) / np.var(y)
    assert abs(log["variance_ratio"] - ratio) <= 5e-7 * ratio
    assert abs(log["explained_variance"] - (1 - ratio)) <= 1e-6 * max(1.0, abs(1 - ratio))


def test_update_defaults_log_and_perm_seed(run, monkeypatch):
    """Without target_kl nothing synchronises and nothing new is launched until train_log(); perm_seed makes the
    update a function of the state and the seed alone, with no torch.randperm."""
    r = run
    r.restore()
    calls = []
    real = torch.randperm
    monkeypatch.setattr(torch, "randperm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    launched = []
    real_log = r.ro._read_log
    monkeypatch.setattr(r.ro, "_read_log", lambda: (launched.append(1), real_log())[1])
    stats = r.ro.update(r.pol, r.module, r.opt, n_epochs=EPOCHS, batch_size=BATCH, perm_seed=SEED, **KW)
    assert not calls and not launched and len(stats) == M_ALL and r.opt.step_count == M_ALL
    a = r.state()
    log = r.ro.train_log()
    assert launched == [1]
    monkeypatch.undo()
    rows = np.stack([s.cpu().numpy() for s in stats]).astype(np.float64)
    assert log["minibatches"] == M_ALL and not log["early_stop"] and log["n_updates"] == EPOCHS
    assert abs(np.float32(log["approx_kl"]) - np.float32(rows[-PER_EPOCH:, 4].mean())) <= np.spacing(np.float32(rows[-PER_EPOCH:, 4].mean()))
    assert np.float32(log["loss"]) == np.float32(rows[-1, 0])
    r.restore()
    r.ro.update(r.pol, r.module, r.opt, n_epochs=EPOCHS, batch_size=BATCH, perm_seed=SEED, **KW)
    ok, why = _equal_states(a, r.state())
    assert ok, why
    r.restore()
    r.ro.update(r.pol, r.module, r.opt, n_epochs=EPOCHS, batch_size=BATCH, perm_seed=SEED + 1, **KW)
    assert not _equal_states(a, r.state())[0]
    # the second update of a rollout draws other permutations than its first
    assert not np.array_equal(R.permutation_reference(240, SEED, 0), R.permutation_reference(240, SEED, EPOCHS))
    p0 = r.ro.permutation(SEED, 2).cpu().numpy()
    assert np.array_equal(p0, R.permutation_reference(240, SEED, 2))
    # value clipping through update, and the Python refusals
    r.restore()
    r.ro.update(r.pol, r.module, r.opt, n_epochs=1, batch_size=BATCH, perm_seed=SEED, clip_range_vf=0.05, **KW)
    assert not _equal_states(a, r.state())[0]
    for bad in (dict(clip_range_vf=-1.0), dict(clip_range_vf=float("nan")), dict(target_kl=-0.1), dict(target_kl=float("inf"))):
        r.restore()
        before = r.state()
        with pytest.raises(ValueError):
            r.ro.update(r.pol, r.module, r.opt, n_epochs=1, batch_size=BATCH, **bad, **KW)
        assert _equal_states(before, r.state())[0]


def test_target_kl_with_a_torch_optimiser(run, kls):
    """A torch.optim optimiser reads approx_kl per minibatch on the host and breaks where the gate would."""
    r = run
    k64, e = kls
    stop_at = PER_EPOCH + 1
    r.restore()
    topt = torch.optim.Adam(r.module.parameters(), lr=LR, eps=1e-5)
    stats = r.ro.update(r.pol, r.module, topt, n_epochs=EPOCHS, batch_size=BATCH, target_kl=_target(k64, e, stop_at),
                        perm_seed=SEED, **KW)
    log = r.ro.train_log()
    assert len(stats) == stop_at and log["minibatches"] == stop_at and log["early_stop"] and log["n_updates"] == 2
    r.restore()
    r.pol.load_state_dict(r.module.state_dict())
