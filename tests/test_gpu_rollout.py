"""The device rollout buffer: the HIP kernel k_gae (include/pgtg.h pgtg_gae) bit for bit against
gae_reference, and pgtg_amd.rollout.Rollout -- the steps recording themselves into the rollout's rows,
finish() and get() -- against the existing set_flat_outputs / set_flat_scalars path and numpy."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
NS = (1, 63, 64, 65, 257, 1000)   # partial waves, partial workgroups, rows that are not 16-byte aligned
TS = (1, 2, 3, 7, 8, 9, 130)      # below, at and above the rows in flight, with a remainder
# whole groups of 16 rows: the unguarded steady groups' cursors must stop inside the rollout (the flag
# cursor once ended one row in front of truncated_only for T = 32, 48, 64, ...: read, never used)
TS_GROUPS = (16, 32, 48, 64, 128, 144)
SHAPES = sorted({(T, n) for n in NS for T in (7, 130)} | {(T, 65) for T in TS + TS_GROUPS} | {(128, 1000)})
PAIRS = ((0.99, 0.95), (0.9, 0.95))
PATTERNS = ("none", "all", "rate", "last_row", "row_0")
# the caller's settings (pgtg/train.py:21-38)
TRAIN = dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=0.2,
             random_map_percentage_of_connections=0.8, traffic_density=0.2, conservative_driver_percentage=0.15,
             normal_driver_percentage=0.50, aggressive_driver_percentage=0.20, elderly_driver_percentage=0.10,
             reckless_driver_percentage=0.05, sliding_observation_window_size=5, max_allowed_deviation=15,
             use_sliding_observation_window=True, use_next_subgoal_direction=True, final_goal_bonus=200,
             standing_still_penalty=1)


def _vec(n, **kw):
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PGTGVecEnv(n, device=0, **kw)


@pytest.fixture(scope="module")
def handle():
    env = _vec(2, random_map_width=3, random_map_height=3)  # (its batch size is not the rollouts')
    yield env
    env.close()


def _inputs(T, N, pattern, seed):
    rng = np.random.default_rng(seed)
    d = {k: (rng.standard_normal((T, N)) * 100).astype(F) for k in ("rewards", "values", "terminal_values")}
    d["last_values"] = (rng.standard_normal(N) * 100).astype(F)
    dones = np.zeros((T + 1, N), bool)
    if pattern == "all":
        dones[:] = True
    elif pattern == "rate":
        dones = rng.random((T + 1, N)) < 0.2
    elif pattern == "last_row":
        dones[T] = True
    elif pattern == "row_0":
        dones[0] = True
    d["dones"] = dones
    d["truncated_only"] = dones[1:] & (rng.random((T, N)) < 0.5)
    return d


def _gae(env, d, gamma, lam, bootstrap="both", steps=None, out=None, n=None):
    """pgtg_gae on device copies of d; returns (rc, advantages, returns) as host arrays."""
    from pgtg_amd import _abi
    T, N = d["rewards"].shape
    # every array is a fresh tensor of exactly its size, starting at offset 0 of its storage: a row in
    # front of it, or behind it, is not the test's memory
    dev = {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    assert all(t.storage_offset() == 0 and t.untyped_storage().nbytes() == t.numel() * t.element_size()
               for t in dev.values())
    adv, ret = out if out is not None else (torch.zeros((T, N), device="cuda"), torch.zeros((T, N), device="cuda"))
    p = lambda k: C.c_void_p(dev[k].data_ptr())  # noqa: E731
    g = _abi.PgtgGae(n=N if n is None else n, steps=T if steps is None else steps, gamma=gamma, gae_lambda=lam, rewards=p("rewards"),
                     values=p("values"), dones=p("dones"), last_values=p("last_values"),
                     truncated_only=p("truncated_only") if bootstrap in ("both", "flags") else None,
                     terminal_values=p("terminal_values") if bootstrap in ("both", "values") else None,
                     advantages=C.c_void_p(adv.data_ptr()), returns=C.c_void_p(ret.data_ptr()))
    env._bind_stream()
    rc = env._lib.pgtg_gae(env._h, C.byref(g))
    torch.cuda.synchronize()
    return rc, adv, ret


def _same_bits(t, a) -> bool:
    want = torch.as_tensor(np.ascontiguousarray(a, dtype=F)).cuda()
    return torch.equal(t.view(torch.int32), want.view(torch.int32))


def _reference(d, gamma, lam):
    from pgtg_amd.rollout import gae_reference
    return gae_reference(d["rewards"], d["values"], d["dones"], d["truncated_only"], d["terminal_values"],
                         d["last_values"], gamma, lam)


@pytest.mark.parametrize("T, N", SHAPES)
def test_k_gae_matches_the_reference(handle, T, N):
    for pattern in PATTERNS:
        d = _inputs(T, N, pattern, seed=1000 * T + N)
        for gamma, lam in PAIRS:
            rc, adv, ret = _gae(handle, d, gamma, lam)
            assert rc == 0
            want_adv, want_ret = _reference(d, gamma, lam)
            assert _same_bits(adv, want_adv), (pattern, gamma)
            assert _same_bits(ret, want_ret), (pattern, gamma)


@pytest.mark.parametrize("T, N", [(7, 65), (130, 257)])
def test_terminal_values_enter_by_select_not_by_add(handle, T, N):
    d = _inputs(T, N, "rate", seed=5)
    free = np.argwhere(~d["truncated_only"])
    t0, e0 = free[len(free) // 2]
    d["rewards"][t0, e0] = F(-0.0)
    d["values"][t0, e0] = F(-0.0)
    d["dones"][t0 + 1, e0] = True  # r + (g nv) 0 - v = -0.0 + 0.0 * ... : the sign depends on every operand
    d["truncated_only"][t0, e0] = False
    rc, adv, ret = _gae(handle, d, 0.99, 0.95)
    dirty = dict(d, terminal_values=np.where(d["truncated_only"], d["terminal_values"], F(np.nan)).astype(F))
    rc2, adv2, ret2 = _gae(handle, dirty, 0.99, 0.95)
    assert rc == rc2 == 0
    assert bool(torch.isfinite(adv2).all()) and bool(torch.isfinite(ret2).all())
    assert torch.equal(adv.view(torch.int32), adv2.view(torch.int32))
    assert torch.equal(ret.view(torch.int32), ret2.view(torch.int32))
    want_adv, want_ret = _reference(dirty, 0.99, 0.95)
    assert _same_bits(adv2, want_adv) and _same_bits(ret2, want_ret)
    # the sample's zero keeps the sign the formula gives it
    assert np.signbit(want_ret[t0, e0]) == bool(torch.signbit(ret2[t0, e0]))
    assert float(ret2[t0, e0]) == 0.0


def test_no_bootstrap_pointers_means_no_truncated_sample(handle):
    d = _inputs(9, 65, "rate", seed=6)
    rc, adv, ret = _gae(handle, d, 0.9, 0.95, bootstrap="none")
    rc0, adv0, ret0 = _gae(handle, dict(d, truncated_only=np.zeros_like(d["truncated_only"])), 0.9, 0.95)
    assert rc == rc0 == 0
    assert torch.equal(adv.view(torch.int32), adv0.view(torch.int32))
    assert torch.equal(ret.view(torch.int32), ret0.view(torch.int32))
    assert not torch.equal(adv, _gae(handle, d, 0.9, 0.95)[1])  # (the truncated samples do matter)


def test_argument_errors_launch_nothing(handle):
    from pgtg_amd import _abi
    d = _inputs(7, 65, "rate", seed=7)
    for kw in (dict(steps=0), dict(bootstrap="flags"), dict(bootstrap="values"), dict(gamma=float("nan")),
               dict(lam=float("inf"))):
        out = (torch.full((7, 65), 5.0, device="cuda"), torch.full((7, 65), 6.0, device="cuda"))
        rc, adv, ret = _gae(handle, d, kw.pop("gamma", 0.99), kw.pop("lam", 0.95), out=out, **kw)
        assert rc == _abi.PGTG_E_INVALID
        assert handle._lib.pgtg_last_error(handle._h).decode().startswith("pgtg_gae")
        assert bool((adv == 5.0).all()) and bool((ret == 6.0).all())
    # no envs: nothing to do
    out = (torch.full((7, 65), 5.0, device="cuda"), torch.full((7, 65), 6.0, device="cuda"))
    rc, adv, ret = _gae(handle, d, 0.99, 0.95, out=out, n=0)
    assert rc == 0 and bool((adv == 5.0).all()) and bool((ret == 6.0).all())


def test_two_runs_give_the_same_bits(handle):
    d = _inputs(130, 1000, "rate", seed=8)
    _, a1, r1 = _gae(handle, d, 0.9, 0.95)
    _, a2, r2 = _gae(handle, d, 0.9, 0.95)
    assert torch.equal(a1.view(torch.int32), a2.view(torch.int32))
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32))


# -- recording ------------------------------------------------------------------------------------
N_REC, T_REC, LIMIT = 300, 12, 5


def _record(obs_dtype):
    """Two rollouts through Rollout and the same steps through the fresh-tensor path of the parent."""
    from pgtg_amd.flat import flat_dim
    a = _vec(N_REC, autoreset=True, max_episode_steps=LIMIT, **TRAIN)
    b = _vec(N_REC, autoreset=True, max_episode_steps=LIMIT, **TRAIN)
    ro = a.rollout(T_REC, gamma=0.99, gae_lambda=0.95, obs_dtype=obs_dtype)
    D = flat_dim(a.spec)
    assert tuple(ro.obs.shape) == (T_REC + 1, N_REC, D) and ro.obs.dtype == obs_dtype
    assert ro.nbytes >= ro.obs.numel() * ro.obs.element_size() + 6 * 4 * T_REC * N_REC
    acts = b.random_actions(2 * T_REC, seed=3)
    new = lambda *s, dt=obs_dtype: torch.empty(s, dtype=dt, device="cuda")  # noqa: E731
    flat0 = new(N_REC, D)
    b.set_flat_outputs(flat0, new(N_REC, D))
    b.reset(seed=7)
    rolls, term, trunc = [], 0, 0
    for k in range(2):
        first = ro.begin(seed=7) if k == 0 else ro.begin()
        assert first.data_ptr() == ro.obs[0].data_ptr()
        if k == 0:
            assert torch.equal(ro.obs[0], flat0) and bool(ro.dones[0].all())
        else:
            assert torch.equal(ro.obs[0], rolls[0]["obs"][T_REC]) and torch.equal(ro.dones[0], rolls[0]["dones"][T_REC])
            assert not bool(ro.dones[0].all())
        for t in range(T_REC):
            flat, fin = new(N_REC, D), new(N_REC, D)
            sc = (new(N_REC, dt=torch.float32), new(N_REC, dt=torch.bool), new(N_REC, dt=torch.bool))
            b.set_flat_outputs(flat, fin)
            b.set_flat_scalars(*sc)
            b.step_launch(acts[k * T_REC + t])
            o, r, dn = ro.step(acts[k * T_REC + t])
            assert o.data_ptr() == ro.obs[t + 1].data_ptr() and r.data_ptr() == ro.rewards[t].data_ptr()
            assert dn.data_ptr() == ro.dones[t + 1].data_ptr()
            assert torch.equal(ro.obs[t + 1], flat)
            assert torch.equal(ro.rewards[t].view(torch.int32), sc[0].view(torch.int32))
            assert torch.equal(ro.dones[t + 1], sc[1]) and torch.equal(ro.truncated_only[t], sc[2])
            assert torch.equal(ro.actions[t], acts[k * T_REC + t])
            assert torch.equal(ro.terminal_obs[sc[1]], fin[sc[1]])
            trunc += int(sc[2].sum())
            term += int((sc[1] & ~sc[2]).sum())
        with pytest.raises(RuntimeError):
            ro.step(acts[0])
        rolls.append({k_: getattr(ro, k_).clone() for k_ in ("obs", "dones", "rewards", "truncated_only", "actions")})
    assert trunc >= 1 and term >= 1, (trunc, term)
    b.close()
    return a, ro, rolls[1]


@pytest.mark.parametrize("obs_dtype", [torch.int8, torch.float32])
def test_rollout_records_what_the_flat_path_writes(obs_dtype):
    a, ro, _ = _record(obs_dtype)
    ro.close()
    a.close()


def test_finish_and_get_on_a_recorded_rollout():
    from pgtg_amd.rollout import gae_reference
    a, ro, kept = _record(torch.int8)
    T, N = T_REC, N_REC
    g = torch.Generator(device="cuda").manual_seed(11)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g) * 100  # noqa: E731
    # a third rollout with synthetic policy outputs: values and log_probs per step, terminal values after it
    acts = a.random_actions(T, seed=5)
    vals, logp, tv = rnd(T, N), rnd(T, N), rnd(T, N)
    ro.begin()
    assert torch.equal(ro.obs[0], kept["obs"][T]) and not bool(ro.terminal_values.any())
    for t in range(T):
        ro.step(acts[t].to(torch.int64), values=vals[t], log_probs=logp[t])
        if t != 3:
            ro.set_terminal_values(tv[t])
    tv[3] = 0  # (never set: the row stays zero)
    for got, want in ((ro.values, vals), (ro.log_probs, logp), (ro.terminal_values, tv), (ro.actions, acts)):
        assert torch.equal(got, want)
    # a tensor that is the row itself is taken as it is
    ro.t = T - 1
    row = ro.actions[T - 1]
    ro.step(row, values=ro.values[T - 1], log_probs=ro.log_probs[T - 1])
    assert torch.equal(ro.actions, acts) and torch.equal(ro.values, vals)
    last = rnd(N)
    ro.finish(last)
    torch.cuda.synchronize()
    host = {k: getattr(ro, k).cpu().numpy() for k in ("rewards", "values", "dones", "truncated_only", "terminal_values")}
    assert host["truncated_only"].any()
    want_adv, want_ret = gae_reference(host["rewards"], host["values"], host["dones"], host["truncated_only"],
                                       host["terminal_values"], last.cpu().numpy(), 0.99, 0.95)
    assert _same_bits(ro.advantages, want_adv) and _same_bits(ro.returns, want_ret)
    # minibatches in SB3's order: sample s of the [T, N] -> [N * T] swap_and_flatten
    perm = np.random.default_rng(2).permutation(T * N)
    flat = lambda x: np.swapaxes(x, 0, 1).reshape(T * N, *x.shape[2:])  # noqa: E731
    obs = flat(ro.obs[:T].cpu().numpy())
    cols = [flat(getattr(ro, k).cpu().numpy()) for k in ("actions", "values", "log_probs", "advantages", "returns")]
    B, seen = 1000, 0  # (3 600 samples: three full minibatches and one of 600)
    for lo, batch in zip(range(0, T * N, B), ro.get(batch_size=B, indices=torch.as_tensor(perm))):
        idx = perm[lo:lo + B]
        o, act, *rest = batch
        assert o.dtype == torch.float32 and act.dtype == torch.int64 and o.shape == (len(idx), ro.obs_dim)
        assert np.array_equal(o.cpu().numpy(), obs[idx].astype(F))
        assert np.array_equal(act.cpu().numpy(), cols[0][idx].astype(np.int64))
        for got, col in zip(rest, cols[1:]):
            assert np.array_equal(got.cpu().numpy().view(np.int32), col[idx].view(np.int32))
        seen += len(idx)
    assert seen == T * N and len(list(ro.get(batch_size=B))) == 4
    (everything,) = list(ro.get())
    assert sorted(everything[2].cpu().numpy().tolist()) == sorted(cols[1].tolist())
    ro.close()
    a.close()


def test_misuse_raises():
    env = _vec(4, autoreset=True, max_episode_steps=3, random_map_width=3, random_map_height=3)
    ro = env.rollout(2)
    ro.begin(seed=1)
    acts = torch.zeros(4, dtype=torch.uint8, device="cuda")
    ro.step(acts)
    with pytest.raises(RuntimeError):
        ro.finish(torch.zeros(4, device="cuda"))  # before T
    ro.step(acts)
    with pytest.raises(RuntimeError):
        ro.step(acts)  # past T
    ro.finish(torch.zeros(4, device="cuda"))
    ro.close()
    env.close()
    env = _vec(4, autoreset=False, random_map_width=3, random_map_height=3)
    with pytest.raises(ValueError):
        env.rollout(2)
    env.close()
    env = _vec(4, autoreset=True, random_map_width=3, random_map_height=3, use_sliding_observation_window=True,
               sliding_observation_window_size=9)
    with pytest.raises(ValueError):
        env.rollout(2)
    env.close()
