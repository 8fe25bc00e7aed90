"""The cost channel through the device rollout (pgtg_amd.rollout.Rollout with cost_limit=): the step's own
k_flatten pass records info["cost"] into costs[t], finish() runs k_cost_scan / k_cost_dual and hands k_gae the
penalised rewards, and the multiplier, the carry and the log cross three consecutive rollouts -- against the
env's own cost output, the CPU oracle, cost_reference and gae_reference, bit for bit."""
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
from digest_parity import _spec
from oracle.oracle import OracleEnv

pytestmark = pytest.mark.gpu

F = np.float32
N, T, ROLLOUTS, LIMIT, SEED = 300, 12, 3, 5, 7  # a full and a partial workgroup; episodes close inside a rollout
CONF = dict(random_map_width=3, random_map_height=3, separate_reward_cost=True, standing_still_penalty=1,
            traffic_density=0.5)
GAMMA, GAE_LAMBDA = 0.99, 0.95
STILL = 4  # the action without acceleration: (a // 3 - 1, a % 3 - 1) = (0, 0)


def _vec(n, conf=CONF, **kw):
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PGTGVecEnv(n, device=0, autoreset=True, max_episode_steps=LIMIT, **conf, **kw)


def _actions(steps, n, seed):
    """Seeded uint8 actions, a third of them the no-acceleration action (standing still occurs)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 9, (steps, n), generator=g)
    a[torch.rand((steps, n), generator=g) < 1 / 3] = STILL
    return a.to(torch.uint8).cuda()


class _Limited:
    """OracleEnv behind a TimeLimit with same-step auto-reset (the test's own step count)."""

    def __init__(self, spec, seed):
        self.o, self.elapsed = OracleEnv(spec), 0
        self.o.reset(seed)

    def step(self, a):
        r = self.o.step(int(a))
        self.elapsed += 1
        if r["terminated"] or self.elapsed >= LIMIT:
            self.elapsed = 0
            self.o.reset(None)
        return r


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.int32, 8: np.int64}[x.dtype.itemsize])


def _run(cost_limit, oracle_envs=(), old_way=False, **kw):
    """ROLLOUTS consecutive rollouts of the same seeds and actions; per rollout the recorded rows, the carry and
    multiplier it started from, and what finish() left, as host arrays."""
    env = _vec(N)
    ro = env.rollout(T, GAMMA, GAE_LAMBDA) if old_way else env.rollout(T, GAMMA, GAE_LAMBDA, cost_limit=cost_limit, **kw)
    acts = _actions(ROLLOUTS * T, N, seed=11)
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    orcs = [_Limited(env.spec, SEED + int(i)) for i in oracle_envs]
    tix = torch.as_tensor(np.asarray(oracle_envs, dtype=np.int64), device="cuda")
    host = lambda x: x.cpu().numpy().copy()  # noqa: E731
    out = []
    for k in range(ROLLOUTS):
        ro.begin(seed=SEED) if k == 0 else ro.begin()
        rec = {}
        if cost_limit is not None:
            rec["carry"], rec["lam"] = host(ro.ep_cost), F(ro.lagrange_multiplier)
        vals, tv, last = rnd(T, N), rnd(T, N), rnd(N)
        for t in range(T):
            ro.step(acts[k * T + t], values=vals[t])
            ro.set_terminal_values(tv[t])
            if cost_limit is not None:
                now = env.cost.clone()
                assert torch.equal(ro.costs[t].view(torch.int32), now.to(torch.float32).view(torch.int32)), (k, t)
                if orcs:
                    got, a = host(ro.costs[t].index_select(0, tix)), host(acts[k * T + t].index_select(0, tix))
                    want = np.array([o.step(a[j])["cost"] for j, o in enumerate(orcs)], dtype=np.float64)
                    assert np.array_equal(_bits(got), _bits(want.astype(F))), (k, t, got, want)
        ro.finish(last)
        torch.cuda.synchronize()
        for name in ("rewards", "values", "dones", "truncated_only", "terminal_values", "advantages", "returns"):
            rec[name] = host(getattr(ro, name))
        rec["last"] = host(last)
        if cost_limit is not None:
            rec.update(costs=host(ro.costs), penalised=host(ro.penalised_rewards), ep_cost=host(ro.ep_cost),
                       log=ro.cost_log(), lam_next=F(ro.lagrange_multiplier))
        out.append(rec)
    assert env.error_count()[0] == 0
    info = dict(nbytes=ro.nbytes, has_costs=hasattr(ro, "costs"))
    ro.close()
    env.close()
    return out, info


@pytest.fixture(scope="module")
def budget_zero():
    idx = np.unique(np.concatenate([[0, 1, 63, 64, 127, 128, 255, 256, 257, N // 2, N - 2, N - 1],
                                    np.random.default_rng(3).choice(N, 14, replace=False)]))[:24]
    assert len(idx) == 24
    return _run(0.0, oracle_envs=idx)


@pytest.fixture(scope="module")
def plain():
    return _run(None)


def test_costs_are_recorded_and_scanned(budget_zero):
    from pgtg_amd.rollout import cost_reference, gae_reference
    recs, info = budget_zero
    carry, lam = np.zeros(N), F(0.0)
    for k, r in enumerate(recs):
        assert np.array_equal(r["carry"], carry) and r["lam"] == lam, k  # (the previous rollout's, or the reset's zeros)
        pen, carry, eps, summary, lam = cost_reference(r["rewards"], r["costs"], r["dones"], r["carry"], r["lam"],
                                                       0.0, 0.05, 100.0)
        # the test's own requirements of its inputs
        assert (r["costs"] != 0).any() and summary["episodes"] > 0 and (eps != 0).any(), k
        assert r["truncated_only"].any()
        assert np.array_equal(_bits(r["penalised"]), _bits(pen)), k
        assert np.array_equal(_bits(r["ep_cost"]), _bits(carry)), k
        assert r["log"] == {"cost/ep_cost_mean": summary["cost_mean"], "cost/ep_cost_max": summary["cost_max"],
                            "cost/episodes": summary["episodes"], "cost/lambda": float(summary["lambda_before"]),
                            "cost/lambda_next": float(summary["lambda_after"])}, (k, r["log"], summary)
        assert _bits(r["lam_next"]) == _bits(lam), k
        adv, ret = gae_reference(pen, r["values"], r["dones"], r["truncated_only"], r["terminal_values"], r["last"],
                                 GAMMA, GAE_LAMBDA)
        assert np.array_equal(_bits(r["advantages"]), _bits(adv)) and np.array_equal(_bits(r["returns"]), _bits(ret)), k
        if k == 0:
            assert lam > 0  # the multiplier is off zero after the first rollout
            assert np.array_equal(_bits(r["penalised"]), _bits(r["rewards"]))  # (which itself ran at lambda = 0)
        else:
            assert (r["carry"] != 0).any() and not np.array_equal(r["penalised"], r["rewards"]), k
    assert (carry != 0).any()


def test_a_budget_out_of_reach_holds_the_multiplier_at_zero(plain):
    recs, _ = _run(1e9)
    for k, (r, p) in enumerate(zip(recs, plain[0])):
        assert r["lam"] == 0 and r["lam_next"] == 0 and r["log"]["cost/lambda_next"] == 0.0 and r["log"]["cost/episodes"] > 0
        assert r["log"]["cost/ep_cost_mean"] > 0  # (the clamp, not an absent cost)
        for name in ("rewards", "dones", "advantages", "returns"):
            assert np.array_equal(_bits(r[name]), _bits(p[name])), (k, name)
        assert np.array_equal(_bits(r["penalised"]), _bits(r["rewards"]))


def test_without_a_budget_the_rollout_is_the_old_one(plain, budget_zero):
    old, old_info = _run(None, old_way=True)
    new, info = plain
    assert not info["has_costs"] and info["nbytes"] == old_info["nbytes"]
    for k, (r, p) in enumerate(zip(new, old)):
        assert sorted(r) == sorted(p)
        for name in r:
            assert np.array_equal(_bits(r[name]), _bits(p[name])), (k, name)
    # with a budget: the same raw rewards, the cost tensors on top, other advantages once the multiplier moved
    recs, cost_info = budget_zero
    assert cost_info["nbytes"] == info["nbytes"] + 2 * T * N * 4 + N * 8 + 4 + 40 + 2 * 24
    for r, p in zip(recs, new):
        assert np.array_equal(_bits(r["rewards"]), _bits(p["rewards"]))
    assert not np.array_equal(recs[1]["advantages"], new[1]["advantages"])


def test_the_arguments_are_checked():
    env = _vec(4, conf=dict(random_map_width=3, random_map_height=3))
    with pytest.raises(ValueError, match="separate_reward_cost"):
        env.rollout(2, cost_limit=1.0)
    env.rollout(2).close()
    env.close()
    env = _vec(4)
    for kw in (dict(cost_limit=float("nan")), dict(cost_limit=1.0, lambda_lr=float("inf")), dict(cost_limit=1.0, lambda_max=-1.0),
               dict(cost_limit=1.0, lambda_init=2.0, lambda_max=1.0)):
        with pytest.raises(ValueError):
            env.rollout(2, **kw)
    ro = env.rollout(2)
    for use in (ro.cost_log, lambda: ro.lagrange_multiplier):
        with pytest.raises(RuntimeError):
            use()
    ro.close()
    ro = env.rollout(2, cost_limit=1.0, lambda_init=0.25, lambda_max=8.0)
    assert ro.lagrange_multiplier == 0.25
    ro.lagrange_multiplier = 3.5  # (a checkpoint's)
    assert ro.lagrange_multiplier == 3.5
    with pytest.raises(ValueError):
        ro.lagrange_multiplier = 9.0
    with pytest.raises(RuntimeError):
        ro.cost_log()  # before finish()
    ro.close()
    env.close()


def test_collect_and_update_run_with_a_budget():
    from pgtg_amd import policy as P
    from pgtg_amd.flat import flat_dim
    env = _vec(N)
    torch.manual_seed(4)
    module = P.MlpPolicyReference(flat_dim(env.spec)).cuda()
    pol = P.DevicePolicy(env, seed=21)
    pol.load_state_dict(module.state_dict())
    opt = P.DeviceAdam(pol, module)
    start = {k: v.clone() for k, v in module.state_dict().items()}
    ro = env.rollout(4, cost_limit=0.5)
    for _ in range(2):
        ro.collect(pol)
        ro.update(pol, module, opt, n_epochs=1, batch_size=600, perm_seed=1)
    torch.cuda.synchronize()
    log = ro.cost_log()
    assert log["cost/episodes"] > 0 and np.isfinite(log["cost/ep_cost_mean"]) and 0.0 <= log["cost/lambda_next"] <= 100.0
    assert all(bool(torch.isfinite(v).all()) for v in module.state_dict().values())
    assert any(not torch.equal(v, start[k]) for k, v in module.state_dict().items())
    assert env.error_count()[0] == 0
    assert np.isfinite(ro.train_log()["loss"])
    ro.close()
    env.close()
