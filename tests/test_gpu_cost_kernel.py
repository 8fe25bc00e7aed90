"""The cost scan of a rollout on synthetic device arrays: the HIP kernels k_cost_scan and k_cost_dual
(include/pgtg.h pgtg_cost_scan; pgtg_amd/csrc/pgtg_cost.h) against cost_reference (pgtg_amd/rollout.py), at
every shape around the workgroup, the wave and the kernel's ring of rows in flight."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
from pgtg_amd.rollout import COST_AHEAD as P

pytestmark = pytest.mark.gpu

F = np.float32
NS = (1, 63, 64, 65, 255, 256, 257, 513, 1000)  # partial waves, a full workgroup, partial workgroups
TS = (1, 2, 3, P - 1, P, P + 1, 2 * P, 2 * P + 1, 4 * P, 4 * P + 1, 130)  # below, at and above the ring, with a remainder
PATTERNS = ("none", "all", "rate", "last_row", "row_0")
# (lam, cost_limit, lambda_lr, lambda_max), all dyadic: the multiplier rises; is clamped at 0; at lambda_max
RISE = (0.5, 0.25, 0.125, 2.0 ** 20)
FLOOR = (0.5, 2.0 ** 20, 0.5, 64.0)
CEIL = (0.5, 0.0, 1024.0, 4.0)
SUMMARY = ("episodes", "cost_sum", "cost_mean", "cost_max", "lambda_before", "lambda_after")


@pytest.fixture(scope="module")
def handle():
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = PGTGVecEnv(2, device=0, random_map_width=3, random_map_height=3)  # (its batch size is not the rollouts')
    yield env
    env.close()


def _inputs(T, N, pattern, seed, exact):
    rng = np.random.default_rng(seed)
    d = dict(rewards=(rng.standard_normal((T, N)) * 100).astype(F))
    if exact:  # multiples of 1/8 below 64: every fp64 sum of them is exact in any order
        d["costs"] = (rng.integers(0, 512, (T, N)) / 8).astype(F)
        d["carry"] = (rng.integers(8, 64, N) / 8).astype(np.float64)  # (non-zero)
    else:
        d["costs"] = (rng.random((T, N)) * 7).astype(F)
        d["carry"] = rng.random(N) + 0.5
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
    return d


def _workspace_bytes(env, n):
    nbytes = C.c_uint64()
    assert env._lib.pgtg_cost_workspace_bytes(n, C.byref(nbytes)) == 0
    return nbytes.value


def _scan(env, d, lam, cost_limit, lambda_lr, lambda_max, fill=None, null=None, **over):
    """pgtg_cost_scan on device copies of d.  fill: the outputs start as this sentinel.  Returns (rc, outputs)."""
    from pgtg_amd import _abi
    T, N = d["rewards"].shape
    # every array is a fresh tensor of exactly its size, starting at offset 0 of its storage: a row in front
    # of it, or behind it, is not the test's memory
    dev = {k: torch.as_tensor(np.ascontiguousarray(d[k])).cuda() for k in ("rewards", "costs", "dones", "carry")}
    dev["penalised"] = torch.full((T, N), 0.0 if fill is None else fill, dtype=torch.float32, device="cuda")
    dev["lambda_"] = torch.full((1,), lam, dtype=torch.float32, device="cuda")
    dev["summary"] = torch.full((5,), 0 if fill is None else int(fill), dtype=torch.int64, device="cuda")
    dev["workspace"] = torch.full((_workspace_bytes(env, N),), 0 if fill is None else int(fill), dtype=torch.uint8, device="cuda")
    assert all(t.storage_offset() == 0 and t.untyped_storage().nbytes() == t.numel() * t.element_size() for t in dev.values())
    p = lambda k: None if k == null else C.c_void_p(dev[k].data_ptr())  # noqa: E731
    a = _abi.PgtgCost(n=over.get("n", N), steps=over.get("steps", T), rewards=p("rewards"), costs=p("costs"), dones=p("dones"),
                      ep_cost=p("carry"), penalised=p("penalised"), lambda_=p("lambda_"), cost_limit=cost_limit,
                      lambda_lr=lambda_lr, lambda_max=lambda_max, summary=p("summary"), workspace=p("workspace"))
    env._bind_stream()
    rc = env._lib.pgtg_cost_scan(env._h, C.byref(a))
    torch.cuda.synchronize()
    s = _abi.PgtgCostSummary.from_buffer_copy(dev["summary"].cpu().numpy().tobytes())
    out = dict(penalised=dev["penalised"].cpu().numpy(), ep_cost=dev["carry"].cpu().numpy(),
               lam=dev["lambda_"].cpu().numpy()[0], summary={f: getattr(s, f) for f in SUMMARY},
               raw_summary=dev["summary"].cpu().numpy(), workspace=dev["workspace"].cpu().numpy())
    return rc, out


def _reference(d, lam, cost_limit, lambda_lr, lambda_max):
    from pgtg_amd.rollout import cost_reference
    return cost_reference(d["rewards"], d["costs"], d["dones"], d["carry"], lam, cost_limit, lambda_lr, lambda_max)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32 if x.dtype == F else np.int64)


def _assert_lane_exact(out, pen, carry, tag):
    assert np.array_equal(_bits(out["penalised"]), _bits(pen)), tag
    assert np.array_equal(_bits(out["ep_cost"]), _bits(carry)), tag


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("T", TS)
def test_exact_costs_match_the_reference_bit_for_bit(handle, T, N):
    with_cost, without_episode = False, False
    for pattern in PATTERNS:
        d = _inputs(T, N, pattern, seed=1000 * T + N, exact=True)
        for setting in ((RISE, FLOOR, CEIL) if pattern == "all" else (RISE,)):
            rc, out = _scan(handle, d, *setting)
            assert rc == 0
            pen, carry, eps, summary, nxt = _reference(d, *setting)
            tag = (pattern, setting)
            _assert_lane_exact(out, pen, carry, tag)
            for f in SUMMARY:
                got, want = out["summary"][f], summary[f]
                assert got == want and (f == "episodes" or np.signbit(got) == np.signbit(want)), (tag, f, got, want)
            assert _bits(F(out["lam"])) == _bits(F(nxt)), tag
            # what the inputs were built to produce, shown by the reference alone
            ended = d["dones"][1:].any(0)
            with_cost |= bool((eps != 0).any())
            without_episode |= bool((~ended).any())
            if pattern == "all":
                lam, _, _, lmax = setting
                assert summary["episodes"] == T * N
                assert {RISE: lam < nxt < lmax, FLOOR: nxt == 0.0, CEIL: nxt == lmax}[setting], tag
            if pattern == "none":
                assert summary["episodes"] == 0 and nxt == F(setting[0])
                assert np.array_equal(carry, d["carry"] + d["costs"].astype(np.float64).sum(0))  # (exact in any order)
    assert with_cost and without_episode


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("T", TS)
def test_rounding_costs_stay_within_the_order_free_bound(handle, T, N):
    lam, cost_limit, lambda_lr, lambda_max = 0.3, 1.5, 0.05, 100.0
    with_cost, without_episode = False, False
    for pattern in PATTERNS:
        d = _inputs(T, N, pattern, seed=7000 * T + N, exact=False)
        rc, out = _scan(handle, d, lam, cost_limit, lambda_lr, lambda_max)
        assert rc == 0
        pen, carry, eps, summary, nxt = _reference(d, lam, cost_limit, lambda_lr, lambda_max)
        # per lane the operations and their order are the reference's
        _assert_lane_exact(out, pen, carry, pattern)
        got = out["summary"]
        k = summary["episodes"]
        assert got["episodes"] == k == len(eps) and got["cost_max"] == summary["cost_max"]
        assert got["lambda_before"] == F(lam)
        # an fp64 sum of k non-negative terms in any order
        bound = k * 2.0 ** -52 * summary["cost_sum"]
        print(T, N, pattern, "cost_sum", got["cost_sum"], summary["cost_sum"], "bound", bound, "lambda", out["lam"], nxt)
        assert abs(got["cost_sum"] - summary["cost_sum"]) <= bound, pattern
        assert abs(got["cost_sum"] - float(np.sum(eps))) <= bound, pattern  # (numpy's pairwise order)
        assert abs(float(out["lam"]) - float(nxt)) <= lambda_lr * bound / max(k, 1) + float(np.spacing(F(nxt))), pattern
        assert got["lambda_after"] == out["lam"]
        # cost_reference sums in the kernels' own order (the tree of pgtg_cost.h), so the bits agree too
        assert got["cost_sum"] == summary["cost_sum"] and got["cost_mean"] == summary["cost_mean"], pattern
        assert _bits(F(out["lam"])) == _bits(F(nxt)), pattern
        with_cost |= bool((eps != 0).any())
        without_episode |= bool((~d["dones"][1:].any(0)).any())
    assert with_cost and without_episode


def test_two_runs_give_the_same_bits(handle):
    d = _inputs(130, 1000, "rate", seed=8, exact=False)
    _, a = _scan(handle, d, 0.3, 1.5, 0.05, 100.0)
    _, b = _scan(handle, d, 0.3, 1.5, 0.05, 100.0)
    for k in ("penalised", "ep_cost", "raw_summary", "workspace"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert _bits(F(a["lam"])) == _bits(F(b["lam"])) and a["summary"]["episodes"] > 0


def test_argument_errors_launch_nothing(handle):
    from pgtg_amd import _abi
    T, N = 7, 65
    d = _inputs(T, N, "rate", seed=9, exact=True)
    nan, inf = float("nan"), float("inf")
    good = dict(lam=0.5, cost_limit=1.0, lambda_lr=0.25, lambda_max=8.0)
    cases = [dict(steps=0), dict(cost_limit=nan), dict(cost_limit=inf), dict(lambda_lr=nan), dict(lambda_lr=-inf),
             dict(lambda_max=-1.0), dict(lambda_max=nan)]
    cases += [dict(null=k) for k in ("rewards", "costs", "dones", "carry", "penalised", "lambda_", "summary", "workspace")]
    big = [dict(steps=1 << 31), dict(n=1 << 41), dict(n=1 << 33, steps=1 << 30)]  # (refused before any launch: never dereferenced)
    for kw in cases + big:
        args = {**good, **{k: v for k, v in kw.items() if k in good}}
        rest = {k: v for k, v in kw.items() if k not in good}
        rc, out = _scan(handle, d, fill=3.0, **args, **rest)
        assert rc == (_abi.PGTG_E_UNSUPPORTED if kw in big else _abi.PGTG_E_INVALID), kw
        assert handle._lib.pgtg_last_error(handle._h).decode().startswith("pgtg_cost_scan"), kw
        assert (out["penalised"] == 3.0).all() and np.array_equal(out["ep_cost"], d["carry"]), kw
        assert out["lam"] == F(0.5) and (out["raw_summary"] == 3).all() and (out["workspace"] == 3).all(), kw
    # no envs: nothing to do
    rc, out = _scan(handle, d, fill=3.0, n=0, **good)
    assert rc == 0 and (out["penalised"] == 3.0).all() and (out["raw_summary"] == 3).all() and out["lam"] == F(0.5)
    # and the same call without the fault runs
    rc, out = _scan(handle, d, fill=3.0, **good)
    assert rc == 0 and not (out["penalised"] == 3.0).any() and out["summary"]["episodes"] > 0
