"""The host side of the rollout's cost channel, no GPU: the library exports the new entry points within ABI
9, the ctypes mirrors match the header, and cost_reference (pgtg_amd/rollout.py) -- the numpy restatement of
k_cost_scan and k_cost_dual, the yardstick of the GPU tests -- agrees with a plain per-env Python loop."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import helpers
from pgtg_amd import _abi, build
from pgtg_amd.rollout import COST_AHEAD, COST_BLOCK, cost_reference

F = np.float32
HEADER = os.path.join(helpers.ROOT, "include", "pgtg.h")


def test_library_exports_the_cost_entry_points():
    syms = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    have = set(re.findall(r" T (pgtg_\w+)", syms))
    for name in ("pgtg_set_flat_cost", "pgtg_cost_workspace_bytes", "pgtg_cost_scan"):
        assert name in have and name in _abi.EXPORTED
        assert getattr(_abi.lib(), name).argtypes is not None
    assert _abi.PGTG_ABI_VERSION == 9 and "#define PGTG_ABI_VERSION 9" in open(HEADER).read()


def test_ctypes_mirrors_match_the_header():
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "pgtg.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(PgtgCostSummary), offsetof(PgtgCostSummary, cost_max),
         offsetof(PgtgCostSummary, lambda_after), sizeof(PgtgCost), offsetof(PgtgCost, rewards), offsetof(PgtgCost, lambda),
         offsetof(PgtgCost, cost_limit), offsetof(PgtgCost, summary), offsetof(PgtgCost, workspace));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), "-o", os.path.join(d, "p"), os.path.join(d, "p.c")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    S, A = _abi.PgtgCostSummary, _abi.PgtgCost
    assert got == [C.sizeof(S), S.cost_max.offset, S.lambda_after.offset, C.sizeof(A), A.rewards.offset, A.lambda_.offset,
                   A.cost_limit.offset, A.summary.offset, A.workspace.offset]
    assert C.sizeof(S) == 40 and C.sizeof(A) == 16 + 6 * 8 + 3 * 8 + 2 * 8


def test_constants_are_the_kernels():
    src = open(os.path.join(helpers.ROOT, "pgtg_amd", "csrc", "pgtg_cost.h")).read()
    assert int(re.search(r"constexpr int kCostAhead = (\d+);", src).group(1)) == COST_AHEAD
    assert int(re.search(r"constexpr int kCostBlock = (\d+);", src).group(1)) == COST_BLOCK


def test_workspace_bytes_without_a_device():
    L = _abi.lib()
    n = C.c_uint64(7)
    assert L.pgtg_cost_workspace_bytes(1000, None) == _abi.PGTG_E_INVALID
    assert L.pgtg_cost_workspace_bytes(0, C.byref(n)) == _abi.PGTG_OK and n.value == 0
    for envs, rows in ((1, 1), (256, 1), (257, 2), (65536, 256)):
        assert L.pgtg_cost_workspace_bytes(envs, C.byref(n)) == _abi.PGTG_OK and n.value == rows * 24


def _random(T, N, seed, rate=0.2, exact=False):
    rng = np.random.default_rng(seed)
    rewards = (rng.standard_normal((T, N)) * 10).astype(F)
    costs = (rng.integers(0, 512, (T, N)) / 8).astype(F) if exact else (rng.random((T, N)) * 7).astype(F)
    dones = rng.random((T + 1, N)) < rate
    carry = (rng.integers(0, 64, N) / 8).astype(np.float64) if exact else rng.random(N) * 3
    return rewards, costs, dones, carry


def _loop(rewards, costs, dones, carry, lam, cost_limit, lambda_lr, lambda_max):
    """The definition, one env at a time in plain Python (the sum over episodes in (env, step) order)."""
    T, N = rewards.shape
    lam = F(lam)
    pen = np.zeros((T, N), F)
    new = np.zeros(N)
    eps = []
    for e in range(N):
        acc = float(carry[e])
        for t in range(T):
            pen[t, e] = F(rewards[t, e] - F(lam * costs[t, e]))
            acc += float(costs[t, e])
            if dones[t + 1, e]:
                eps.append(acc)
                acc = 0.0
        new[e] = acc
    nxt = lam
    if eps:
        l = float(lam) + lambda_lr * (sum(eps) / len(eps) - cost_limit)
        nxt = F(min(max(l, 0.0), lambda_max))
    return pen, new, eps, nxt


def test_cost_reference_against_the_plain_loop():
    for T, N, seed in ((1, 1, 1), (5, 3, 2), (17, 65, 3), (9, 300, 4), (3, 600, 5)):
        for exact in (True, False):
            d = _random(T, N, seed, exact=exact)
            pen, carry, eps, summary, nxt = cost_reference(*d, lam=0.375, cost_limit=3.0, lambda_lr=0.25, lambda_max=50.0)
            w_pen, w_carry, w_eps, w_nxt = _loop(*d, 0.375, 3.0, 0.25, 50.0)
            assert pen.dtype == F and np.array_equal(pen.view(np.int32), w_pen.view(np.int32))
            assert np.array_equal(carry, w_carry)
            assert np.array_equal(eps, np.array(w_eps))
            assert summary["episodes"] == len(w_eps) and summary["lambda_before"] == F(0.375)
            assert summary["lambda_after"] == nxt and nxt.dtype == F
            if w_eps:
                assert summary["cost_max"] == max(w_eps)
            if exact:  # every fp64 sum of multiples of 1/8 is exact in any order
                assert summary["cost_sum"] == sum(w_eps) and nxt == w_nxt
                assert summary["cost_mean"] == (sum(w_eps) / len(w_eps) if w_eps else 0.0)
            else:  # the tree's order is not the loop's: an fp64 sum of non-negative terms in any order
                bound = len(w_eps) * 2.0 ** -52 * sum(w_eps)
                assert abs(summary["cost_sum"] - sum(w_eps)) <= bound
                assert abs(float(nxt) - float(w_nxt)) <= 0.25 * bound / max(len(w_eps), 1) + np.spacing(w_nxt)


def test_the_carry_joins_two_rollouts_into_one():
    T, N = 11, 70
    rewards, costs, dones, carry = _random(2 * T, N, 9, exact=True)
    _, c1, e1, s1, _ = cost_reference(rewards[:T], costs[:T], dones[:T + 1], carry, 0.5, 1.0, 0.125, 10.0)
    _, c2, e2, s2, _ = cost_reference(rewards[T:], costs[T:], dones[T:], c1, 0.5, 1.0, 0.125, 10.0)
    _, c, e, s, _ = cost_reference(rewards, costs, dones, carry, 0.5, 1.0, 0.125, 10.0)
    assert np.array_equal(c2, c)
    assert s1["episodes"] + s2["episodes"] == s["episodes"] > 0
    assert sorted(np.concatenate([e1, e2]).tolist()) == sorted(e.tolist())
    assert s1["cost_sum"] + s2["cost_sum"] == s["cost_sum"]
    assert (c1 != 0).any()  # (episodes did cross the cut)


def test_a_zero_multiplier_returns_the_rewards():
    rewards, costs, dones, carry = _random(6, 40, 10)
    rewards[0, 0], rewards[1, 1] = F(-0.0), F(np.inf)
    pen = cost_reference(rewards, costs, dones, carry, 0.0, 1.0, 0.05, 100.0)[0]
    assert np.array_equal(pen.view(np.int32), rewards.view(np.int32))


def test_the_update_clamps_at_zero_and_at_lambda_max():
    d = _random(8, 50, 11, exact=True)
    mean = cost_reference(*d, 1.0, 0.0, 0.0, 1.0)[3]["cost_mean"]
    assert mean > 1.0
    low = cost_reference(*d, lam=1.0, cost_limit=mean + 1000.0, lambda_lr=0.5, lambda_max=10.0)
    assert low[4] == F(0.0) and low[3]["lambda_after"] == F(0.0) and low[3]["lambda_before"] == F(1.0)
    high = cost_reference(*d, lam=1.0, cost_limit=0.0, lambda_lr=1000.0, lambda_max=10.0)
    assert high[4] == F(10.0)
    inside = cost_reference(*d, lam=1.0, cost_limit=mean - 1.0, lambda_lr=0.5, lambda_max=10.0)
    assert inside[4] == F(1.5)


def test_no_finished_episode_leaves_the_multiplier():
    rewards, costs, dones, carry = _random(8, 50, 12)
    dones[1:] = False
    _, new, eps, summary, nxt = cost_reference(rewards, costs, dones, carry, 2.5, 0.0, 1.0, 100.0)
    assert len(eps) == 0 and nxt == F(2.5)
    assert summary == dict(episodes=0, cost_sum=0.0, cost_mean=0.0, cost_max=0.0, lambda_before=F(2.5), lambda_after=F(2.5))
    want = carry.copy()
    for t in range(8):
        want = want + costs[t].astype(np.float64)
    assert np.array_equal(new, want)
