"""The host side of the rollout's reward normalisation, no GPU: the library exports the entry points within ABI
9, the ctypes mirror matches the header, the constants are the kernels', and reward_norm_reference
(pgtg_amd/rollout.py) -- the numpy restatement of k_ret_scan, k_ret_stats and k_ret_apply, the yardstick of the
GPU tests -- agrees with SB3's VecNormalize loop written plainly (np.mean and np.var per step)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import helpers
from pgtg_amd import _abi, build
from pgtg_amd.rollout import NORM_AHEAD, NORM_BLOCK, NORM_PARTIAL, NORM_RMS_INIT, reward_norm_reference

F = np.float32
HEADER = os.path.join(helpers.ROOT, "include", "pgtg.h")
NS, TS = (1, 5, 64, 300), (1, 9, 40)
GAMMA, EPS, CLIP = 0.99, 1e-8, 10.0
# 16 x the largest relative difference measured on the inputs below (see the test), and never looser than 1e-10
MEASURED = 3.84e-15
BOUND = min(16 * MEASURED, 1e-10)


def test_library_exports_the_norm_entry_points():
    syms = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    have = set(re.findall(r" T (pgtg_\w+)", syms))
    for name in ("pgtg_reward_norm_workspace_bytes", "pgtg_reward_norm"):
        assert name in have and name in _abi.EXPORTED
        assert getattr(_abi.lib(), name).argtypes is not None
    assert _abi.PGTG_ABI_VERSION == 9 and "#define PGTG_ABI_VERSION 9" in open(HEADER).read()


def test_ctypes_mirror_matches_the_header():
    fields = [name for name, _ in _abi.PgtgRewardNorm._fields_]
    assert fields == ["n", "steps", "gamma", "epsilon", "clip", "training", "rewards", "dones", "returns", "rms", "row_var",
                      "normalised", "workspace"]
    offs = ", ".join(f"offsetof(PgtgRewardNorm, {f})" for f in fields)
    probe = ('#include <stdio.h>\n#include <stddef.h>\n#include "pgtg.h"\nint main(void) {\n'
             '  size_t v[] = {sizeof(PgtgRewardNorm), %s};\n'
             '  for (unsigned i = 0; i < sizeof v / sizeof *v; i++) printf("%%zu ", v[i]);\n  return 0;\n}\n' % offs)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.run(["gcc", "-I", os.path.dirname(HEADER), "-o", os.path.join(d, "p"), os.path.join(d, "p.c")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    A = _abi.PgtgRewardNorm
    assert got == [C.sizeof(A)] + [getattr(A, f).offset for f in fields]
    assert C.sizeof(A) == 2 * 8 + 3 * 8 + 8 + 7 * 8  # (the int32 is padded to the pointers' alignment)


def test_constants_are_the_kernels():
    src = open(os.path.join(helpers.ROOT, "pgtg_amd", "csrc", "pgtg_norm.h")).read()
    for name, value in (("kNormBlock", NORM_BLOCK), ("kNormPartial", NORM_PARTIAL), ("kNormAhead", NORM_AHEAD)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == value
    assert NORM_PARTIAL == 64 and NORM_BLOCK % NORM_PARTIAL == 0
    assert NORM_RMS_INIT == (0.0, 1.0, 1e-4)


def test_workspace_bytes_and_the_handle_check_without_a_device():
    L = _abi.lib()
    n = C.c_uint64(7)
    assert L.pgtg_reward_norm_workspace_bytes(1000, 4, None) == _abi.PGTG_E_INVALID
    assert L.pgtg_reward_norm_workspace_bytes(1 << 41, 4, C.byref(n)) == _abi.PGTG_E_INVALID
    assert L.pgtg_reward_norm_workspace_bytes(1 << 33, 1 << 30, C.byref(n)) == _abi.PGTG_E_UNSUPPORTED and n.value == 7
    assert L.pgtg_reward_norm_workspace_bytes(0, 5, C.byref(n)) == _abi.PGTG_OK and n.value == 0
    # per step one 24-byte (n, mean, M2) per wave of 64 envs, and one for the step as a whole
    for envs, steps, parts in ((1, 1, 1), (64, 3, 1), (65, 3, 2), (300, 40, 5), (16385, 3, 257), (65536, 128, 1024)):
        assert L.pgtg_reward_norm_workspace_bytes(envs, steps, C.byref(n)) == _abi.PGTG_OK
        assert n.value == steps * (parts + 1) * 24, (envs, steps)
    # every other argument check reports through a handle, and a handle needs a device: without one the call
    # is refused before anything is read
    a = _abi.PgtgRewardNorm(n=4, steps=0)
    assert L.pgtg_reward_norm(None, C.byref(a)) == _abi.PGTG_E_INVALID


def _inputs(T, N, seed):
    """Rewards in +-200 with runs of zeros, episode ends at a rate of 0.1, a carried return and a used state."""
    rng = np.random.default_rng(seed)
    rewards = (rng.random((T, N)) * 400 - 200).astype(F)
    rewards[rng.random((T, N)) < 0.3] = 0
    for t in range(0, T, 7):  # runs of zeros: whole rows, and whole columns of three steps
        rewards[t] = 0
    rewards[T // 2:T // 2 + 3, ::3] = 0
    dones = rng.random((T + 1, N)) < 0.1
    ret = rng.standard_normal(N) * 50
    rms = np.array([rng.standard_normal() * 5, 900.0 * rng.random() + 1, 1000.0 * rng.random() + 1])
    return rewards, dones, ret, rms


def _sb3(rewards, dones, ret, rms, gamma, epsilon, clip, training=True):
    """VecNormalize's reward half as SB3 writes it: np.mean / np.var of the returns of a step, then
    RunningMeanStd.update_from_moments, then the clipped quotient."""
    T, N = rewards.shape
    ret = np.array(ret, dtype=np.float64)
    mean, var, count = (float(x) for x in rms)
    out = np.empty((T, N), F)
    row_var = np.empty(T)
    for t in range(T):
        if training:
            ret = ret * gamma + rewards[t].astype(np.float64)
            mb, vb, nb = float(np.mean(ret)), float(np.var(ret)), float(N)
            delta = mb - mean
            tot = count + nb
            new_mean = mean + delta * nb / tot
            m2 = var * count + vb * nb + np.square(delta) * count * nb / tot
            mean, var, count = new_mean, float(m2 / tot), tot
        row_var[t] = var
        out[t] = np.clip(rewards[t].astype(np.float64) / np.sqrt(var + epsilon), -clip, clip).astype(F)
        if training:
            ret[dones[t + 1]] = 0.0
    return out, ret, np.array([mean, var, count]), row_var


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny)))


def _ulps(a, b):
    """Distance in float32 steps (finite values of any sign)."""
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32), x.view(np.int32)).astype(np.int64)  # noqa: E731
    return np.abs(key(np.ascontiguousarray(a)) - key(np.ascontiguousarray(b)))


def test_reference_against_the_plain_sb3_loop():
    """The two differ in the order of the sums over the envs alone: pairwise trees of count-aware merges against
    np.mean and np.var.  Largest relative difference of mean, var and row_var measured over these twelve shapes, a
    used and the initial state: 3.84e-15 (N = 64, T = 9, the used state; 6.7e-16 at N = 300, T = 40); asserted:
    16 x that, 6.1e-14.  normalised: within one float32 step everywhere, equal where the clip binds (each
    shape runs once more with clip = 1, where it binds on both sides)."""
    worst = 0.0
    for N in NS:
        for T in TS:
            for fresh, clip in ((False, CLIP), (True, CLIP), (False, 1.0)):  # (at 1.0 the clip binds often)
                rewards, dones, ret, rms = _inputs(T, N, seed=100 * T + N)
                if fresh:
                    ret, rms = np.zeros(N), np.array(NORM_RMS_INIT)
                got = reward_norm_reference(rewards, dones, ret, rms, GAMMA, EPS, clip, True)
                want = _sb3(rewards, dones, ret, rms, GAMMA, EPS, clip)
                assert got[0].dtype == F and got[0].shape == (T, N) and got[3].shape == (T,)
                assert np.array_equal(got[1], want[1])  # (the returns: no sum over the envs in them)
                assert got[2][2] == want[2][2]  # (the counts: N added T times in both)
                rel = max(_rel(got[2][0], want[2][0]), _rel(got[2][1], want[2][1]), _rel(got[3], want[3]))
                print(N, T, fresh, "rel", rel)
                worst = max(worst, rel)
                assert rel <= BOUND, (N, T, fresh, rel)
                assert int(_ulps(got[0], want[0]).max()) <= 1, (N, T, fresh)
                bound = np.abs(want[0]) == F(clip)
                assert np.array_equal(got[0][bound], want[0][bound])
                if clip == 1.0 and N > 1 and T > 1:
                    assert (want[0] == F(clip)).any() and (want[0] == F(-clip)).any() and (np.abs(want[0]) < clip).any()
    print("worst", worst)
    assert BOUND <= 1e-10


def test_frozen_statistics_divide_every_row_by_the_stored_variance():
    rewards, dones, ret, rms = _inputs(9, 70, seed=3)
    out, new_ret, new_rms, row_var = reward_norm_reference(rewards, dones, ret, rms, GAMMA, EPS, CLIP, False)
    assert np.array_equal(new_ret, ret) and np.array_equal(new_rms, rms) and (row_var == rms[1]).all()
    want = _sb3(rewards, dones, ret, rms, GAMMA, EPS, CLIP, training=False)[0]
    assert np.array_equal(out.view(np.int32), want.view(np.int32))


def test_the_carried_state_joins_two_rollouts_into_one():
    T, N = 11, 130
    rewards, dones, ret, rms = _inputs(2 * T, N, seed=5)
    a = reward_norm_reference(rewards[:T], dones[:T + 1], ret, rms, GAMMA, EPS, CLIP)
    b = reward_norm_reference(rewards[T:], dones[T:], a[1], a[2], GAMMA, EPS, CLIP)
    w = reward_norm_reference(rewards, dones, ret, rms, GAMMA, EPS, CLIP)
    assert np.array_equal(np.concatenate([a[0], b[0]]).view(np.int32), w[0].view(np.int32))
    assert np.array_equal(b[1], w[1]) and np.array_equal(b[2], w[2]) and np.array_equal(np.concatenate([a[3], b[3]]), w[3])
    assert (a[1] != 0).any()  # (episodes did cross the cut)


def test_identical_returns_and_all_zero_rewards():
    # every env the same: the batch variance is exactly 0 and the mean exactly the value
    T, N = 3, 200
    rewards = np.full((T, N), 7.0, F)
    dones = np.zeros((T + 1, N), bool)
    out, ret, rms, row_var = reward_norm_reference(rewards, dones, np.full(N, 2.0), (1.0, 4.0, 50.0), 0.5, 0.0, 10.0)
    want = _sb3(rewards, dones, np.full(N, 2.0), (1.0, 4.0, 50.0), 0.5, 0.0, 10.0)
    assert np.array_equal(rms, want[2]) and np.array_equal(row_var, want[3]) and np.array_equal(out, want[0])
    # all-zero rewards from the initial state: the returns stay 0, the variance shrinks towards 0 and the output is 0
    out, ret, rms, row_var = reward_norm_reference(np.zeros((T, N), F), dones, np.zeros(N), NORM_RMS_INIT, 0.99)
    assert not out.any() and not ret.any() and rms[0] == 0.0 and 0.0 < rms[1] < 1e-6 and rms[2] == 1e-4 + T * N


@pytest.mark.parametrize("N", (1, 63, 64, 65, 257, 16385))
def test_the_tree_counts_every_env_once(N):
    rewards = np.ones((2, N), F)
    dones = np.zeros((3, N), bool)
    _, ret, rms, _ = reward_norm_reference(rewards, dones, np.zeros(N), (0.0, 1.0, 0.0), 1.0)
    assert (ret == 2.0).all() and rms[2] == 2 * N and rms[0] == 1.5 and rms[1] == 0.25
