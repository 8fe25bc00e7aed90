"""The host side of the device rollout buffer, no GPU: the library exports pgtg_gae within ABI 9, the
ctypes mirror of PgtgGae matches the header, and gae_reference / sample_index (pgtg_amd/rollout.py) agree
with an independent scalar loop, with closed forms and with SB3's sample order."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
from pgtg_amd import _abi, build
from pgtg_amd.rollout import gae_reference, sample_index

F = np.float32


def test_library_exports_pgtg_gae():
    syms = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    assert "pgtg_gae" in set(re.findall(r" T (pgtg_\w+)", syms))
    assert "pgtg_gae" in _abi.EXPORTED
    assert _abi.lib().pgtg_gae.argtypes is not None


def test_gae_struct_matches_the_header_and_abi_stays_9():
    src = open(os.path.join(helpers.ROOT, "include", "pgtg.h")).read()
    assert re.search(r"^#define PGTG_ABI_VERSION 9$", src, re.M) and _abi.PGTG_ABI_VERSION == 9
    body = re.search(r"typedef struct \{([^}]*)\} PgtgGae;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"^\W+", "", d.split()[-1]) for stmt in body.split(";") for d in stmt.split(",") if d.strip()]
    assert names == [f for f, _ in _abi.PgtgGae._fields_]
    # two uint64, two doubles, eight pointers
    assert C.sizeof(_abi.PgtgGae) == 16 + 16 + 8 * C.sizeof(C.c_void_p) == 96
    assert _abi.PgtgGae.gamma.offset == 16 and _abi.PgtgGae.rewards.offset == 32
    assert _abi.PgtgGae.returns.offset == 88
    assert re.search(r"int pgtg_gae\(pgtg_handle\* h, const PgtgGae\* a\);", src)


def _scalar_gae(rew, val, dones, tonly, tval, last_values, gamma, gae_lambda, gl=None):
    """Per env, explicit np.float32 operations in the order of include/pgtg.h."""
    T, N = rew.shape
    g = F(gamma)
    gl = F(gamma * gae_lambda) if gl is None else gl
    adv, ret = np.zeros((T, N), F), np.zeros((T, N), F)
    for e in range(N):
        last = F(0)
        for t in range(T - 1, -1, -1):
            r = F(rew[t, e])
            if tonly is not None and tonly[t, e]:
                r = F(r + F(g * F(tval[t, e])))
            nnt = F(F(1) - F(dones[t + 1, e] != 0))
            nv = F(last_values[e]) if t == T - 1 else F(val[t + 1, e])
            delta = F(F(r + F(F(g * nv) * nnt)) - F(val[t, e]))
            last = F(delta + F(F(gl * nnt) * last))
            adv[t, e] = last
            ret[t, e] = F(last + F(val[t, e]))
    return adv, ret


def _inputs(T, N, seed, done_rate=0.3):
    rng = np.random.default_rng(seed)
    rew = (rng.standard_normal((T, N)) * 100).astype(F)
    val = (rng.standard_normal((T, N)) * 100).astype(F)
    tval = (rng.standard_normal((T, N)) * 100).astype(F)
    last = (rng.standard_normal(N) * 100).astype(F)
    dones = rng.random((T + 1, N)) < done_rate
    tonly = dones[1:] & (rng.random((T, N)) < 0.5)
    return rew, val, dones, tonly, tval, last


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


@pytest.mark.parametrize("T, N", [(1, 1), (2, 3), (7, 5), (33, 4)])
@pytest.mark.parametrize("gamma, lam", [(0.99, 0.95), (0.9, 0.95)])
def test_gae_reference_matches_the_scalar_loop(T, N, gamma, lam):
    rew, val, dones, tonly, tval, last = _inputs(T, N, seed=100 * T + N)
    keep = rew.copy()
    adv, ret = gae_reference(rew, val, dones, tonly, tval, last, gamma, lam)
    assert np.array_equal(rew, keep)  # (the bootstrap is applied to a copy)
    want_adv, want_ret = _scalar_gae(rew, val, dones, tonly, tval, last, gamma, lam)
    assert adv.dtype == ret.dtype == F
    assert np.array_equal(_bits(adv), _bits(want_adv)) and np.array_equal(_bits(ret), _bits(want_ret))
    # no bootstrap arrays = no truncated sample
    a0, r0 = gae_reference(rew, val, dones, None, None, last, gamma, lam)
    a1, r1 = gae_reference(rew, val, dones, np.zeros_like(tonly), tval, last, gamma, lam)
    assert np.array_equal(_bits(a0), _bits(a1)) and np.array_equal(_bits(r0), _bits(r1))


def test_returns_are_suffix_sums_without_discount():
    # gamma = lambda = 1, no dones, small integers: every float32 operation is exact, and
    # returns[t] = rewards[t] + ... + rewards[T-1] + last_values
    rng = np.random.default_rng(3)
    T, N = 12, 6
    rew = rng.integers(-9, 10, (T, N)).astype(F)
    val = rng.integers(-9, 10, (T, N)).astype(F)
    last = rng.integers(-9, 10, N).astype(F)
    dones = np.zeros((T + 1, N), bool)
    adv, ret = gae_reference(rew, val, dones, None, None, last, 1.0, 1.0)
    want = np.cumsum(rew[::-1], axis=0)[::-1] + last
    assert np.array_equal(ret, want.astype(F)) and np.array_equal(adv, (want - val).astype(F))


def test_a_done_cuts_the_scan_and_dones_row_0_is_unused():
    rng = np.random.default_rng(4)
    T, N, cut = 10, 4, 6
    rew = rng.integers(-9, 10, (T, N)).astype(F)
    val = rng.integers(-9, 10, (T, N)).astype(F)
    last = rng.integers(-9, 10, N).astype(F)
    dones = np.zeros((T + 1, N), bool)
    dones[cut + 1, 1] = True  # env 1's episode ends with step `cut`
    adv, ret = gae_reference(rew, val, dones, None, None, last, 1.0, 1.0)
    # rows 0 .. cut of env 1 see nothing after the cut: its own suffix sum up to `cut`, no next value
    want = np.cumsum(rew[cut::-1, 1])[::-1]
    assert np.array_equal(ret[:cut + 1, 1], want.astype(F))
    # ... exactly what a rollout that ends at the cut with a done gives
    d2 = np.zeros((cut + 2, N), bool)
    d2[cut + 1, 1] = True
    _, ret2 = gae_reference(rew[:cut + 1], val[:cut + 1], d2, None, None, val[cut + 1] * 0 + 77, 1.0, 1.0)
    assert np.array_equal(ret[:cut + 1, 1], ret2[:, 1])
    # the other envs are untouched by env 1's done
    free = gae_reference(rew, val, np.zeros_like(dones), None, None, last, 1.0, 1.0)[1]
    assert np.array_equal(np.delete(ret, 1, axis=1), np.delete(free, 1, axis=1))
    # dones[0] (the episode starts of step 0) enters nothing
    d3 = dones.copy()
    d3[0] = True
    a3, r3 = gae_reference(rew, val, d3, None, None, last, 1.0, 1.0)
    assert np.array_equal(_bits(a3), _bits(adv)) and np.array_equal(_bits(r3), _bits(ret))


@pytest.mark.parametrize("gamma, lam", [(0.9, 0.95), (0.99, 0.92)])
def test_gamma_lambda_is_rounded_once_from_the_double_product(gamma, lam):
    once, twice = F(gamma * lam), F(F(gamma) * F(lam))
    assert once != twice  # (the pair discriminates the two roundings)
    rew, val, dones, tonly, tval, last = _inputs(33, 4, seed=9, done_rate=0.1)
    adv, ret = gae_reference(rew, val, dones, tonly, tval, last, gamma, lam)
    a1, r1 = _scalar_gae(rew, val, dones, tonly, tval, last, gamma, lam, gl=once)
    a2, r2 = _scalar_gae(rew, val, dones, tonly, tval, last, gamma, lam, gl=twice)
    assert np.array_equal(_bits(adv), _bits(a1)) and np.array_equal(_bits(ret), _bits(r1))
    assert not np.array_equal(_bits(a2), _bits(a1))  # the other choice changes at least one output bit


@pytest.mark.parametrize("T, N", [(1, 1), (3, 5), (12, 7)])
def test_sample_index_is_swap_and_flatten_order(T, N):
    a = np.arange(T * N).reshape(T, N)
    flat = np.swapaxes(a, 0, 1).reshape(T * N)  # SB3's swap_and_flatten of a [T, N] array
    s = np.arange(T * N)
    e, t = sample_index(s, T)
    assert np.array_equal(a[t, e], flat)
    assert sample_index(T * N - 1, T) == (N - 1, T - 1)
