"""The reward normalisation of a rollout on synthetic device arrays: the HIP kernels k_ret_scan, k_ret_stats and
k_ret_apply (include/pgtg.h pgtg_reward_norm; pgtg_amd/csrc/pgtg_norm.h) against reward_norm_reference
(pgtg_amd/rollout.py), bit for bit, at every shape around the wave, the workgroup, the 256 partials a merge
round takes and the scan's ring of rows in flight."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
from pgtg_amd.rollout import NORM_AHEAD as P
from pgtg_amd.rollout import NORM_BLOCK, NORM_PARTIAL, NORM_RMS_INIT

pytestmark = pytest.mark.gpu

F = np.float32
NS = (1, 63, 64, 65, 255, 256, 257, 1000)  # partial waves, a full workgroup, partial workgroups
TS = (1, P - 1, P, P + 1, 2 * P, 2 * P + 1)  # below, at and above the ring, with a remainder
WIDE = NORM_BLOCK * NORM_PARTIAL + 1  # one partial more than a merge round of k_ret_stats takes
SHAPES = [(T, N) for N in NS for T in TS] + [(3, WIDE)]
GAMMA, EPS, CLIP = 0.99, 1e-8, 0.5  # (at 0.5 both bounds bind on rewards in +-200, and many stay inside)
OUT = ("normalised", "ret", "rms", "row_var")


@pytest.fixture(scope="module")
def handle():
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = PGTGVecEnv(2, device=0, random_map_width=3, random_map_height=3)  # (its batch size is not the rollouts')
    yield env
    env.close()


def _inputs(T, N, seed):
    """Rewards in +-200 with zeros among them, episode ends at a rate of 0.2, a carried return and a used state.
    Step 0 ends every env's episode and (T > 1) step 1 pays every env the same, so its returns are identical and
    their batch variance exactly 0; the last step (T > 1) ends no episode."""
    rng = np.random.default_rng(seed)
    rewards = (rng.random((T, N)) * 400 - 200).astype(F)
    rewards[rng.random((T, N)) < 0.25] = 0
    dones = rng.random((T + 1, N)) < 0.2
    dones[1] = True
    if T > 1:
        rewards[1] = 3.5
        dones[T] = False
    return dict(rewards=rewards, dones=dones, ret=rng.standard_normal(N) * 50 + 1,
                rms=np.array([rng.standard_normal() * 5, 900.0 * rng.random() + 1, 1000.0 * rng.random() + 1]))


def _workspace_bytes(env, n, steps):
    nbytes = C.c_uint64()
    assert env._lib.pgtg_reward_norm_workspace_bytes(n, steps, C.byref(nbytes)) == 0
    return nbytes.value


def _norm(env, d, gamma=GAMMA, epsilon=EPS, clip=CLIP, training=1, fill=None, null=None, shift=None, **over):
    """pgtg_reward_norm on device copies of d.  fill: the outputs start as this sentinel.  shift: a pointer moved by
    four bytes (the tensor has the room).  Returns (rc, outputs)."""
    from pgtg_amd import _abi
    T, N = d["rewards"].shape
    # every array is a fresh tensor of its own: a row in front of it, or behind it, is not the test's memory
    dev = {k: torch.as_tensor(np.ascontiguousarray(d[k])).cuda() for k in ("rewards", "dones", "ret", "rms")}
    sentinel = 0.0 if fill is None else fill
    dev["normalised"] = torch.full((T, N), sentinel, dtype=torch.float32, device="cuda")
    dev["row_var"] = torch.full((T + 1,), sentinel, dtype=torch.float64, device="cuda")  # (one spare word for shift)
    dev["workspace"] = torch.full((_workspace_bytes(env, N, T) + 8,), 0 if fill is None else int(fill), dtype=torch.uint8,
                                  device="cuda")
    if shift in ("ret", "rms"):
        dev[shift] = torch.cat([dev[shift], dev[shift][:1]])
    p = lambda k: None if k == null else C.c_void_p(dev[k].data_ptr() + (4 if k == shift else 0))  # noqa: E731
    a = _abi.PgtgRewardNorm(n=over.get("n", N), steps=over.get("steps", T), gamma=gamma, epsilon=epsilon, clip=clip,
                            training=training, rewards=p("rewards"), dones=p("dones"), returns=p("ret"), rms=p("rms"),
                            row_var=p("row_var"), normalised=p("normalised"), workspace=p("workspace"))
    env._bind_stream()
    rc = env._lib.pgtg_reward_norm(env._h, C.byref(a))
    torch.cuda.synchronize()
    out = {k: dev[k].cpu().numpy() for k in ("normalised", "ret", "rms", "workspace")}
    out["row_var"] = dev["row_var"].cpu().numpy()[:T]
    return rc, out


def _reference(d, gamma=GAMMA, epsilon=EPS, clip=CLIP, training=True):
    from pgtg_amd.rollout import reward_norm_reference
    return dict(zip(OUT, reward_norm_reference(d["rewards"], d["dones"], d["ret"], d["rms"], gamma, epsilon, clip, training)))


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32 if x.dtype == F else np.int64)


def _assert_equal(out, want, tag):
    for k in OUT:
        assert out[k].dtype == want[k].dtype and np.array_equal(_bits(out[k]), _bits(want[k])), (tag, k, out[k], want[k])


@pytest.mark.parametrize("T,N", SHAPES)
def test_matches_the_reference_bit_for_bit(handle, T, N):
    d = _inputs(T, N, seed=1000 * T + N)
    rc, out = _norm(handle, d, fill=3.0)
    assert rc == 0
    want = _reference(d)
    _assert_equal(out, want, (T, N))
    # what the inputs were built to produce, shown by the reference alone
    assert d["dones"][1].all() and (d["ret"] != 0).all()
    if T > 1:
        assert not d["dones"][T].any() and (N < 63 or (want["ret"] != 0).any())
    if T * N >= 64:
        assert (want["normalised"] == F(CLIP)).any() and (want["normalised"] == F(-CLIP)).any()
        assert (np.abs(want["normalised"]) < CLIP).any()


def test_identical_returns_have_no_batch_variance(handle):
    """All envs at the same return in every step (and so merges of equal means at every level of every tree)."""
    for T, N in ((3, 1), (4, 65), (2 * P + 1, 300), (3, WIDE)):
        d = dict(rewards=np.full((T, N), 7.0, F), dones=np.zeros((T + 1, N), bool), ret=np.full(N, 2.0),
                 rms=np.array([1.0, 4.0, 50.0]))
        d["dones"][2] = True
        rc, out = _norm(handle, d, gamma=0.5)
        want = _reference(d, gamma=0.5)
        assert rc == 0
        _assert_equal(out, want, (T, N))
        # update_from_moments with vb = 0 exactly, on the host in plain Python
        mean, var, count, r = 1.0, 4.0, 50.0, 2.0
        for t in range(T):
            r = r * 0.5 + 7.0
            delta, tot = r - mean, count + N
            mean, var, count = mean + delta * N / tot, (var * count + 0.0 * N + delta * delta * count * N / tot) / tot, tot
            assert out["row_var"][t] == var, (T, N, t)
            r = 0.0 if t == 1 else r
        assert out["rms"].tolist() == [mean, var, count]


def test_all_zero_rewards_from_the_initial_state(handle):
    for T, N in ((1, 1), (P + 1, 65), (3, 1000)):
        d = dict(rewards=np.zeros((T, N), F), dones=np.zeros((T + 1, N), bool), ret=np.zeros(N), rms=np.array(NORM_RMS_INIT))
        rc, out = _norm(handle, d, clip=10.0, fill=3.0)
        assert rc == 0
        _assert_equal(out, _reference(d, clip=10.0), (T, N))
        assert not out["normalised"].any() and not out["ret"].any()
        assert out["rms"][0] == 0.0 and 0.0 < out["rms"][1] < 1.0 and out["rms"][2] > T * N


def test_two_runs_give_the_same_bits(handle):
    d = _inputs(2 * P + 1, 1000, seed=8)
    _, a = _norm(handle, d, fill=3.0)
    _, b = _norm(handle, d, fill=3.0)
    for k in OUT + ("workspace",):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert not (a["normalised"] == 3.0).any()


def test_frozen_statistics_leave_the_state_untouched(handle):
    for T, N in ((1, 1), (P + 1, 257), (3, 1100)):
        d = _inputs(T, N, seed=11 * T + N)
        rc, out = _norm(handle, d, training=0, fill=3.0)
        assert rc == 0
        want = _reference(d, training=False)
        assert np.array_equal(_bits(out["normalised"]), _bits(want["normalised"]))
        assert np.array_equal(_bits(out["ret"]), _bits(d["ret"])) and np.array_equal(_bits(out["rms"]), _bits(d["rms"]))
        assert (out["row_var"] == 3.0).all() and (out["workspace"] == 3).all()  # (only k_ret_apply ran)
        assert (want["row_var"] == d["rms"][1]).all()


def test_a_second_call_continues_the_first(handle):
    T, N = P + 3, 300
    d = _inputs(2 * T, N, seed=5)
    first = dict(d, rewards=d["rewards"][:T], dones=d["dones"][:T + 1])
    rc, a = _norm(handle, first)
    assert rc == 0 and (a["ret"] != 0).any()  # (episodes cross the cut)
    second = dict(rewards=d["rewards"][T:], dones=d["dones"][T:], ret=a["ret"], rms=a["rms"])
    rc, b = _norm(handle, second)
    assert rc == 0
    want = _reference(d)
    assert np.array_equal(_bits(np.concatenate([a["normalised"], b["normalised"]])), _bits(want["normalised"]))
    assert np.array_equal(_bits(np.concatenate([a["row_var"], b["row_var"]])), _bits(want["row_var"]))
    assert np.array_equal(_bits(b["ret"]), _bits(want["ret"])) and np.array_equal(_bits(b["rms"]), _bits(want["rms"]))


def test_argument_errors_launch_nothing(handle):
    from pgtg_amd import _abi
    T, N = 7, 65
    d = _inputs(T, N, seed=9)
    nan, inf = float("nan"), float("inf")
    cases = [dict(steps=0), dict(epsilon=nan), dict(epsilon=inf), dict(epsilon=-1e-8), dict(clip=nan), dict(clip=inf),
             dict(clip=-1.0), dict(gamma=nan), dict(gamma=-0.01), dict(gamma=1.01)]
    cases += [dict(null=k) for k in ("rewards", "dones", "ret", "rms", "row_var", "normalised", "workspace")]
    cases += [dict(shift=k) for k in ("ret", "rms", "row_var", "workspace")]
    big = [dict(steps=1 << 31), dict(n=1 << 41), dict(n=1 << 33, steps=1 << 30)]  # (refused before any launch: never dereferenced)
    for kw in cases + big:
        rc, out = _norm(handle, d, fill=3.0, **kw)
        assert rc == (_abi.PGTG_E_UNSUPPORTED if kw in big else _abi.PGTG_E_INVALID), kw
        assert handle._lib.pgtg_last_error(handle._h).decode().startswith("pgtg_reward_norm"), kw
        assert (out["normalised"] == 3.0).all() and (out["row_var"] == 3.0).all() and (out["workspace"] == 3).all(), kw
        assert np.array_equal(out["ret"][:N], d["ret"]) and np.array_equal(out["rms"][:3], d["rms"]), kw
    # no envs: nothing to do
    rc, out = _norm(handle, d, fill=3.0, n=0)
    assert rc == 0 and (out["normalised"] == 3.0).all() and np.array_equal(out["rms"], d["rms"])
    # the ends of the ranges are inside them, and the same call without the fault runs
    for kw in (dict(gamma=0.0), dict(gamma=1.0), dict(epsilon=0.0), dict(clip=0.0), {}):
        rc, out = _norm(handle, d, fill=3.0, **kw)
        assert rc == 0 and not (out["normalised"] == 3.0).any(), kw
        _assert_equal(out, _reference(d, **kw), kw)
