"""k_envq writes only the observation lines that changed; k_envb writes them all.

On the one-tile fast path without traffic an env's observation is a function of its tile, that tile's
plan word, its used-subgoal bit, the episode's start/goal word and the light colour (obs_key), so a
step launch that finds the bound obs buffer current writes the 128-byte lines of the envs whose key
changed (or that finished) and leaves the rest.  The tests poison the buffer behind the handle's back
(0xAA, which no observation byte holds) to see which bytes a launch wrote, with a twin handle and the
CPU restatement as references: the skip is live and exact, every call that makes the buffer stale is
followed by a full write, step_many equals single steps, and other configurations write everything.
k_envb keeps the parent's code (the delta write made its one- and two-round launches 2-6 % slower,
DESIGN.md 5k): its cases run the same checks and assert that no byte is left in place.

Shapes: 5*128+37 envs of 5x5 maps in blocks of 128 (one round, a partial last block, 729-byte rows that
straddle lines) on k_envq and on k_envb, and 3x3 maps in blocks of 16 over more than two rounds of
k_envq's persistent grid (the two alternating line masks)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
from digest_parity import ACT_SEED, _spec
from oracle import oracle

pytestmark = pytest.mark.gpu

CFG2 = dict(random_map_width=3, random_map_height=3)
CFG5 = dict(random_map_width=5, random_map_height=5)
K_ENVQ, K_ENVB = "pgtg::k_envq<false>", "pgtg::k_envb<false>"
N5 = 5 * 128 + 37
WARM, TICKS = 20, 10
POISON = 0xAA


def _make(n, conf, tune):
    from pgtg_amd.vector import PGTGVecEnv
    return PGTGVecEnv(n, spec=_spec(conf), device=0, autoreset=True, tune=tune)


@functools.lru_cache(maxsize=None)
def _rounds_n():
    """Envs for more than two rounds of k_envq's persistent grid in blocks of 16 (tests/test_gpu_plan_slot.py)"""
    probe = _make(64, CFG2, dict(envs_per_block=16, queue_mode=1))
    kern, shape, occ = probe.step_kernel(), probe.launch_info(), probe.occupancy()
    probe.close()
    assert kern == K_ENVQ and shape[0] == 16, (kern, shape)
    grid = min(occ * torch.cuda.get_device_properties(0).multi_processor_count, 4096)  # (kMaxQueueGrid)
    return 2 * grid * 16 + 5


def _case(name):
    """(envs, config, tune, step kernel)"""
    if name == "envq":
        return N5, CFG5, dict(envs_per_block=128, queue_mode=1), K_ENVQ
    if name == "envb":
        return N5, CFG5, dict(envs_per_block=128, queue_mode=2), K_ENVB
    return _rounds_n(), CFG2, dict(envs_per_block=16, queue_mode=1), K_ENVQ


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The restatement's digests [WARM + TICKS, n] of a case, computed once and shared."""
    n, conf, _, _ = _case(name)
    ref = oracle.rollout_digest(_spec(conf), n, WARM + TICKS, ACT_SEED)
    ref.setflags(write=False)
    return ref


def _digest(dg):
    return dg.step_digest().cpu().numpy().view(np.uint64)


def _pair(name):
    n, conf, tune, kern = _case(name)
    a, b = _make(n, conf, tune), _make(n, conf, tune)
    assert a.step_kernel() == kern and b.step_kernel() == kern, (a.step_kernel(), kern)
    a.reset(seed=0)
    b.reset(seed=0)
    return a, b


def _warm(a, b, ticks=WARM):
    for t in range(ticks):
        a.step_random(ACT_SEED, t)
        b.step_random(ACT_SEED, t)


@pytest.mark.parametrize("name", ["envq", "envb", "envq_rounds"])
def test_skip_is_live_and_exact(name):
    from pgtg_amd.digest import Digest
    ref = _ref(name)
    a, b = _pair(name)
    try:
        n = a.num_envs
        db = Digest(b)
        for t in range(WARM):
            a.step_random(ACT_SEED, t)
            b.step_random(ACT_SEED, t)
            assert np.array_equal(_digest(db), ref[t]), f"warm tick {t}"
        kept = total = 0
        for t in range(WARM, WARM + TICKS):
            before = a.obs_map.clone()
            b_before = b.obs_map.clone()
            a.obs_map.fill_(POISON)  # (behind the handle's back)
            a.step_random(ACT_SEED, t)
            b.step_random(ACT_SEED, t)
            left = a.obs_map == POISON
            assert torch.equal(torch.where(left, before, a.obs_map), b.obs_map), f"tick {t}: not the twin's observation"
            fresh = (b.terminated | b.truncated) | (b.obs_map != b_before).reshape(n, -1).any(dim=1)
            stale = left.reshape(n, -1).any(dim=1) & fresh
            assert not bool(stale.any()), f"tick {t}: envs {torch.nonzero(stale).flatten()[:8].tolist()} reset or changed and kept bytes"
            assert np.array_equal(_digest(db), ref[t]), f"tick {t}: the twin against the restatement"
            kept += int(left.sum())
            total += left.numel()
            a.obs_map.copy_(b.obs_map)  # (what the handle believes the buffer holds)
        print(f"{name}: {kept / total:.3f} of the observation bytes left in place over {TICKS} ticks")
        if a.step_kernel() == K_ENVB:
            assert kept == 0, f"k_envb left {kept} bytes in place"
        else:  # the restatement leaves about half in place; a factor of two for the small batch
            assert kept >= total / 4, f"{kept} of {total} bytes left in place"
        a.obs_map.fill_(POISON)
        a.observe()
        assert torch.equal(a.obs_map, b.obs_map), "observe()"
        assert a.error_count()[0] == 0 and b.error_count()[0] == 0
    finally:
        a.close()
        b.close()


def _rebind(env):
    new = torch.full_like(env.obs_map, POISON)
    env.obs_map = new
    env._outs.obs = new.data_ptr()
    rc = env._lib.pgtg_set_outputs(env._h, C.byref(env._outs))
    assert rc == 0, rc


def _masked_reset(env):
    mask = torch.zeros(env.num_envs, dtype=torch.uint8, device=env.device)
    mask[::3] = 1
    env.reset(seed=1234, mask=mask)


def _other_tile(env, i):
    """set_agent of env i into a neighbouring tile's centre (9 squares per tile)"""
    s = env.env_state(i)
    x, y = int(s["x"]), int(s["y"])
    tx = x // 9
    nx = (tx + 1 if tx + 1 < 5 else tx - 1) * 9 + 4
    env.set_agent(i, nx, (y // 9) * 9 + 4, 0, 0)


def _set_agent(env):
    for i in (0, 1, 130, env.num_envs - 1):
        _other_tile(env, i)


def _set_to_state(env):
    for i in (2, 131, env.num_envs - 2):
        s = env.env_state(i)
        x, y = int(s["x"]), int(s["y"])
        tx = x // 9
        env.set_to_state(i, (tx + 1 if tx + 1 < 5 else tx - 1) * 9 + 4, (y // 9) * 9 + 4, 0, 0, False)


_BLOB = {}


def _load_blob(env):
    # another batch's state (the same handle shape), loaded without the observe() the API asks for
    env.load_state(_BLOB[env.step_kernel()], observe=False)


def _load_snapshot(env):
    idx = list(range(0, env.num_envs, 7))
    src = [(i + 3) % env.num_envs for i in idx]
    snap = env.snapshot(len(idx))
    try:
        snap.save(env, env_idx=src, slot_idx=list(range(len(idx))))
        snap.load(env, slot_idx=list(range(len(idx))), env_idx=idx, observe=False)
    finally:
        snap.close()


CALLS = {"rebind": _rebind, "masked_reset": _masked_reset, "set_agent": _set_agent, "set_to_state": _set_to_state,
         "load_state": _load_blob, "snapshot_load": _load_snapshot}


@pytest.mark.parametrize("call", sorted(CALLS))
@pytest.mark.parametrize("name", ["envq", "envb"])
def test_invalidation(name, call):
    a, b = _pair(name)
    try:
        if call == "load_state" and a.step_kernel() not in _BLOB:
            n, conf, tune, _ = _case(name)
            other = _make(n, conf, tune)
            try:
                other.reset(seed=99)
                for t in range(7):
                    other.step_random(ACT_SEED, t)
                _BLOB[a.step_kernel()] = other.dump_state()
            finally:
                other.close()
        _warm(a, b)
        CALLS[call](a)
        CALLS[call](b)
        a.obs_map.fill_(POISON)
        a.step_random(ACT_SEED, WARM)
        b.step_random(ACT_SEED, WARM)
        assert not bool((a.obs_map == POISON).any()), f"{call}: bytes left in place"
        assert torch.equal(a.obs_map, b.obs_map), call
        b.obs_map.fill_(POISON)
        b.observe()
        assert torch.equal(a.obs_map, b.obs_map), f"{call}: observe()"
        if a.step_kernel() == K_ENVQ:  # and the launch after that one skips again
            a.obs_map.fill_(POISON)
            a.step_random(ACT_SEED, WARM + 1)
            assert bool((a.obs_map == POISON).any()), f"{call}: the step after the full write wrote every line"
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("name", ["envq", "envb"])
def test_step_many_gives_the_digests_of_single_steps(name):
    from pgtg_amd.digest import Digest
    ref = _ref(name)
    a, b = _pair(name)
    try:
        _warm(a, b, 5)
        acts = a.random_actions(5, ACT_SEED, t0=5)
        a.step_many(acts)
        da, db = Digest(a), Digest(b)
        for t in range(5):
            b.step_actions(acts[t])
        assert np.array_equal(_digest(da), _digest(db))
        assert np.array_equal(_digest(da), ref[9])
        assert torch.equal(a.obs_map, b.obs_map)
    finally:
        a.close()
        b.close()


def test_a_sliding_window_writes_every_line():
    conf = dict(CFG5, use_sliding_observation_window=True, sliding_observation_window_size=5)
    tune = dict(envs_per_block=128, queue_mode=1)
    a, b = _make(N5, conf, tune), _make(N5, conf, tune)
    try:
        assert a.step_kernel() == K_ENVQ, a.step_kernel()
        a.reset(seed=0)
        b.reset(seed=0)
        _warm(a, b, 5)
        a.obs_map.fill_(POISON)
        a.step_random(ACT_SEED, 5)
        b.step_random(ACT_SEED, 5)
        assert not bool((a.obs_map == POISON).any())
        assert torch.equal(a.obs_map, b.obs_map)
    finally:
        a.close()
        b.close()
