"""pgtg_step_many on a k_envq handle: several ticks per launch (k_envq<BIG, true>) against a launch per tick.

Both handles of a comparison are forced onto the persistent map-queue kernel with 16 envs per workgroup
and a grid smaller than the number of blocks (tune queue_mode 1, envs_per_block 16, queue_grid), so that
workgroups own several blocks, unequal numbers of them, and a partial last block; they differ only in
tune step_ticks (1: a launch per tick).  After every call all outputs, the state blob and the per-env
digests must be equal bit for bit, the window must have ended episodes and generated maps, and the handles'
launch counts show which path each took.  (A state dump fills every ring and drops the pending requests,
on both handles alike, so the launch after it finds empty lists.)"""
import numpy as np
import pytest
import torch

import helpers  # noqa: F401
from digest_parity import ACT_SEED, _spec
from oracle import oracle
from test_gpu_state import _sections

pytestmark = pytest.mark.gpu

N_SMALL = 16 * 70 + 5  # 71 blocks, the last one of 5 envs
SPEC3 = dict(random_map_width=3, random_map_height=3)


def _tune(grid, step_ticks=None, envs_per_block=16):
    t = dict(queue_mode=1, envs_per_block=envs_per_block, queue_grid=grid)
    if step_ticks is not None:
        t["step_ticks"] = step_ticks
    return t


def _pair(spec, n, grid, step_ticks=None, seed=11, envs_per_block=16, **kw):
    """(several ticks per launch, a launch per tick), both reset with the same seed; kw: PGTGVecEnv's"""
    from pgtg_amd.vector import PGTGVecEnv
    a = PGTGVecEnv(n, spec=spec, device=0, tune=_tune(grid, step_ticks, envs_per_block), **kw)
    b = PGTGVecEnv(n, spec=spec, device=0, tune=_tune(grid, 1, envs_per_block), **kw)
    for e in (a, b):
        e.reset(seed=seed)
        assert "k_envq" in e.step_kernel(), e.step_kernel()
    return a, b


class _Window:
    """counters of a handle at the start of a compared window"""

    def __init__(self, env):
        self.env, self.c0, self.m0, self.l0 = env, env.counters(), env.queue_maps(), env.step_launches()

    def check_busy(self, tag, launches):
        """episodes ended, maps were generated, and the window took `launches` step-kernel launches"""
        c, m = self.env.counters(), self.env.queue_maps()
        assert c[1] > self.c0[1], f"{tag}: no episode ended in the window"
        assert m > self.m0, f"{tag}: no map was generated in the window"
        assert self.env.step_launches() - self.l0 == launches, (tag, self.env.step_launches() - self.l0, launches)


def _warm(a, b, ticks, seed):
    """single steps on both handles, so that the compared windows start in mid-episode with requests pending"""
    acts = a.random_actions(ticks, seed)
    for t in range(ticks):
        a.step_actions(acts[t])
        b.step_actions(acts[t])


def _assert_same(a, b, tag, state=True):
    from pgtg_amd.digest import Digest
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(a._bound_tensors(), b._bound_tensors())):
        assert torch.equal(x, y), f"{tag}: output {k} differs at {torch.nonzero(x != y)[:4].tolist()}"
    da, db = Digest(a).step_digest(), Digest(b).step_digest()
    assert torch.equal(da, db), f"{tag}: digests differ"
    assert a.counters() == b.counters(), tag
    assert a.queue_maps() == b.queue_maps(), tag
    assert a.error_count() == b.error_count() and a.error_count()[0] == 0, (tag, a.error_count())
    if state:
        sa, sb = a.dump_state(), b.dump_state()
        assert sa.size == sb.size, tag
        diff = [sec for sec, (x, y) in _sections(sa, sb).items() if not np.array_equal(x, y)]
        assert not diff, f"{tag}: state sections differ: {diff}"  # (the blob's alignment gaps are not compared)


@pytest.mark.parametrize("grid", [8, 64])  # 9 or 8 blocks per workgroup; 2 or 1 (the same block tick after tick)
def test_ticks_in_one_launch_equal_a_launch_per_tick(grid):
    """K = 1, 2, 3, 7 and 13 ticks per call: every phase of the two list buffers and the three rotating
    sets, and more than two episode ends per env.  Six single steps come first: the call of one tick
    serves the requests of the last of them (a call of one tick is a launch per tick on both handles), and
    every later call follows a state dump, so each of them is one launch of K ticks: a map generated in
    a window of two ticks was requested in its first tick and made in its second, inside the launch."""
    a, b = _pair(_spec(SPEC3), N_SMALL, grid)
    try:
        _warm(a, b, 6, 0xBEF0)
        t0 = 0
        for K in (1, 2, 3, 7, 13):
            acts = a.random_actions(K, 0xF05E, t0=t0)
            wa, wb = _Window(a), _Window(b)
            a.step_many(acts)
            b.step_many(acts)
            wa.check_busy(f"K {K}", 1)
            wb.check_busy(f"K {K}", K)
            _assert_same(a, b, f"grid {grid} K {K}")
            t0 += K
        assert a.counters()[1] > 2 * N_SMALL, "fewer than two episode ends per env"
    finally:
        a.close()
        b.close()


def test_launches_cut_at_step_ticks():
    """step_ticks 3 and K = 7: launches of 3 + 3 + 1 ticks, the request lists handed from one to the next.
    Three calls: a state dump lies between the first and the second, none between the second and the
    third, whose first launch serves the list of the second call's last."""
    a, b = _pair(_spec(SPEC3), N_SMALL, 8, step_ticks=3)
    try:
        _warm(a, b, 4, 0xBEF1)
        for rep in range(3):
            acts = a.random_actions(7, 0xC07, t0=7 * rep)
            wa, wb = _Window(a), _Window(b)
            a.step_many(acts)
            b.step_many(acts)
            # (after the single steps the first call's first launch is one tick alone: 1 + 3 + 3)
            wa.check_busy(f"cut rep {rep}", 3)
            wb.check_busy(f"cut rep {rep}", 7)
            _assert_same(a, b, f"cut rep {rep}", state=rep != 1)
    finally:
        a.close()
        b.close()


def test_hand_over_to_and_from_single_steps():
    """step_many(5), one step_actions, a masked reset, step_many(4), one step_actions, step_many(6): the
    list rotation handed over in both directions, the write-every-line flag on a first tick, and a
    launch per tick's lists served by the first launch that follows."""
    a, b = _pair(_spec(SPEC3), N_SMALL, 8)
    try:
        acts = a.random_actions(17, 0xAB5)
        mask = torch.zeros(N_SMALL, dtype=torch.uint8, device="cuda")
        mask[::3] = 1
        wa, wb = _Window(a), _Window(b)
        for e in (a, b):
            e.step_many(acts[0:5])
            e.step_actions(acts[5])
        _assert_same(a, b, "after 5 + 1", state=False)
        for e in (a, b):
            e.reset(mask=mask)
            e.step_many(acts[6:10])
        _assert_same(a, b, "after the masked reset + 4", state=False)
        for e in (a, b):
            e.step_actions(acts[10])
            e.step_many(acts[11:17])
        # a: 1 launch of 5 ticks, a step, 1 launch of 4 (the reset emptied the lists), a step, then 1 + 5 ticks
        wa.check_busy("hand-over", 6)
        wb.check_busy("hand-over", 17)
        _assert_same(a, b, "after 1 + 6")
    finally:
        a.close()
        b.close()


def test_against_the_restatement_5x5():
    """4 096 envs on 5x5 maps, 12 ticks in calls of 5 and 7: every env's digest after each call against the
    CPU restatement's."""
    from pgtg_amd.digest import Digest
    from pgtg_amd.vector import PGTGVecEnv
    spec, n, T = _spec(dict(random_map_width=5, random_map_height=5)), 4096, 12
    ref, flags = oracle.rollout_digest(spec, n, T, ACT_SEED, flags_out=True)
    assert (flags != 0).sum() > 0, "no episode ends in the restatement's window"
    env = PGTGVecEnv(n, spec=spec, device=0, autoreset=True, tune=_tune(24))  # 256 blocks: 11 or 10 per workgroup
    try:
        env.reset(seed=0)
        assert "k_envq" in env.step_kernel()
        acts = env.random_actions(T, ACT_SEED)
        dg, w = Digest(env), _Window(env)
        for lo, hi in ((0, 5), (5, 12)):
            env.step_many(acts[lo:hi])
            got = dg.step_digest().cpu().numpy().view(np.uint64)
            bad = np.argwhere(got != ref[hi - 1])
            assert bad.size == 0, f"tick {hi - 1}: {len(bad)} env digests differ, first {bad[:8].ravel().tolist()}"
        w.check_busy("5x5", 2)
        assert env.counters()[1] - w.c0[1] == int((flags != 0).sum())  # episodes ended in the 12 ticks
        assert env.error_count()[0] == 0
    finally:
        env.close()


def test_per_launch_timing_keeps_a_launch_per_tick():
    """With per-launch timing on, step_many queues a launch per tick (every one of them timed); outputs and
    the maps-generated counter are those of the other path."""
    a, b = _pair(_spec(SPEC3), N_SMALL, 8)
    try:
        K = 9
        acts = a.random_actions(K, 0x71E)
        a.enable_timing(1)
        wa, wb = _Window(a), _Window(b)
        a.step_many(acts)
        b.step_many(acts)
        wa.check_busy("timed", K)
        wb.check_busy("timed", K)
        assert a.timing_read()[1] == K
        _assert_same(a, b, "timed")
        # timing off again: several ticks per launch, still equal
        a.enable_timing(0)
        more = a.random_actions(K, 0x71E, t0=K)
        wa = _Window(a)
        a.step_many(more)
        b.step_many(more)
        wa.check_busy("timing off again", 1)
        _assert_same(a, b, "timing off again")
    finally:
        a.close()
        b.close()
