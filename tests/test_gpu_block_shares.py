"""k_envq<BIG, true> with block shares from a table against a launch per tick.

The shapes of test_gpu_step_fused.py: 1 125 3x3 envs in 71 blocks of 16 on queue grids of 8 and 64, and 128-env
workgroups on a grid of 4.  Handle `a` runs pgtg_step_many with forced, frozen shares that change between calls
(an env then moves to another workgroup with its refill request of the last tick already served: the drain) or
with the device's own shares; handle `b` runs a launch per tick.  After every call the outputs, digests,
counters, queue_maps and (where stated) the state sections must be equal, and the launch counts are asserted."""
import numpy as np
import pytest
import torch

import helpers  # noqa: F401
from digest_parity import _spec
from test_gpu_step_fused import N_SMALL, SPEC3, _assert_same, _pair, _warm, _Window

pytestmark = pytest.mark.gpu


def _layouts(grid, nblk, capb):
    """forced shares inside the request cap: all the cap allows on workgroup 0 and the rest spread; zeros on half
    the workgroups; alternating 1 and many; the last workgroup owning one block alone.  (The ranges are over the
    column order, block w + k * grid at place (w, k): the short tail block, the last of column (blocks - 1) % grid,
    falls inside another workgroup's range in every layout.)"""
    def spread(first, rest_n):
        rest = nblk - first
        c = np.full(rest_n, rest // rest_n, np.int64)
        c[:rest % rest_n] += 1
        return c
    heavy = np.concatenate([[min(capb, nblk - (grid - 1))], spread(min(capb, nblk - (grid - 1)), grid - 1)])
    half = np.zeros(grid, np.int64)
    half[::2] = spread(0, (grid + 1) // 2)
    alt = np.ones(grid, np.int64)
    alt[1::2] = spread(len(alt[::2]), grid // 2)
    tail = np.concatenate([spread(1, grid - 1), [1]])
    out = [heavy, half, alt, tail]
    for c in out:
        assert c.sum() == nblk and c.max() <= capb and len(c) == grid, c
    return out


@pytest.mark.parametrize("grid,n,epb,dump", [(8, N_SMALL, 16, False), (8, N_SMALL, 16, True), (64, N_SMALL, 16, False),
                                             (64, N_SMALL, 16, True), (4, 128 * 9 + 5, 128, False)])
def test_forced_shares_changing_between_calls(grid, n, epb, dump):
    """dump: the state sections compared after every call too (a dump fills the rings on both handles, so the
    rows without it are the ones where a call starts on what the drain of the call before left)"""
    a, b = _pair(_spec(SPEC3), n, grid, step_ticks=3 if grid == 8 else None, envs_per_block=epb)
    try:
        nblk = -(-n // epb)
        capb = 3 * -(-nblk // grid)
        assert a.block_shares().sum() == nblk
        lay = _layouts(grid, nblk, capb)
        _warm(a, b, 4, 0xB10C)
        t0, first = 0, True
        for k, K in enumerate((2, 5, 12, 7)):
            a.set_block_shares(lay[k % 4], freeze=True)
            assert np.array_equal(a.block_shares(), lay[k % 4])
            acts = a.random_actions(K, 0x5A5E, t0=t0)
            wa, wb = _Window(a), _Window(b)
            a.step_many(acts)
            b.step_many(acts)
            cut = 3 if grid == 8 else 64
            wa.check_busy(f"K {K}", 1 + -(-(K - 1) // cut) if first else -(-K // cut))  # (first: the hand-over tick)
            wb.check_busy(f"K {K}", K)
            first = False
            # no state dump between the calls: a dump would fill the rings and hide what the drain left
            _assert_same(a, b, f"grid {grid} layout {k} K {K}", state=dump)
            t0 += K
        _assert_same(a, b, f"grid {grid} end", state=True)
        assert a.counters()[1] > n, "fewer than one episode end per env"
    finally:
        a.close()
        b.close()


def test_hook_refuses_what_the_lists_cannot_hold():
    a, b = _pair(_spec(SPEC3), N_SMALL, 8)
    try:
        c = np.ones(8, np.int64)
        c[0] = 71 - 7  # above 3 x 9 blocks of requests
        for bad in (c, np.full(8, 9), np.full(7, 10)):
            with pytest.raises(Exception) as e:
                a.set_block_shares(bad)
            assert "INVALID" in str(e.value).upper() or "block shares" in str(e.value), str(e.value)
    finally:
        a.close()
        b.close()


def test_shares_changed_around_reset_single_step_and_state_load():
    a, b = _pair(_spec(SPEC3), N_SMALL, 8)
    try:
        lay = _layouts(8, 71, 27)
        acts = a.random_actions(24, 0xAB6)
        mask = torch.zeros(N_SMALL, dtype=torch.uint8, device="cuda")
        mask[::3] = 1
        a.set_block_shares(lay[0])
        for e in (a, b):
            e.step_many(acts[0:5])
        _assert_same(a, b, "first call", state=False)
        # a masked reset directly behind the multi-tick launch: the requests its drain served for the envs now
        # reset are not counted (a launch per tick drops them here)
        assert a.counters()[1] > 0
        for e in (a, b):
            e.reset(seed=77, mask=mask)
        _assert_same(a, b, "masked reset behind a drain", state=False)
        a.set_block_shares(lay[1])
        l0 = a.step_launches()
        for e in (a, b):
            e.step_many(acts[6:9])
        assert a.step_launches() - l0 == 1  # (a reset fills the rings and empties the lists: no hand-over tick)
        _assert_same(a, b, "after the masked reset", state=False)
        for e in (a, b):  # an unseeded reset of every env behind a drain
            e.reset()
        _assert_same(a, b, "full reset behind a drain", state=False)
        for e in (a, b):
            e.step_many(acts[9:11])
        _assert_same(a, b, "after the full reset", state=False)
        for e in (a, b):  # a single step: k_envq<BIG, false> serves nothing on a (drained), the last tick's list on b
            e.step_actions(acts[11])
        _assert_same(a, b, "single step", state=False)
        a.set_block_shares(lay[2])
        l0 = a.step_launches()
        for e in (a, b):
            e.step_many(acts[6:12])
        assert a.step_launches() - l0 == 2  # (the hand-over tick, then 5)
        _assert_same(a, b, "after the single step", state=False)
        blob = a.dump_state()
        b.dump_state()
        for e in (a, b):
            e.step_many(acts[12:15])
        a.set_block_shares(lay[3])
        for e in (a, b):
            e.load_state(blob)
            e.step_many(acts[15:24])
        _assert_same(a, b, "after the state load", state=True)
    finally:
        a.close()
        b.close()


def test_unfrozen_shares_settle_inside_the_clamps_and_change_nothing():
    a, b = _pair(_spec(SPEC3), N_SMALL, 8)
    try:
        _warm(a, b, 3, 0xB10D)
        acts = a.random_actions(130, 0x77)
        l0 = a.step_launches()
        a.step_many(acts)
        b.step_many(acts)
        assert a.step_launches() - l0 == 1 + 3  # the hand-over tick, then 64 + 64 + 1
        _assert_same(a, b, "130 ticks, the device's shares")
        c = a.block_shares()
        print("shares after 130 ticks:", c.tolist())
        assert c.sum() == 71 and c.min() >= 8 - 2 and c.max() <= 8 + 2
        # k_shares ran: a forced layout far outside the clamps, not frozen, is back inside them after one launch
        skew = np.array([27, 7, 7, 6, 6, 6, 6, 6])
        a.set_block_shares(skew, freeze=False)
        acts = a.random_actions(9, 0x78)
        a.step_many(acts)
        b.step_many(acts)
        _assert_same(a, b, "9 more ticks from a skewed layout")
        c = a.block_shares()
        print("shares after the skewed launch:", c.tolist())
        assert c.sum() == 71 and c.min() >= 6 and c.max() <= 10 and not np.array_equal(c, skew)
        # ... and frozen shares stay as set
        a.set_block_shares(skew, freeze=True)
        a.step_many(acts)
        b.step_many(acts)
        assert np.array_equal(a.block_shares(), skew)
        _assert_same(a, b, "9 ticks on frozen skewed shares")
    finally:
        a.close()
        b.close()


def test_5x5_against_the_restatement_with_uneven_shares():
    """4 096 envs on 5x5 maps, 256 blocks on 24 workgroups, 12 ticks in calls of 5 and 7 with the shares changed
    between them: every env's digest after the last tick of each call against the CPU restatement's."""
    from digest_parity import ACT_SEED
    from oracle import oracle
    from pgtg_amd.digest import Digest
    from pgtg_amd.vector import PGTGVecEnv
    from test_gpu_step_fused import _tune
    spec, n, T = _spec(dict(random_map_width=5, random_map_height=5)), 4096, 12
    ref = oracle.rollout_digest(spec, n, T, ACT_SEED)
    env = PGTGVecEnv(n, spec=spec, device=0, autoreset=True, tune=_tune(24))
    try:
        env.reset(seed=0)
        assert "k_envq" in env.step_kernel()
        acts = env.random_actions(T, ACT_SEED)
        dg, l0 = Digest(env), env.step_launches()
        for (lo, hi), c in (((0, 5), _layouts(24, 256, 33)[0]), ((5, 12), _layouts(24, 256, 33)[2])):
            env.set_block_shares(c, freeze=True)
            env.step_many(acts[lo:hi])
            got = dg.step_digest().cpu().numpy().view(np.uint64)
            bad = np.argwhere(got != ref[hi - 1])
            assert bad.size == 0, f"tick {hi - 1}: {len(bad)} env digests differ, first {bad[:8].ravel().tolist()}"
        assert env.step_launches() - l0 == 2
        assert env.error_count()[0] == 0
    finally:
        env.close()
