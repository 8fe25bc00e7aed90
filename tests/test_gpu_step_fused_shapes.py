"""k_envq<BIG, true> (pgtg_step_many) at every instance and workgroup shape, at the default cut of
64 ticks, over padded action rows and with observation outputs left unbound.

tests/test_gpu_step_fused.py runs the small-map instance with 16 envs per workgroup and at most 13 ticks per
launch.  Here the same comparison -- several ticks per launch against a launch per tick, everything equal bit
for bit -- runs on maps of 72 tiles (k_envq<true, true>: the used-subgoal marks stored into the cur ring slot
and staged again by the same lane, obs_key<true>, stage_plan<true>) and with 32, 64, 128 and 192 envs per
workgroup (one to three env waves, an image per lane, a writer wave without envs, request lists of several
batches of kQueueLanes), and two rows are also held to the CPU restatement's digests.  Every case asserts
launch_info()[0] and step_kernel(), so a handle that fell back to another block size or kernel fails.

Whether the kernel writes only the changed observation lines (its `delta`, `om != nullptr`) is not exposed by
the handle; _delta_lines restates the kernel's condition from launch_info() and the observation's shape, and
every case prints it.  The condition is 2 * lm_words <= 3 * envs with lm_words = ceil((envs * bits / 128 + 1) /
32) line-mask words, bits = channels * 9 * 9 for these one-tile windows: it holds at every row of SHAPES (on
both handles: the path depends on the layout, not on the ticks per launch), from each launch's second tick on
and on its first tick too when the handle's observation buffer is current.  The other case, `om == nullptr`
for a whole launch, is test_observation_outputs_left_unbound's (no `obs`: neither obs, and final_obs without
obs) and the sliding-window fixtures of tests/test_gpu_fuzz_reference.py's envq_many mode."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
from digest_parity import ACT_SEED, _spec
from oracle import oracle
from test_gpu_step_fused import N_SMALL, SPEC3, _assert_same, _pair, _Window

pytestmark = pytest.mark.gpu

BIG = dict(random_map_width=9, random_map_height=8)  # 72 tiles: k_envq<true, true>
SPEC4 = dict(random_map_width=4, random_map_height=4)
WARM = 6
CALLS = (2, 5, 12)

SHAPES = {
    # name: (map, envs per workgroup, envs, queue_grid, compared with the restatement too)
    "big_e16_grid8": (BIG, 16, 16 * 70 + 5, 8, True),      # 71 blocks: 9 or 8 per workgroup
    "big_e16_grid64": (BIG, 16, 16 * 70 + 5, 64, False),   # 2 blocks or 1 (the qstate byte read back)
    "s3_e32_grid4": (SPEC3, 32, 32 * 20 + 5, 4, False),    # the last value of group_obs's E <= 32 path
    "s3_e64_grid4": (SPEC3, 64, 64 * 12 + 5, 4, False),    # one full env wave, an image per lane
    "s3_e128_grid4": (SPEC3, 128, 128 * 8 + 5, 4, True),   # the benchmark's shape: two env waves, 3 or 2 blocks
    "s3_e128_grid8": (SPEC3, 128, 128 * 8 + 5, 8, False),  # two blocks on workgroup 0, one on the other seven
    # (a 3x3 map at 192 envs per workgroup gets k_env: create keeps three env waves for maps of 16 tiles or more)
    "s4_e192_grid4": (SPEC4, 192, 192 * 5 + 5, 4, False),  # three env waves: the helper is the last wave
}


def _delta_lines(env, obs_bound=True):
    """The kernel's `delta` condition (pgtg_env.hip k_envq, lds_tail) for a launch that finds the observation
    buffer current, restated from launch_info() and the observation's shape: a map-queue handle without
    traffic whose image holds the whole workgroup."""
    E = env.launch_info()[0]
    bits = len(env.keys) * env.window * env.window
    lines = (127 + E * bits) // 128 + 1
    lm_words = (lines + 31) // 32 if lines <= 64 * 32 else 0
    return bool(lm_words) and obs_bound and not env.spec.sliding and 2 * lm_words <= 3 * E


def _check_shape(e, epb, n, grid, big):
    assert e.launch_info()[0] == epb, e.launch_info()
    assert "k_envq" in e.step_kernel() and ("<true>" in e.step_kernel()) == big, e.step_kernel()
    assert (n + epb - 1) // epb > grid  # (more blocks than workgroups: step_many may run several ticks per launch)


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_instance_and_block_shape(name):
    """Six single steps, a state dump (the comparison after the warm-up: it serves the pending requests on both
    handles, so that every call that follows is one launch), then calls of 2, 5 and 12 ticks."""
    from pgtg_amd.digest import Digest
    conf, epb, n, grid, restated = SHAPES[name]
    spec, T = _spec(conf), WARM + sum(CALLS)
    a, b = _pair(spec, n, grid, seed=0, envs_per_block=epb)
    try:
        for e in (a, b):
            _check_shape(e, epb, n, grid, conf is BIG)
        print(f"{name}: {a.step_kernel()} {a.launch_info()} delta lines: {_delta_lines(a)} / {_delta_lines(b)}")
        assert _delta_lines(a) and _delta_lines(b)  # (see the module's docstring for the other case)
        ref = flags = None
        if restated:
            ref, flags = oracle.rollout_digest(spec, n, T, ACT_SEED, flags_out=True)
            assert len(np.unique(ref)) >= 1000, "degenerate digests"
        acts = a.random_actions(T, ACT_SEED)
        for t in range(WARM):
            a.step_actions(acts[t])
            b.step_actions(acts[t])
        _assert_same(a, b, f"{name} warm-up")
        dg, t0 = Digest(a), WARM
        for K in CALLS:
            wa, wb = _Window(a), _Window(b)
            a.step_many(acts[t0:t0 + K])
            b.step_many(acts[t0:t0 + K])
            t0 += K
            wa.check_busy(f"{name} K {K}", 1)
            wb.check_busy(f"{name} K {K}", K)
            if restated:
                assert (flags[t0 - K:t0] != 0).any(1).all(), "a tick without an episode end in the restatement"
                got = dg.step_digest().cpu().numpy().view(np.uint64)
                bad = np.argwhere(got != ref[t0 - 1])
                assert bad.size == 0, f"{name} tick {t0 - 1}: {len(bad)} env digests differ, first {bad[:8].ravel().tolist()}"
                assert a.counters()[1] - wa.c0[1] == int((flags[t0 - K:t0] != 0).sum())
            _assert_same(a, b, f"{name} K {K}")
            for e in (a, b):
                _check_shape(e, epb, n, grid, conf is BIG)
    finally:
        a.close()
        b.close()


def test_default_cut_of_64_ticks():
    """step_ticks unset: 130 ticks in launches of 64 + 64 + 2, then (a state dump between) 65 in 64 + 1,
    against a launch per tick and, after ticks 130 and 195, every env's digest against the restatement."""
    from pgtg_amd.digest import Digest
    spec, n = _spec(SPEC3), N_SMALL
    ref, flags = oracle.rollout_digest(spec, n, 195, ACT_SEED, flags_out=True)
    ends = (flags[:130] != 0).sum(0)
    print("episode ends in 130 ticks:", int(ends.sum()), "at most per env:", int(ends.max()))
    assert int(ends.sum()) == 63292 and int(ends.max()) == 78 and (flags != 0).any(1).all()
    a, b = _pair(spec, n, 8, seed=0, autoreset=True)
    try:
        acts = a.random_actions(195, ACT_SEED)
        _assert_same(a, b, "cut: reset")
        dg, t0 = Digest(a), 0
        for K, launches in ((130, 3), (65, 2)):
            wa, wb = _Window(a), _Window(b)
            a.step_many(acts[t0:t0 + K])
            b.step_many(acts[t0:t0 + K])
            t0 += K
            wa.check_busy(f"cut K {K}", launches)
            wb.check_busy(f"cut K {K}", K)
            got = dg.step_digest().cpu().numpy().view(np.uint64)
            bad = np.argwhere(got != ref[t0 - 1])
            assert bad.size == 0, f"tick {t0 - 1}: {len(bad)} env digests differ, first {bad[:8].ravel().tolist()}"
            assert a.counters()[1] - wa.c0[1] == int((flags[t0 - K:t0] != 0).sum())
            _assert_same(a, b, f"cut K {K}")
    finally:
        a.close()
        b.close()


def test_padded_action_rows():
    """Action rows of stride n + 37 (the pad columns hold 9, no valid action), 7 ticks cut 3 + 3 + 1: the
    second and third launch start at actions + k * row_stride, and every tick inside a launch advances by
    the stride.  The other handle is fed the contiguous copy, a launch per tick."""
    n, K = N_SMALL, 7
    a, b = _pair(_spec(SPEC3), n, 8, step_ticks=3)
    try:
        for rep in range(2):  # (the second call finds the first one's lists pending)
            acts = a.random_actions(K, 0x9AD, t0=K * rep)
            wide = torch.full((K, n + 37), 9, dtype=torch.uint8, device="cuda")
            wide[:, :n] = acts
            view = wide[:, :n]
            assert view.stride() == (n + 37, 1) and torch.equal(view, acts) and int(acts.max()) <= 8
            wa, wb = _Window(a), _Window(b)
            a.step_many(view)
            b.step_many(acts.contiguous())
            wa.check_busy(f"padded rep {rep}", 3)
            wb.check_busy(f"padded rep {rep}", K)
            _assert_same(a, b, f"padded rep {rep}", state=rep == 1)
        assert torch.equal(wide[:, n:], torch.full((K, 37), 9, dtype=torch.uint8, device="cuda"))
    finally:
        a.close()
        b.close()


UNBOUND = {"neither": ("obs", "final_obs"), "obs_without_final_obs": ("final_obs",), "final_obs_without_obs": ("obs",)}


@pytest.mark.parametrize("name", list(UNBOUND))
def test_observation_outputs_left_unbound(name):
    """pgtg_set_outputs with null observation pointers after the reset, on both handles: 5 ticks in one
    launch, a single step, then 7 ticks (a launch of one tick for the single step's lists, then one of 6).
    The small outputs, counters and every state section equal the launch-per-tick handle's; the tensors
    that are no longer bound keep the marker written into them."""
    a, b = _pair(_spec(SPEC3), N_SMALL, 8)
    try:
        marked = []
        for e in (a, b):
            for field in UNBOUND[name]:
                setattr(e._outs, field, None)
                t = e.obs_map if field == "obs" else e.final_map
                t.fill_(7)
                marked.append(t)
            assert e._lib.pgtg_set_outputs(e._h, C.byref(e._outs)) == 0
        bound = "obs" not in UNBOUND[name]
        print(f"{name}: delta lines: {_delta_lines(a, bound)} / {_delta_lines(b, bound)}")
        assert _delta_lines(a, bound) == bound
        acts = a.random_actions(13, 0x0B5)
        wa, wb = _Window(a), _Window(b)
        for e in (a, b):
            e.step_many(acts[0:5])
        _assert_same(a, b, f"{name} after 5", state=False)
        for e in (a, b):
            e.step_actions(acts[5])
            e.step_many(acts[6:13])
        wa.check_busy(name, 4)
        wb.check_busy(name, 13)
        _assert_same(a, b, f"{name} after 5 + 1 + 7")
        assert all(bool((t == 7).all()) for t in marked), "an output that is not bound was written"
        if bound:  # (the observation still goes out, by changed lines)
            assert int(a.obs_map.max()) == 1
    finally:
        a.close()
        b.close()
