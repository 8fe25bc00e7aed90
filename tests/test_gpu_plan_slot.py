"""k_envq's three-slot map rings: the live tile plan stays in its ring slot (cur), no plan row.

Every case runs the persistent map-queue kernel (tune queue_mode=1) and is compared with the CPU
restatement on every env at every step (digest_parity / oracle.rollout_digest, as in
tests/test_gpu_exhaustive.py): several rounds of the persistent grid (the block counter, the qstate
bytes fetched one block ahead, a partial last block, the groups of <= 32 envs), one round with the
overflow lists, a time limit of one step (every slot cycles cur -> freed -> refilled -> head), maps of
more than 64 tiles (used-subgoal bits kept in the cur slot), the readers of an env's plan (squares,
map plan, save_map), and state blobs and snapshots of such handles."""
import functools
import json

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
from digest_parity import ACT_SEED, _compare_run, _spec
from oracle import oracle
from oracle.oracle import OracleEnv
from pgtg_amd import config as cfg

pytestmark = pytest.mark.gpu

CFG2 = dict(random_map_width=3, random_map_height=3)
CFG5 = dict(random_map_width=5, random_map_height=5)
K_ENVQ, K_ENVQ_BIG, K_ENVB = "pgtg::k_envq<false>", "pgtg::k_envq<true>", "pgtg::k_envb<false>"
F_EXITS = np.uint64(0xF << 33)  # the oracle keeps exit markers in its square words; the ABI does not
N5, T5 = 5 * 128 + 37, 40
TUNE5 = dict(envs_per_block=128, queue_mode=1)


def _make(n, conf, tune, L=0):
    from pgtg_amd.vector import PGTGVecEnv
    return PGTGVecEnv(n, spec=_spec(conf), device=0, autoreset=True, max_episode_steps=L or None, tune=tune)


@functools.lru_cache(maxsize=None)
def _ref5():
    """The restatement's rollout of the 5x5 case, computed once and shared: (digests [T, N], flags)."""
    ref, flags = oracle.rollout_digest(_spec(CFG5), N5, T5, ACT_SEED, flags_out=True)
    ref.setflags(write=False)
    flags.setflags(write=False)
    return ref, flags


def _digest(dg):
    return dg.step_digest().cpu().numpy().view(np.uint64)


def test_several_rounds_of_the_persistent_grid():
    tune = dict(envs_per_block=16, queue_mode=1)
    probe = _make(64, CFG2, tune)
    kern, shape, occ = probe.step_kernel(), probe.launch_info(), probe.occupancy()
    probe.close()
    assert kern == K_ENVQ and shape[0] == 16, (kern, shape)
    grid = min(occ * torch.cuda.get_device_properties(0).multi_processor_count, 4096)  # (kMaxQueueGrid)
    n = 2 * grid * 16 + 5
    run = _compare_run(_spec(CFG2), n, 30, tune, f"rounds {n} envs")
    assert run.kernel == K_ENVQ and run.launch[0] == 16, (run.kernel, run.launch)
    assert (run.flags & 1).sum() > n, "few episodes ended"


def test_one_round_with_overflow_lists():
    from pgtg_amd.digest import Digest
    ref, flags = _ref5()
    assert len(np.unique(ref)) >= 1000, "degenerate digests"
    env = _make(N5, CFG5, TUNE5)
    try:
        assert env.step_kernel() == K_ENVQ and env.launch_info()[0] == 128
        env.reset(seed=0)
        dg = Digest(env)
        for t in range(T5):
            env.step_random(ACT_SEED, t)
            bad = np.flatnonzero(_digest(dg) != ref[t])
            assert bad.size == 0, f"tick {t}: {bad.size} envs differ, first {bad[:8].tolist()}"
        assert env.error_count()[0] == 0
        assert (flags & 1).sum() > N5
        assert env.queue_overflow() > 0, "no workgroup listed more than 64 requests in a launch: the overflow lists did not run"
    finally:
        env.close()


def test_tightest_rotation_every_env_resets_in_every_launch():
    from pgtg_amd.digest import Digest
    n, T = 3 * 128 + 11, 12
    ref, flags = oracle.rollout_digest(_spec(CFG5), n, T, ACT_SEED, max_episode_steps=1, flags_out=True)
    assert (flags != 0).all()
    env = _make(n, CFG5, TUNE5, L=1)
    try:
        assert env.step_kernel() == K_ENVQ and env.launch_info()[0] == 128
        env.reset(seed=0)
        dg = Digest(env)
        truncated = 0
        for t in range(T):
            env.step_random(ACT_SEED, t)
            bad = np.flatnonzero(_digest(dg) != ref[t])
            assert bad.size == 0, f"tick {t}: {bad.size} envs differ, first {bad[:8].tolist()}"
            truncated += int(env.truncated.sum())
        assert truncated == n * T
        assert env.error_count()[0] == 0
        assert env.queue_overflow() > 0, "128 requests per workgroup and launch: the overflow lists ran"
    finally:
        env.close()


def _big_case():
    """The largest map of more than 64 tiles that the map queue accepts: (config, tune)."""
    for w, h in ((9, 9), (9, 8), (11, 6), (13, 5)):
        conf = dict(random_map_width=w, random_map_height=h)
        for epb in (None, 64, 32, 16):
            tune = dict(queue_mode=1) if epb is None else dict(queue_mode=1, envs_per_block=epb)
            probe = _make(200, conf, tune)
            kern = probe.step_kernel()
            probe.close()
            if kern == K_ENVQ_BIG:
                return conf, tune
    return None, None


def test_big_plan_keeps_used_subgoals_in_the_cur_slot():
    from pgtg_amd.digest import Digest
    conf, tune = _big_case()
    assert conf is not None, "no map of more than 64 tiles runs k_envq<true>"
    n, T = 200, 60
    ref, flags = oracle.rollout_digest(_spec(conf), n, T, ACT_SEED, flags_out=True)
    assert len(np.unique(ref)) >= 1000, "degenerate digests"
    env = _make(n, conf, tune)
    try:
        env.reset(seed=0)
        dg = Digest(env)
        marked = set()
        stepped_again = 0
        for t in range(T):
            env.step_random(ACT_SEED, t)
            bad = np.flatnonzero(_digest(dg) != ref[t])
            assert bad.size == 0, f"{conf} tick {t}: {bad.size} envs differ, first {bad[:8].tolist()}"
            if t in (20, 40):  # (the bits read back from the cur slot through pgtg_get_env_state)
                marked = {i for i in range(0, n, 4) if env.env_state(i)["used_subgoals"] != 0}
                assert marked, "no env of the sample has marked a subgoal used"
            elif t in (21, 41):  # the marked envs (mid-episode: a new episode has no bit set) stepped from those bits
                stepped_again += len(marked)
        assert stepped_again > 0, "no env marked a subgoal used and stepped again"
        assert env.error_count()[0] == 0
    finally:
        env.close()


def test_readers_follow_the_slot(tmp_path):
    """squares, map plan and save_map of envs whose plan was taken in the last launch and of envs whose
    plan has been in its slot for several launches, against per-env oracles"""
    T = 7
    env = _make(N5, CFG5, TUNE5)
    try:
        env.reset(seed=0)
        acts = env.random_actions(T, ACT_SEED)
        for t in range(T):
            env.step_actions(acts[t])
        torch.cuda.synchronize()
        done = (env.terminated | env.truncated).cpu().numpy().astype(bool)
        fresh, old = np.flatnonzero(done)[:3], np.flatnonzero(~done)[-3:]
        assert len(fresh) == 3 and len(old) == 3, (len(fresh), len(old))
        a = acts.cpu().numpy()
        spec = _spec(CFG5)
        for i in [int(x) for x in np.concatenate([fresh, old])]:
            o = OracleEnv(spec)
            o.reset(i)  # (the batch was reset with seed 0: env i with seed i)
            for t in range(T):
                if o.step(int(a[t, i]))["terminated"]:
                    o.reset(None)
            want = o.squares() & ~F_EXITS
            assert np.array_equal(env.squares(i).reshape(-1), want.reshape(-1)), f"env {i} squares"
            assert env.map_plan(i) == o.map_plan(), f"env {i} map plan"
            pa, pb = str(tmp_path / f"gpu{i}"), str(tmp_path / f"orc{i}")
            cfg.save_map_plan(env.map_plan(i), pa)
            cfg.save_map_plan(o.map_plan(), pb)
            with open(pa + ".json") as fa, open(pb + ".json") as fb:
                assert json.load(fa) == json.load(fb), f"env {i} saved map"
    finally:
        env.close()


def _sections(blob):
    """{section id: bytes} of a pgtg_dump_state blob (tests/test_gpu_snapshot.py _sections)"""
    hdr = 4 + 4 + 8 + 4 * 4 + 4 * 4 + 8
    n_sec = int(np.frombuffer(blob[16:20].tobytes(), np.uint32)[0])
    ent = np.frombuffer(blob[hdr:hdr + 16 * n_sec].tobytes(), dtype=[("id", "<u4"), ("pad", "<u4"), ("bytes", "<u8")])
    off, out = hdr + 16 * n_sec, {}
    for e in ent:
        off = (off + 15) & ~15
        out[int(e["id"])] = blob[off:off + int(e["bytes"])]
        off += int(e["bytes"])
    assert off == blob.size
    return out


def test_blob_resumes_bit_identically_and_the_other_kernel_refuses_it():
    from pgtg_amd.digest import Digest
    ref, _ = _ref5()
    a, b, other = _make(N5, CFG5, TUNE5), _make(N5, CFG5, TUNE5), _make(N5, CFG5, dict(envs_per_block=128, queue_mode=2))
    try:
        assert b.step_kernel() == K_ENVQ and other.step_kernel() == K_ENVB
        a.reset(seed=0)
        da, db = Digest(a), Digest(b)
        for t in range(9):
            a.step_random(ACT_SEED, t)
        blob = a.dump_state()
        secs = _sections(blob)
        assert 3 not in secs and 40 in secs and 41 in secs, sorted(secs)  # no plan rows: the rings hold the plans
        assert secs[40].size == N5 * 3 * 128, secs[40].size  # three 128-byte slots per env of a 5x5 map
        b.reset(seed=777)  # other episodes, replaced by the load
        b.load_state(blob)
        for t in range(9, 19):
            a.step_random(ACT_SEED, t)
            b.step_random(ACT_SEED, t)
            ga, gb = _digest(da), _digest(db)
            assert np.array_equal(ga, ref[t]) and np.array_equal(gb, ref[t]), f"tick {t}"
        sa, sb = _sections(a.dump_state()), _sections(b.dump_state())
        assert [k for k in sa if k != 5 and not np.array_equal(sa[k], sb[k])] == []
        other.reset(seed=0)
        kept = _sections(other.dump_state())
        with pytest.raises(ValueError):
            other.load_state(blob)
        now = _sections(other.dump_state())
        # (the batch-wide counters, id 5, aside, as in tests/test_gpu_snapshot.py)
        assert [k for k in kept if k != 5 and not np.array_equal(kept[k], now[k])] == [], "the refused blob changed the handle"
    finally:
        for e in (a, b, other):
            e.close()


def test_snapshot_restore_and_fork_between_two_envq_handles():
    from pgtg_amd.digest import Digest
    T0, K = 6, 5
    a, b = _make(N5, CFG5, TUNE5), _make(3 * 128 + 11, CFG5, TUNE5)
    snap = None
    try:
        a.reset(seed=0)
        b.reset(seed=4242)
        acts = a.random_actions(T0 + 2 * K + 12, ACT_SEED)
        for t in range(T0):
            a.step_actions(acts[t])
        torch.cuda.synchronize()
        done = (a.terminated | a.truncated).cpu().numpy().astype(bool)
        mid = [int(i) for i in np.flatnonzero(~done)[:16]]  # mid-episode envs
        assert len(mid) == 16
        snap = a.snapshot(16)
        snap.save(a, env_idx=mid, slot_idx=list(range(16)))
        dg = Digest(a)
        first = []
        for t in range(K):
            a.step_actions(acts[T0 + t])
            first.append(_digest(dg)[mid])
        snap.load(a, slot_idx=list(range(16)), env_idx=mid)
        for t in range(K):  # the same actions again: the restored envs repeat themselves
            a.step_actions(acts[T0 + t])
            assert np.array_equal(_digest(dg)[mid], first[t]), f"restore: tick {t}"
        # fork: the saved envs into envs 20..35 of another k_envq handle, same actions from the save on
        dst = list(range(20, 36))
        snap.load(b, slot_idx=list(range(16)), env_idx=dst)
        db = Digest(b)
        rows = torch.full((K + 12, b.num_envs), 4, dtype=torch.uint8, device=a.device)
        rows[:, dst] = acts[T0:T0 + K + 12][:, mid]
        snap.load(a, slot_idx=list(range(16)), env_idx=mid)
        ended = 0
        for t in range(K + 12):
            a.step_actions(acts[T0 + t])
            b.step_actions(rows[t])
            assert np.array_equal(_digest(dg)[mid], _digest(db)[dst]), f"fork: tick {t}"
            ended += int((b.terminated | b.truncated)[dst].sum())
        assert ended > 0, "no forked env finished an episode: the loaded rings were not used"
        assert a.error_count()[0] == 0 and b.error_count()[0] == 0
    finally:
        if snap is not None:
            snap.close()
        a.close()
        b.close()
