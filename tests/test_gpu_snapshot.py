"""Device-resident snapshots (include/pgtg.h pgtg_snapshot_*, pgtg_amd/vector.py Snapshot): single envs
saved, restored and forked on the GPU by the kernel k_state_copy.

  * a fork against the CPU restatement: after t0 ticks every env is saved, env j is loaded from the slot
    of a random env src[j] (with repeats) and fed src[j]'s actions: seeds, actions and digests depend on
    the source index only, so env j's digests must be oracle.rollout_digest(...)[t][src[j]] from then on,
    on every step-kernel path and into a second handle of another batch size;
  * nothing left out: save all + load all into a fresh handle leaves byte-identical state blobs;
  * partial loads, count 0 and 1, out-of-range pairs, copy_envs with overlapping sides;
  * refusals, light_step(actions), the episode statistics across a load."""
import functools
import os

import numpy as np
import pytest
import torch

import digest_parity
import helpers
from digest_parity import ACT_SEED, _spec
from oracle import oracle
from pgtg_amd import config as cfg

pytestmark = pytest.mark.gpu

N, N2, T = 1000, 1537, 20  # (neither a multiple of 64 nor of 256)
CFG2 = dict(random_map_width=3, random_map_height=3)
# the reference's training caller (pgtg/train.py:21-37), as in tests/test_gpu_truncation.py
CALLER = dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=0.2,
              random_map_percentage_of_connections=0.8, traffic_density=0.2, conservative_driver_percentage=0.15,
              normal_driver_percentage=0.50, aggressive_driver_percentage=0.20, elderly_driver_percentage=0.10,
              reckless_driver_percentage=0.05, sliding_observation_window_size=5, max_allowed_deviation=15,
              use_sliding_observation_window=True, use_next_subgoal_direction=True, final_goal_bonus=200,
              standing_still_penalty=1)
DENSE = dict(random_map_width=4, random_map_height=4, traffic_density=0.3)
BIG = dict(random_map_width=9, random_map_height=9)
FIXED_MAP = os.path.join(helpers.TESTDATA, "map_with_all_directions.json")

K_ENV, K_ENVQ, K_ENVB = "pgtg::k_env<false, false>", "pgtg::k_envq<false>", "pgtg::k_envb<false>"
K_TRAFFIC = "pgtg::k_env<true, false> + pgtg::k_traffic"

# name: (config, tune, max_episode_steps, t0, step kernel, distinct digests asked of the compared ticks)
# The guard against degenerate digests is digest_parity._compare_run's: random maps at 1000 envs give
# about 2 000 distinct outputs without traffic and one per (tick, env) with it; a fixed map has one
# episode map and a few hundred outputs at any batch size, so that case asks for 250.
FORK = {
    "envq": (CFG2, dict(queue_mode=1), 0, 6, K_ENVQ, 1000),
    "envb": (CFG2, dict(queue_mode=2), 0, 6, K_ENVB, 1000),
    "caller_L3": (CALLER, None, 3, 6, K_TRAFFIC, 1000),
    "dense_fresh": (DENSE, None, 0, 0, K_TRAFFIC, 1000),
    "big_map": (BIG, None, 0, 6, "true>", 1000),
    "fixed_map": (FIXED_MAP, None, 0, 6, K_ENV, 250),
}


def _case_spec(conf):
    return cfg.make_spec(conf) if isinstance(conf, str) else _spec(conf)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The restatement's rollout of a FORK case, computed once: (digests [T, N], flags [T, N])."""
    conf, _, L, _, _, _ = FORK[name]
    ref, flags = oracle.rollout_digest(_case_spec(conf), N, T, ACT_SEED, max_episode_steps=L, flags_out=True)
    ref.setflags(write=False)
    return ref, flags


def _digest(dg, n=None):
    d = dg.step_digest().cpu().numpy().view(np.uint64)
    return d if n is None else d[:n]


def _make(n, conf, tune=None, L=0, **kw):
    from pgtg_amd.vector import PGTGVecEnv
    return PGTGVecEnv(n, spec=_case_spec(conf), device=0, autoreset=True, max_episode_steps=L or None, tune=tune, **kw)


@pytest.mark.parametrize("name, second", [(k, False) for k in sorted(FORK)] + [("caller_L3", True), ("envq", True)])
def test_fork_matches_the_oracle(name, second):
    from pgtg_amd.digest import Digest
    conf, tune, L, t0, kernel, distinct = FORK[name]
    ref, flags = _reference(name)
    # the comparison has teeth (digest_parity._compare_run's guard, on the ticks compared here), and
    # episodes end after the fork: the loaded rings, step counts and RNG streams are used
    assert len(np.unique(ref[t0:])) >= min(ref[t0:].size // 4, distinct), "degenerate digests"
    assert (flags[t0:] & 1).sum() > N, "few episodes end after the fork"
    if L:
        assert (flags[t0:] == 2).sum() > 0, "no env is truncated after the fork"
    rng = np.random.default_rng(2024)
    src = rng.integers(0, N, N)
    assert (src != np.arange(N)).mean() > 0.99 and len(np.unique(src)) < N  # moved, with repeats
    a = _make(N, conf, tune, L)
    b = _make(N2, conf, tune, L) if second else a
    snap = None
    try:
        assert a.step_kernel().endswith(kernel) if kernel == "true>" else a.step_kernel() == kernel, a.step_kernel()
        assert b.step_kernel() == a.step_kernel()
        a.reset(seed=0)
        dg = Digest(a)
        for t in range(t0):
            a.step_random(ACT_SEED, t)
            assert np.array_equal(_digest(dg), ref[t]), f"{name}: tick {t} before the fork"
        acts = a.random_actions(T, ACT_SEED)  # row t = the actions of tick t, as step_random draws them
        tsrc = torch.as_tensor(src, device=a.device)
        rows = torch.full((T, b.num_envs), 4, dtype=torch.uint8, device=a.device)
        rows[:, :N] = acts.index_select(1, tsrc)
        snap = a.snapshot()
        assert snap.slots == N and snap.nbytes == N * snap.bytes_per_env
        snap.save(a)
        if second:
            b.reset(seed=31337)  # other episodes: the first N are replaced, the rest go on
        snap.load(b, slot_idx=tsrc)  # slot src[j] -> env j, j < N
        dg = Digest(b)
        for t in range(t0, T):
            b.step_actions(rows[t])
            got, want = _digest(dg, N), ref[t][src]
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"{name} tick {t}: {bad.size} envs differ, first {bad[:8].tolist()} from {src[bad[:8]].tolist()}"
        assert b.error_count()[0] == 0
    finally:
        if snap is not None:
            snap.close()
        a.close()
        if second:
            b.close()


# ---- nothing left out ---------------------------------------------------------------------------------

def _sections(blob):
    """{section id: bytes} of a pgtg_dump_state blob: PgtgStateHeader (56 bytes, n_sections at 16), then
    n_sections x {id u32, pad u32, bytes u64}, then each section at a 16-byte aligned offset."""
    hdr = 4 + 4 + 8 + 4 * 4 + 4 * 4 + 8
    assert bytes(blob[:4]) == b"PGTS"
    n_sec = int(np.frombuffer(blob[16:20].tobytes(), np.uint32)[0])
    ent = np.frombuffer(blob[hdr:hdr + 16 * n_sec].tobytes(), dtype=[("id", "<u4"), ("pad", "<u4"), ("bytes", "<u8")])
    off, out = hdr + 16 * n_sec, {}
    for e in ent:
        off = (off + 15) & ~15
        out[int(e["id"])] = blob[off:off + int(e["bytes"])]
        off += int(e["bytes"])
    assert off == blob.size and len(out) == n_sec, (off, blob.size)
    return out


def _state_diff(x, y):
    """Ids of the sections in which two blobs differ, the batch-wide counters (id 5) aside."""
    sx, sy = _sections(x), _sections(y)
    assert sorted(sx) == sorted(sy) and 1 in sx and 5 in sx
    return [k for k in sorted(sx) if k != 5 and not np.array_equal(sx[k], sy[k])]


WHOLE = {
    "queue_envq": (CFG2, dict(queue_mode=1)),
    "queue_envb": (CFG2, dict(queue_mode=2)),
    "traffic": (DENSE, None),
    "obstacles_visited": (dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=1.0,
                               random_map_ice_probability_weight=1, random_map_broken_road_probability_weight=1,
                               random_map_sand_probability_weight=1, random_map_traffic_light_probability_weight=1,
                               already_visited_position_penalty=0.5, separate_reward_cost=True), None),
}


@pytest.mark.parametrize("name", sorted(WHOLE))
def test_save_all_load_all_leaves_identical_blobs(name):
    """Every section of the state blob but the counters, byte for byte, in a second handle that holds
    other episodes: a section added to the blob later and forgotten in the copy fails here."""
    conf, tune = WHOLE[name]
    a, b = _make(N, conf, tune), _make(N, conf, tune)
    snap = a.snapshot()
    try:
        a.reset(seed=3)
        b.reset(seed=99)
        for t in range(8):
            a.step_random(0x5A7E, t)
        snap.save(a)
        snap.load(b)
        x, y = a.dump_state(), b.dump_state()
        assert x.size == y.size
        ids = sorted(_sections(x))
        if name.startswith("queue"):
            assert 40 in ids and 41 in ids
        if name == "traffic":
            assert {31, 32, 33, 34, 35, 36, 37} <= set(ids)
        if name == "obstacles_visited":
            assert 30 in ids
        assert _state_diff(x, y) == [], name
        assert not np.array_equal(_sections(x)[1], np.zeros_like(_sections(x)[1]))
    finally:
        snap.close()
        a.close()
        b.close()


# ---- partial loads and edge shapes --------------------------------------------------------------------

PARTIAL_CFG = {"envq": (CFG2, dict(queue_mode=1)), "traffic": (DENSE, None)}
M = 600
BIG_IDX = 4_000_000_000  # (as uint32 far outside every side)
# name: (slot_idx, env_idx, check): slot s was saved from env s at tick T_SAVE
PAIRS = {
    "none": ([], [], True),
    "one": ([123], [77], True),
    "middle_37": (list(range(400, 437)), list(range(400, 437)), True),
    "unchecked_out_of_range": ([3, 10**6, 5, 7, 8, 9], [10, 11, BIG_IDX, 2, -1, M], False),
}
T_SAVE, T_LOAD, T_MORE = 3, 5, 6


@pytest.mark.parametrize("pairs", sorted(PAIRS))
@pytest.mark.parametrize("conf", sorted(PARTIAL_CFG))
def test_partial_load_touches_the_loaded_envs_only(conf, pairs):
    """A twin handle records the digests of the plain rollout.  The handle under test saves every env at
    tick 3 and at tick 5 loads some: env e loaded from slot s then gets the actions env s had from tick
    3 on, and must repeat the twin's env s from tick 3; every other env goes on as the twin's."""
    from pgtg_amd.digest import Digest
    c, tune = PARTIAL_CFG[conf]
    slots, envs, check = PAIRS[pairs]
    valid = [(s, e) for s, e in zip(slots, envs) if 0 <= s < M and 0 <= e < M]
    assert len(valid) == {"none": 0, "one": 1, "middle_37": 37, "unchecked_out_of_range": 2}[pairs]
    a, w = _make(M, c, tune), _make(M, c, tune)
    snap = a.snapshot()
    try:
        total = T_LOAD + T_MORE
        acts = a.random_actions(total, 0xFACE)
        w.reset(seed=9)
        dw = Digest(w)
        rec = []
        for t in range(total):
            w.step_actions(acts[t])
            rec.append(_digest(dw))
        a.reset(seed=9)
        da = Digest(a)
        for t in range(T_LOAD):
            if t == T_SAVE:
                snap.save(a)
            a.step_actions(acts[t])
            assert np.array_equal(_digest(da), rec[t])
        errors = a.error_count()
        snap.load(a, slot_idx=slots, env_idx=envs, check=check)
        assert a.error_count() == errors
        es = np.array([e for _, e in valid], dtype=np.int64)
        ss = np.array([s for s, _ in valid], dtype=np.int64)
        rest = np.setdiff1d(np.arange(M), es)
        for k in range(T_MORE):
            row = acts[T_LOAD + k].clone()
            if len(valid):
                row[torch.as_tensor(es, device=a.device)] = acts[T_SAVE + k][torch.as_tensor(ss, device=a.device)]
            a.step_actions(row)
            got = _digest(da)
            assert np.array_equal(got[rest], rec[T_LOAD + k][rest]), f"step {k} after the load: an env outside the load changed"
            assert np.array_equal(got[es], rec[T_SAVE + k][ss]), f"step {k} after the load: a loaded env"
        assert a.error_count() == errors
    finally:
        snap.close()
        a.close()
        w.close()


def test_load_checks_ranges_and_duplicate_destinations():
    a = _make(64, CFG2)
    snap = a.snapshot(16)
    try:
        a.reset(seed=1)
        assert snap.slots == 16 and snap.nbytes == 16 * snap.bytes_per_env
        snap.save(a, env_idx=list(range(16)))
        before = a.dump_state()
        for slot_idx, env_idx in (([0, 16], [1, 2]), ([0, 1], [64, 2]), ([0, -1], [1, 2]), ([0, 1], [1, -2]),
                                  ([0, 1], [5, 5]), ([0, 1, 2], [1, 2]), (None, list(range(17)))):
            with pytest.raises(ValueError):
                snap.load(a, slot_idx=slot_idx, env_idx=env_idx)
        with pytest.raises(ValueError):
            snap.load(a, slot_idx=[0.5], env_idx=[1])
        assert _state_diff(before, a.dump_state()) == []
        snap.load(a, slot_idx=[3, 3], env_idx=[5, 6])  # (a slot may repeat)
        after = a.dump_state()
        rec = lambda blob, i: _sections(blob)[1].reshape(64, -1)[i]  # noqa: E731
        assert np.array_equal(rec(after, 5), rec(before, 3)) and np.array_equal(rec(after, 6), rec(before, 3))
    finally:
        snap.close()
        a.close()


@pytest.mark.parametrize("conf", sorted(PARTIAL_CFG))
def test_copy_envs_with_overlapping_sides_is_a_gather(conf):
    """A cyclic shift by one inside the batch: env k + 1 becomes what env k was, for every k at once."""
    from pgtg_amd.digest import Digest
    c, tune = PARTIAL_CFG[conf]
    a, w = _make(M, c, tune), _make(M, c, tune)
    try:
        acts = a.random_actions(10, 0xC0C0)
        for e in (a, w):
            e.reset(seed=4)
            for t in range(4):
                e.step_actions(acts[t])
        src = torch.arange(M, device=a.device)
        dst = (src + 1) % M
        a.copy_envs(src, dst)
        da, dw = Digest(a), Digest(w)
        assert torch.equal(a.obs_map.roll(-1, 0), w.obs_map)  # (the observation re-emitted after the load)
        for t in range(4, 10):
            w.step_actions(acts[t])
            a.step_actions(acts[t].roll(1))
            assert np.array_equal(np.roll(_digest(da), -1), _digest(dw)), f"tick {t}"
        with pytest.raises(ValueError):
            a.copy_envs([0, M], [1, 2])
    finally:
        a.close()
        w.close()


# ---- refusals ---------------------------------------------------------------------------------------------

def test_other_handles_are_refused_and_nothing_changes():
    """Another configuration hash, another car capacity (handles with car slots: no map queue), and the
    other map-queue step kernel, whose rings hold another number of maps (handles without car slots)."""
    base = _make(64, CFG2, min_car_capacity=4)
    others = {
        "config hash": _make(64, dict(CFG2, crash_penalty=7), min_car_capacity=4),
        "car capacity": _make(64, CFG2, min_car_capacity=9),
    }
    plain = {"envq": _make(64, CFG2, dict(queue_mode=1)), "envb": _make(96, CFG2, dict(queue_mode=2))}
    same = _make(96, CFG2, min_car_capacity=4)
    snap = base.snapshot()
    psnap = plain["envq"].snapshot()
    try:
        assert plain["envq"].step_kernel() == K_ENVQ and plain["envb"].step_kernel() == K_ENVB
        base.reset(seed=1)
        base.step_random(1, 0)
        snap.save(base)
        kept = base.dump_state()
        for e in list(others.values()) + list(plain.values()):
            e.reset(seed=2)
        plain["envq"].step_random(1, 0)
        psnap.save(plain["envq"])
        cases = [(snap, o, why) for why, o in others.items()] + [(psnap, plain["envb"], "ring depth")]
        for s, o, why in cases:
            blob = o.dump_state()
            with pytest.raises(ValueError, match="snapshot"):
                s.load(o, slot_idx=[0], env_idx=[0])
            with pytest.raises(ValueError, match="snapshot"):
                s.save(o)
            with pytest.raises(ValueError, match="snapshot"):
                s.save(o, env_idx=[], slot_idx=[])  # (refused whatever the count)
            assert _state_diff(blob, o.dump_state()) == [], why
        # the refused saves wrote nothing into the snapshot: it still restores the handle it came from,
        # and a handle of the same configuration and another batch size accepts it
        for t in range(3):
            base.step_random(1, 1 + t)
        assert _state_diff(kept, base.dump_state()) != []
        snap.load(base)
        assert _state_diff(kept, base.dump_state()) == []
        same.reset(seed=5)
        snap.load(same, env_idx=list(range(20, 84)))
        rec = lambda e: _sections(e.dump_state())[1].reshape(e.num_envs, -1)  # noqa: E731
        assert np.array_equal(rec(same)[20:84], rec(base))
    finally:
        snap.close()
        psnap.close()
        for e in list(others.values()) + list(plain.values()) + [base, same]:
            e.close()


# ---- light_step(actions) ------------------------------------------------------------------------------

@pytest.mark.parametrize("conf", ["caller", "envq"])
def test_light_step_returns_the_step_and_leaves_no_trace(conf):
    from pgtg_amd.digest import Digest
    c, tune = {"caller": (CALLER, None), "envq": (CFG2, dict(queue_mode=1))}[conf]
    n = 300
    a, stepped, never = _make(n, c, tune, 4), _make(n, c, tune, 4), _make(n, c, tune, 4)
    try:
        acts = a.random_actions(9, 0x11687)
        for e in (a, stepped, never):
            e.reset(seed=12)
            for t in range(3):
                e.step_actions(acts[t])
        obs, rew, term, trunc = a.light_step(acts[3])
        sobs, srew, sterm, strunc, _ = stepped.step(acts[3])
        assert torch.equal(rew, srew) and torch.equal(term, sterm) and torch.equal(trunc, strunc)
        assert torch.equal(obs["position"], sobs["position"]) and torch.equal(obs["velocity"], sobs["velocity"])
        assert sorted(obs["map"]) == sorted(sobs["map"])
        assert all(torch.equal(obs["map"][k], sobs["map"][k]) for k in sobs["map"])
        if "next_subgoal_direction" in sobs:
            assert torch.equal(obs["next_subgoal_direction"], sobs["next_subgoal_direction"])
        assert rew.data_ptr() != a.reward.data_ptr()  # clones, not views of the bound tensors
        assert bool((term | trunc).any()), "no episode ended in the light step"

        def same_outputs(tag):
            for x, y in zip(a._bound_tensors(), never._bound_tensors()):
                assert torch.equal(x, y), tag

        same_outputs("after light_step")
        da, dn = Digest(a), Digest(never)
        for t in range(3, 8):
            a.step_actions(acts[t])
            never.step_actions(acts[t])
            assert np.array_equal(_digest(da), _digest(dn)), f"tick {t}"
            same_outputs(f"tick {t}")
    finally:
        for e in (a, stepped, never):
            e.close()


# ---- episode statistics -------------------------------------------------------------------------------

def test_load_restarts_the_loaded_envs_episode_statistics():
    """Standing still on 3x3 maps under a limit of 4 steps: every episode is truncated at its 4th step.
    Saved at tick 5 (one step into the second episodes), loaded at tick 7 for envs 50..87: their running
    length restarts at 0 while their step count, which is state, is 1 again -- so they are truncated
    three steps later with a length of 3; the other envs and the summary are untouched by the load."""
    n, L = 200, 4
    a = _make(n, dict(CFG2, use_next_subgoal_direction=True), None, L)
    snap = a.snapshot()
    try:
        a.reset(seed=7)
        ep_ret, ep_len = a.enable_episode_stats()
        stand = torch.full((n,), 4, dtype=torch.uint8, device=a.device)
        for t in range(7):
            a.step_actions(stand)
            assert not bool(a.terminated.any())
            if t == 4:
                snap.save(a)
        assert ep_len.tolist() == [3] * n
        summary = a.episode_summary(reset=False)
        assert summary["episodes"] == n and summary["truncated_only"] == n and summary["length_sum"] == 4 * n
        idx = torch.arange(50, 88, device=a.device)
        snap.load(a, slot_idx=idx, env_idx=idx)
        assert a.episode_summary(reset=False) == summary
        loaded = np.zeros(n, bool)
        loaded[50:88] = True
        want = [(np.where(loaded, 1, 4), ~loaded), (np.where(loaded, 2, 1), np.zeros(n, bool)), (np.where(loaded, 3, 2), loaded)]
        for k, (length, trunc) in enumerate(want):
            a.step_actions(stand)
            assert np.array_equal(ep_len.cpu().numpy(), length), k
            assert np.array_equal(a.truncated.cpu().numpy(), trunc) and not bool(a.terminated.any()), k
        after = a.episode_summary(reset=False)
        assert after["episodes"] == 2 * n and after["length_sum"] == 4 * n + 4 * (n - 38) + 3 * 38
    finally:
        snap.close()
        a.close()
