"""The in-kernel TimeLimit (max_episode_steps) on every step-kernel path, against the CPU restatement.

The oracle's rollout applies gymnasium's TimeLimit over same-step auto-reset itself
(oracle.rollout_digest(max_episode_steps=L); tests/test_digest.py pins it to an env-by-env count around
OracleEnv), so every env of a batch is compared at every step, as in tests/test_gpu_exhaustive.py.
A time limit ends every episode of a batch in the same launch, which random actions never do: every
ring of a map-queue workgroup drains together (k_envb: the uncapped level-0 fill, then the capped
refills running short everywhere at once; k_envq: 128 requests per workgroup for a 64-entry list, no
helper with a spare lane, the overflow lists full), k_env compacts 256 resets with no helper lanes
left, and k_traffic has the whole batch on its work list launch after launch.  The cases are the
smallest batches that reach each of these regimes: a few workgroups and a ragged tail, forced into
the launch shape with the tune knobs, which each case then checks through step_kernel() and
launch_info().  The regime counts come from the oracle's flags, never from the kernel's.

Beside the digests: the outputs that the digest does not hold (terminal position, velocity,
next-subgoal direction, the car list at the truncation) compared directly for a sample of envs, and
the life cycle of the step count (masked reset, dump_state / load_state, autoreset=False)."""
import os

import numpy as np
import pytest
import torch

import helpers
from digest_parity import ACT_SEED, _compare_run, _spec
from oracle import oracle
from oracle.oracle import OracleEnv
from pgtg_amd import config as cfg

pytestmark = pytest.mark.gpu

CFG5 = dict(random_map_width=5, random_map_height=5)
CFG2 = dict(random_map_width=3, random_map_height=3)
TRAFFIC = dict(random_map_width=5, random_map_height=5, traffic_density=0.5)
LANES = dict(random_map_width=3, random_map_height=3, random_map_obstacle_probability=0.5,
             features_to_include_in_observation=["walls", "goals", "car_spawner", "car_lane all right",
                                                 "traffic_light", "ice", "start", "final goal"])
# the reference's training caller (pgtg/train.py:21-37), tests/test_gpu_exhaustive.py train_caller_8192x30
CALLER = dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=0.2,
              random_map_percentage_of_connections=0.8, traffic_density=0.2, conservative_driver_percentage=0.15,
              normal_driver_percentage=0.50, aggressive_driver_percentage=0.20, elderly_driver_percentage=0.10,
              reckless_driver_percentage=0.05, sliding_observation_window_size=5, max_allowed_deviation=15,
              use_sliding_observation_window=True, use_next_subgoal_direction=True, final_goal_bonus=200,
              standing_still_penalty=1)
OBST_VISITED = dict(random_map_width=3, random_map_height=3, random_map_obstacle_probability=1.0,
                    already_visited_position_penalty=0.25)
FIXED_MAP = os.path.join(helpers.TESTDATA, "4x1_map.json")

K_ENV, K_ENVQ, K_ENVB = "pgtg::k_env<false, false>", "pgtg::k_envq<false>", "pgtg::k_envb<false>"
K_TRAFFIC = "pgtg::k_env<true, false> + pgtg::k_traffic"

# The guard against degenerate digests (digest_parity._compare_run, min_distinct) counts the distinct
# digests of the restatement's rollout.  Under a limit of one to three steps the agent never leaves the
# tile it starts on, and the observation is the 9x9 window of that one tile: without traffic a rollout
# has a few hundred distinct outputs at any batch size (98 325 5x5 envs x 6 steps at L = 2: 688), so
# the short no-traffic cases ask for 250; a fixed map with one start has 9^L action sequences at most.
FEW = 250

CASES = {
    # name: (config, envs, steps, limit, tune, step kernel, envs per workgroup where forced, min_distinct)
    "envb_L1": (CFG5, 5 * 128 + 37, 8, 1, dict(envs_per_block=128, queue_mode=2), K_ENVB, 128, FEW),
    "envb_L2": (CFG5, 5 * 128 + 37, 10, 2, dict(envs_per_block=128, queue_mode=2), K_ENVB, 128, FEW),
    "envb_wg192_L3": (CFG5, 3 * 192 + 50, 12, 3, dict(envs_per_block=192, queue_mode=2), K_ENVB, 192, FEW),
    "envb_wg16_L1": (CFG2, 9 * 16 + 5, 8, 1, dict(envs_per_block=16, queue_mode=2), K_ENVB, 16, FEW),
    "envq_one_round_L1": (CFG5, 5 * 128 + 37, 8, 1, dict(envs_per_block=128, queue_mode=1), K_ENVQ, 128, FEW),
    "envq_one_round_L2": (CFG5, 5 * 128 + 37, 10, 2, dict(envs_per_block=128, queue_mode=1), K_ENVQ, 128, FEW),
    "env_wg256_L1": (CFG2, 2 * 256 + 19, 8, 1, dict(envs_per_block=256), K_ENV, 256, FEW),
    "env_wg256_sub32_L2": (CFG2, 2 * 256 + 19, 10, 2, dict(envs_per_block=256, obs_sub=32), K_ENV, 256, FEW),
    "env_lane_channels_L2": (LANES, 3 * 32 + 7, 10, 2, dict(envs_per_block=32), K_ENV, 32, 1000),
    "env_fixed_map_L2": (FIXED_MAP, 2 * 64 + 9, 10, 2, None, K_ENV, None, 16),
    # more than 64 tiles: the BIG instantiation of whichever step kernel the batch gets
    "env_big_map_L3": (dict(random_map_width=9, random_map_height=9), 64 + 7, 12, 3, None, "true>", None, 1000),
    "traffic_L1": (TRAFFIC, 300, 6, 1, None, K_TRAFFIC, None, 1000),
    "traffic_rounds_L2": (TRAFFIC, 700, 8, 2, dict(kt_grid=4, kt_cap=5), K_TRAFFIC, None, 1000),
    "traffic_pairs_L2": (TRAFFIC, 800, 8, 2, dict(kt_grid=8), K_TRAFFIC, None, 1000),
    "traffic_wg256_L2": (TRAFFIC, 2 * 256 + 40, 8, 2, dict(envs_per_block=256), K_TRAFFIC, 256, 1000),
    "traffic_serial_L2": (TRAFFIC, 512, 8, 2, dict(kt_grid=8, kt_serial=1), K_TRAFFIC, None, 1000),
    "caller_L10": (CALLER, 2048, 25, 10, None, K_TRAFFIC, None, 1000),
    "caller_L100": (CALLER, 512, 110, 100, None, K_TRAFFIC, None, 1000),
    # What every reset path shares -- the obstacle streams of the new episode, its visited bitmap, its
    # start square and record -- through each step kernel: every square an obstacle, a penalty for visited
    # squares, and a limit under which every env resets six times or more in 20 ticks.  64 envs in
    # workgroups of 32 (the group-built images); 33 in one workgroup (a partly filled wave, an image
    # per lane); k_env's 256-env workgroup runs its resets compacted.
    "envq_obstacles_visited_L4": (OBST_VISITED, 64, 20, 4, dict(envs_per_block=32, queue_mode=1), K_ENVQ, 32, 1000),
    "envb_obstacles_visited_L4": (OBST_VISITED, 64, 20, 4, dict(envs_per_block=32, queue_mode=2), K_ENVB, 32, 1000),
    "env_obstacles_visited_L4": (OBST_VISITED, 64, 20, 4, dict(envs_per_block=256), K_ENV, 256, 1000),
    "envq_obstacles_visited_33_L4": (OBST_VISITED, 33, 20, 4, dict(envs_per_block=64, queue_mode=1), K_ENVQ, 64, 1000),
    "envb_obstacles_visited_33_L4": (OBST_VISITED, 33, 20, 4, dict(envs_per_block=64, queue_mode=2), K_ENVB, 64, 1000),
    "env_obstacles_visited_33_L4": (OBST_VISITED, 33, 20, 4, dict(envs_per_block=256), K_ENV, 256, 1000),
}


def _case_spec(conf):
    if isinstance(conf, str):
        return cfg.make_spec(conf)
    return _spec(conf)


def _check_regime(flags, L):
    """The rollout reaches what the case is for, counted on the restatement's flags."""
    assert (flags == 2).sum() > 0, "no env was truncated without terminating"
    if L >= 2:
        assert (flags & 1).sum() > 0, "no env terminated"
    else:
        assert (flags != 0).all(), "L = 1 ends every episode in every launch"


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_env_every_step_truncated(name):
    conf, n, T, L, tune, kernel, epb, distinct = CASES[name]
    run = _compare_run(_case_spec(conf), n, T, tune, name, min_distinct=distinct, max_episode_steps=L)
    # the case ran the kernel and the launch shape it is meant for
    assert run.kernel.endswith(kernel) if kernel == "true>" else run.kernel == kernel, run.kernel
    if epb is not None:
        assert run.launch[0] == epb, run.launch
    _check_regime(run.flags, L)
    if name.startswith("envq_one_round"):
        assert run.overflow > 0, "no overflow request was served: the one-round overflow path did not run"


def test_sub_batched_case_is_sub_batched():
    """env_wg256_sub32_L2's obs_sub knob takes effect at its shape: the sub-batched image needs less LDS."""
    from pgtg_amd.vector import PGTGVecEnv
    conf, n, _, L, tune, _, _, _ = CASES["env_wg256_sub32_L2"]
    lds = []
    for tn in (tune, dict(envs_per_block=256)):
        env = PGTGVecEnv(n, spec=_case_spec(conf), device=0, max_episode_steps=L, tune=tn)
        lds.append(env.launch_info())
        env.close()
    assert lds[0][0] == lds[1][0] == 256 and lds[0][1] < lds[1][1], lds


def test_envq_persistent_L2():
    """k_envq's persistent grid with more blocks than resident workgroups: the request lists of blocks
    that a workgroup takes from the counter, every env's episode ending every second launch."""
    from pgtg_amd.vector import PGTGVecEnv
    spec, T, L = _spec(CFG5), 6, 2
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for epb in (64, 128):  # (128 where 64 envs per workgroup do not keep the map queue on)
        tune = dict(envs_per_block=epb, queue_mode=1)
        probe = PGTGVecEnv(4 * epb, spec=spec, device=0, max_episode_steps=L, tune=tune)
        kern, shape, occ = probe.step_kernel(), probe.launch_info(), probe.occupancy()
        probe.close()
        if kern == K_ENVQ and shape[0] == epb:
            break
    assert kern == K_ENVQ and shape[0] == epb, (kern, shape)
    resident = occ * cus
    n = epb * (resident + resident // 2) + 21
    blocks = (n + epb - 1) // epb
    assert blocks > resident
    run = _compare_run(spec, n, T, tune, f"envq_persistent_L2 {n} envs", min_distinct=2 * FEW, max_episode_steps=L)
    assert run.kernel == K_ENVQ and run.launch[0] == epb, (run.kernel, run.launch)
    _check_regime(run.flags, L)


@pytest.mark.parametrize("name", ["3x3", "9x8"])
def test_truncation_inside_a_launch_of_several_ticks(name):
    """pgtg_step_many on a k_envq handle (k_envq<BIG, true>): 12 ticks in launches of 5 and 7 under
    a limit of 4 steps, 71 blocks of 16 envs on 8 workgroups.  The step count lives in the env record from
    tick to tick inside a launch, and a truncated env takes its ring head like a terminated one: every env's
    digest after each call against the restatement's, whose flags show truncations at ticks that are not
    the last of their launch (the first ones at tick 3)."""
    from pgtg_amd.digest import Digest
    from pgtg_amd.vector import PGTGVecEnv
    conf = CFG2 if name == "3x3" else dict(random_map_width=9, random_map_height=8)
    spec, n, T, L, calls = _spec(conf), 16 * 70 + 5, 12, 4, ((0, 5), (5, 12))
    ref, flags = oracle.rollout_digest(spec, n, T, ACT_SEED, max_episode_steps=L, flags_out=True)
    _check_regime(flags, L)
    print(name, "truncations", int((flags & 2).astype(bool).sum()), "terminations", int((flags & 1).sum()),
          "first truncation at tick", int(np.nonzero((flags & 2).any(1))[0][0]))
    inside = [t for lo, hi in calls for t in range(lo, hi - 1) if (flags[t] & 2).any()]
    assert 3 in inside and any(t >= 5 for t in inside), inside  # in both launches, not at their last tick
    assert len(np.unique(ref)) >= 1000, "degenerate digests"
    env = PGTGVecEnv(n, spec=spec, device=0, autoreset=True, max_episode_steps=L,
                     tune=dict(queue_mode=1, envs_per_block=16, queue_grid=8))
    try:
        env.reset(seed=0)
        assert env.step_kernel() == (K_ENVQ if name == "3x3" else "pgtg::k_envq<true>"), env.step_kernel()
        assert env.launch_info()[0] == 16
        acts = env.random_actions(T, ACT_SEED)
        dg, l0, e0 = Digest(env), env.step_launches(), env.counters()[1]
        for lo, hi in calls:
            env.step_many(acts[lo:hi])
            got = dg.step_digest().cpu().numpy().view(np.uint64)
            bad = np.argwhere(got != ref[hi - 1])
            assert bad.size == 0, f"{name} tick {hi - 1}: {len(bad)} env digests differ, first {bad[:8].ravel().tolist()}"
            trunc = env.truncated.cpu().numpy()
            assert np.array_equal(trunc, (flags[hi - 1] & 2) != 0), f"{name} tick {hi - 1}: truncated flags"
        assert env.step_launches() - l0 == len(calls)  # (several ticks per launch: the path this case is for)
        assert env.counters()[1] - e0 == int((flags != 0).sum())
        assert env.error_count()[0] == 0
    finally:
        env.close()


# ---- the outputs outside the digest, env by env ----------------------------------------------------

DIRECT = {
    # name: (config, envs, limit, tune)
    "traffic": (TRAFFIC, 300, 3, None),
    "traffic_pairs": (TRAFFIC, 800, 2, dict(kt_grid=8)),
    "next_subgoal": (dict(random_map_width=6, random_map_height=5, use_sliding_observation_window=True,
                          sliding_observation_window_size=3, use_next_subgoal_direction=True), 300, 3,
                     dict(envs_per_block=64)),
    "caller": (CALLER, 300, 4, None),
}


class _Limited:
    """OracleEnv behind gymnasium's TimeLimit with same-step auto-reset: the test's own step count."""

    def __init__(self, spec, L, seed):
        self.o, self.L, self.elapsed = OracleEnv(spec), L, 0
        self.first = self.o.reset(seed)

    def reset(self, seed):
        self.elapsed = 0
        return self.o.reset(seed)

    def step(self, a, autoreset=True):
        """(the step's result with `truncated` set, the result the caller sees after the reset or None,
        the car list at the end of the episode)"""
        r = self.o.step(int(a))
        self.elapsed += 1
        r["truncated"] = self.L > 0 and self.elapsed >= self.L
        if (r["terminated"] or r["truncated"]) and autoreset:
            cars = self.o.cars()
            return r, self.reset(None), cars
        return r, None, None


@pytest.mark.parametrize("name", sorted(DIRECT))
def test_truncation_outputs_env_by_env(name):
    """24 envs spread over the workgroups, waves and lanes, every step: both flags, reward, cost, the
    terminal position / velocity / next-subgoal direction / observation of a finished env, the new
    episode's outputs, and the car list after the step."""
    from pgtg_amd.vector import PGTGVecEnv
    conf, n, L, tune = DIRECT[name]
    spec, T = _spec(conf), 10
    rng = np.random.default_rng(n + L)
    idx = np.unique(np.concatenate([[0, 1, 15, 16, 63, 64, 127, 128, n // 2, n - 2, n - 1],
                                    rng.choice(n, 13, replace=False)]))
    tix = torch.as_tensor(idx, device="cuda")
    env = PGTGVecEnv(n, spec=spec, device=0, autoreset=True, max_episode_steps=L, tune=tune)
    try:
        env.reset(seed=11)
        orcs = [_Limited(spec, L, 11 + int(i)) for i in idx]
        acts = env.random_actions(T, 0xBEE)
        seen = set()
        for t in range(T):
            env.step_actions(acts[t])
            torch.cuda.synchronize()
            sel = lambda x: None if x is None else x.index_select(0, tix).cpu().numpy()  # noqa: E731
            a = sel(acts[t])
            m, fm, pos, vel, fpos, fvel = (sel(x) for x in (env.obs_map, env.final_map, env.position, env.velocity,
                                                            env.final_position, env.final_velocity))
            rew, cost, term, trunc, nsd, fnsd = (sel(x) for x in (env.reward, env.cost, env.terminated, env.truncated,
                                                                  env.nsd, env.final_nsd))
            for j, i in enumerate(idx):
                r, nr, _ = orcs[j].step(a[j])
                tag = f"{name} t{t} env{int(i)}"
                assert bool(term[j]) == r["terminated"] and bool(trunc[j]) == r["truncated"], tag + " flags"
                assert rew[j] == r["reward"], tag + " reward"
                if cost is not None:
                    assert cost[j] == r["cost"], tag + " cost"
                seen.add(int(r["terminated"]) | int(r["truncated"]) << 1)
                if nr is not None:
                    assert np.array_equal(fm[j], r["obs"]), tag + " terminal obs"
                    assert tuple(fpos[j]) == r["pos"] and tuple(fvel[j]) == r["vel"], tag + " terminal pos/vel"
                    if fnsd is not None:
                        assert fnsd[j] == r["nsd"], tag + " terminal nsd"
                    r = nr
                assert np.array_equal(m[j], r["obs"]), tag + " obs"
                assert tuple(pos[j]) == r["pos"] and tuple(vel[j]) == r["vel"], tag + " pos/vel"
                if nsd is not None:
                    assert nsd[j] == r["nsd"], tag + " nsd"
                if env.has_cars:
                    assert np.array_equal(env.cars(int(i)), orcs[j].o.cars()), tag + " cars"
        assert {0, 2} <= seen, seen  # running and truncated-only steps were compared
    finally:
        env.close()


# ---- the life cycle of the step count ---------------------------------------------------------------

LIFE = {
    "plain": dict(random_map_width=4, random_map_height=4, use_next_subgoal_direction=True),
    "traffic": dict(random_map_width=4, random_map_height=4, traffic_density=0.3),
}
L_LIFE = 6


# how the masked envs are reset: unseeded, seed + i, or a list of seeds
MASKED = {"plain_unseeded": ("plain", None), "traffic_seed": ("traffic", 900), "plain_seed_list": ("plain", "list")}


@pytest.mark.parametrize("name", sorted(MASKED))
def test_masked_reset_zeroes_the_step_count_of_the_masked_envs_only(name):
    """A masked reset at tick 3: from then on the batch truncates on two schedules, every env compared
    with the oracle at every step.  The envs outside the mask go on as if nothing had happened: a
    seeded masked reset leaves them the seeds that their later unseeded resets draw from."""
    from pgtg_amd.vector import PGTGVecEnv
    conf, how = MASKED[name]
    spec, n, T, L = _spec(LIFE[conf]), 150, 16, L_LIFE
    mask = np.arange(n) % 3 == 1
    seeds = None if how is None else [2000 + 7 * i for i in range(n)] if how == "list" else [how + i for i in range(n)]
    env = PGTGVecEnv(n, spec=spec, device=0, autoreset=True, max_episode_steps=L)
    try:
        env.reset(seed=40)
        orcs = [_Limited(spec, L, 40 + i) for i in range(n)]
        rng = np.random.default_rng(9)
        trunc_ticks = {True: set(), False: set()}  # masked?: ticks at which such an env was truncated only
        for t in range(T):
            if t == 3:
                env.reset(seed=seeds if how == "list" else how, mask=torch.as_tensor(mask))
                torch.cuda.synchronize()
                m = env.obs_map.cpu().numpy()
                for i in np.nonzero(mask)[0]:
                    r = orcs[i].reset(seeds[i] if seeds else None)
                    assert np.array_equal(m[i], r["obs"]), f"{name} masked reset obs env{i}"
                    if env.has_cars:
                        assert np.array_equal(env.cars(int(i)), orcs[i].o.cars()), f"{name} masked reset cars env{i}"
            # mostly standing still, so that most episodes last until their limit
            acts = np.where(rng.random(n) < 0.7, 4, rng.integers(0, 9, n)).astype(np.uint8)
            env.step(torch.as_tensor(acts))
            torch.cuda.synchronize()
            m, fm = env.obs_map.cpu().numpy(), env.final_map.cpu().numpy()
            rew, term, trunc = env.reward.cpu().numpy(), env.terminated.cpu().numpy(), env.truncated.cpu().numpy()
            for i in range(n):
                r, nr, _ = orcs[i].step(acts[i])
                tag = f"{name} t{t} env{i}"
                assert bool(term[i]) == r["terminated"] and bool(trunc[i]) == r["truncated"], tag + " flags"
                assert rew[i] == r["reward"], tag + " reward"
                if r["truncated"] and not r["terminated"]:
                    trunc_ticks[bool(mask[i])].add(t)
                if nr is not None:
                    assert np.array_equal(fm[i], r["obs"]), tag + " terminal obs"
                    r = nr
                assert np.array_equal(m[i], r["obs"]), tag + " obs"
                if env.has_cars and (t % 4 == 3 or nr is not None):
                    assert np.array_equal(env.cars(i), orcs[i].o.cars()), tag + " cars"
        # envs that never terminate: the unmasked ones run out at ticks 5 and 11, the masked ones at 8 and 14
        # (a masked env's count restarts at tick 3, so none of them can run out before tick 8)
        assert {5, 11} <= trunc_ticks[False] and {8, 14} <= trunc_ticks[True], trunc_ticks
        assert min(trunc_ticks[True]) == 8, trunc_ticks
    finally:
        env.close()


@pytest.mark.parametrize("name", sorted(LIFE))
def test_dump_load_restores_the_step_count(name):
    """dump_state at tick 4, four more ticks, load_state, the same four ticks: flags and digests are
    identical, the envs that run out of steps do so at tick 5 both times (their count of 4 steps is in
    the blob), and the whole rollout equals the oracle's."""
    from pgtg_amd.digest import Digest
    from pgtg_amd.vector import PGTGVecEnv
    spec, n, L = _spec(LIFE[name]), 200, L_LIFE
    ref, flags = oracle.rollout_digest(spec, n, 8, ACT_SEED, max_episode_steps=L, flags_out=True)
    # envs run out of steps in the replayed ticks: at tick 5 those that never finished, later the others
    assert (flags[5] == 2).sum() >= 5 and (flags[4:] == 2).sum() >= 10 and (flags[:4] & 1).any()
    env = PGTGVecEnv(n, spec=spec, device=0, autoreset=True, max_episode_steps=L)
    try:
        env.reset(seed=0)
        dg = Digest(env)

        def ticks(t0, t1):
            d, f = [], []
            for t in range(t0, t1):
                env.step_random(ACT_SEED, t)
                d.append(dg.step_digest().cpu().numpy().view(np.uint64))
                f.append((env.terminated.to(torch.uint8) | env.truncated.to(torch.uint8) << 1).cpu().numpy())
            return np.stack(d), np.stack(f)

        d0, f0 = ticks(0, 4)
        blob = env.dump_state()
        d1, f1 = ticks(4, 8)
        assert np.array_equal(np.concatenate([d0, d1]), ref) and np.array_equal(np.concatenate([f0, f1]), flags)
        env.load_state(blob)
        d2, f2 = ticks(4, 8)
        assert np.array_equal(f2, f1), f"{name}: flags after load differ at {np.argwhere(f2 != f1)[:5]}"
        assert np.array_equal(d2, d1), f"{name}: digests after load differ at {np.argwhere(d2 != d1)[:5]}"
    finally:
        env.close()


def test_truncated_env_without_autoreset_is_done_until_reset():
    """autoreset=False: a truncated env reports truncated = 1 with its own last observation, is not
    reset, and refuses another step like a terminated one (PGTG_E_DONE)."""
    from pgtg_amd import _abi
    from pgtg_amd.vector import PGTGVecEnv
    spec, n, L = _spec(dict(random_map_width=3, random_map_height=3, use_next_subgoal_direction=True)), 64, L_LIFE
    env = PGTGVecEnv(n, spec=spec, device=0, autoreset=False, max_episode_steps=L)
    try:
        env.reset(seed=7)
        orcs = [_Limited(spec, L, 7 + i) for i in range(n)]
        # standing still: no env terminates before its limit (one would stop the whole batch's steps)
        for t, acts in enumerate([np.full(n, 4)] * L):
            env.step(torch.as_tensor(acts.astype(np.uint8)))
            torch.cuda.synchronize()
            m, term, trunc = env.obs_map.cpu().numpy(), env.terminated.cpu().numpy(), env.truncated.cpu().numpy()
            pos = env.position.cpu().numpy()
            for i in range(n):
                r, _, _ = orcs[i].step(acts[i], autoreset=False)
                assert not r["terminated"], f"t{t} env{i}: the plan of actions was meant to keep every env running"
                assert not term[i] and bool(trunc[i]) == r["truncated"] == (t == L - 1), (t, i)
                assert np.array_equal(m[i], r["obs"]) and tuple(pos[i]) == r["pos"], (t, i)
        assert all(env.env_state(i)["elapsed"] == L for i in (0, 1, n // 2, n - 1))
        with pytest.raises(RuntimeError, match="Already done"):
            env.step(torch.as_tensor(np.full(n, 4, np.uint8)))
        cnt, code = env.error_count()
        assert cnt == n and code == _abi.PGTG_E_DONE
        # a reset ends the refusal and restarts the count
        env.reset(seed=7)
        for t in range(L):
            env.step(torch.as_tensor(np.full(n, 4, np.uint8)))
            assert bool(env.truncated.all()) == (t == L - 1) and not bool(env.terminated.any()), t
    finally:
        env.close()
