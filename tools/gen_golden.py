"""Container-only: generate golden vectors by running the REFERENCE (imported through the
stand-ins of tools/refshim, see tools/refload.py) and write them as small compressed fixtures to
tests/golden/.  The reference itself never travels; only these data files do.

Vector semantics (what the batched product implements): env i is reset with seed `seed_base+i`,
then stepped with actions[t, i]; when it terminates it is reset unseeded (next spawn block), the
gymnasium/SB3 auto-reset convention.  Recorded per (t, i): the step's returned observation
(terminal one when it ended), reward, cost, terminated, position, velocity, next_subgoal_direction,
a digest of the car list, the braking flag, the byte of triggered rules (bit r: rule r's name is in
rule_engine.rule_triggers) and the post-reset observation of envs that were reset.

A case of RULE_CASES carries its own traffic rules: after construction the env's default rules are
removed and the case's are added through add_traffic_rule; the list is stored in the fixture's meta.

A case of FUZZ_CASES is a draw of tests/fuzz_configs.py (imported, not restated): fuzz_NN is
random_kwargs(NN), the configuration tests/test_gpu_config_fuzz.py runs as case NN, wide_NN is
wide_kwargs(NN).  They go to tests/golden/fuzz/ and are made on request only.

Usage:  python tools/gen_golden.py [name | prefix* ...]
        no argument: CONFIGS, RULE_CASES, the numpy vectors and the reproducibility fixture (not the fuzz cases)
        python tools/gen_golden.py 'fuzz_*' 'wide_*'    every fuzz case;  wide_07: that one
"""
import copy
import json
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refload  # noqa: E402

env_mod, mg, rparser, rmap, td, const = refload.load()
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
FUZZ_OUT = os.path.join(OUT, "fuzz")
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.append(_p)
import fuzz_configs  # noqa: E402  (tests/fuzz_configs.py)
TESTDATA = "/root/reference/tests/test_data"
ROUTES = sorted({f.split()[1] for t in td.TRAFFIC_LANES.values() for c in t for s in c for f in s
                 if f.startswith("car_lane") and f.split()[1] != "all"})
PROFILES = ["conservative", "normal", "aggressive", "elderly", "reckless"]
# obstacle mask ids: constants.OBSTACLE_MASK_NAMES order, then the traffic-light masks
OMASKS = list(const.OBSTACLE_MASK_NAMES) + [m for m in td.OBSTACLE_MASKS if m.startswith("traffic_light")]

CONFIGS = {
    # name: (kwargs, map_path, n_envs, steps, action_mode)
    "s3_default": (dict(random_map_width=3, random_map_height=3), None, 48, 100, "uniform"),
    "s3_obstacles": (dict(random_map_width=3, random_map_height=3, random_map_obstacle_probability=1.0),
                     None, 32, 60, "cautious"),
    "s3_obstacles_tlkey": (dict(random_map_width=3, random_map_height=3, random_map_obstacle_probability=0.7,
                                random_map_traffic_light_probability_weight=3,
                                features_to_include_in_observation=["walls", "goals", "traffic_light", "sand",
                                                                    "start", "used subgoal", "car_spawner",
                                                                    "car_lane all right", "nonexistent"]),
                           None, 16, 60, "cautious"),
    "s5_default": (dict(random_map_width=5, random_map_height=5), None, 24, 60, "uniform"),
    "s5_traffic05": (dict(random_map_width=5, random_map_height=5, traffic_density=0.5), None, 6, 40, "cautious"),
    "s4_train": (dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=0.2,
                      traffic_density=0.2, use_sliding_observation_window=True,
                      sliding_observation_window_size=5, use_next_subgoal_direction=True),
                 None, 12, 60, "cautious"),
    "s4_penalties": (dict(traffic_density=0.1, ignore_traffic_collisions=True, standing_still_penalty=3,
                          already_visited_position_penalty=2, final_goal_bonus=7, separate_reward_cost=True),
                     None, 12, 60, "cautious"),
    "s4_nsd_fixed": (dict(use_next_subgoal_direction=True, random_map_obstacle_probability=0.3,
                          sum_subgoals_reward=7), None, 16, 50, "uniform"),
    "tl_heavy": (dict(random_map_width=3, random_map_height=3, random_map_obstacle_probability=1.0,
                      random_map_traffic_light_probability_weight=1000, traffic_density=0.3,
                      traffic_light_phases_duration=(2, 1, 2), features_to_include_in_observation=[
                          "walls", "goals", "traffic", "traffic_light"]),
                 None, 8, 60, "cautious"),
    "random_start_goal": (dict(random_map_width=4, random_map_height=3, random_map_start_position="random",
                               random_map_goal_position="random",
                               random_map_minimum_distance_between_start_and_goal=3,
                               random_map_obstacle_probability=0.3), None, 24, 40, "uniform"),
    "start_goal_2tuple": (dict(random_map_width=3, random_map_height=4, random_map_start_position=(0, 2),
                               random_map_goal_position=(-1, -1), random_map_percentage_of_connections=0.8),
                          None, 16, 40, "uniform"),
    "tiny_1x1": (dict(random_map_width=1, random_map_height=1, traffic_density=0.5), None, 8, 30, "uniform"),
    "strip_2x1_full": (dict(random_map_width=2, random_map_height=1, random_map_percentage_of_connections=1.0),
                       None, 8, 30, "uniform"),
    # maps of > 64 tiles (the 256-bit generator path): the reference's own integration-test env
    # (tests/test_integration.py:25-42, 9x9), a 10x10 with obstacles and penalties, a 16x16 with traffic
    "s9_integration": (dict(random_map_width=9, random_map_height=9, random_map_percentage_of_connections=0.9,
                            random_map_obstacle_probability=0.8, random_map_broken_road_probability_weight=2,
                            random_map_ice_probability_weight=4, random_map_sand_probability_weight=8,
                            render_mode="pil_image", final_goal_bonus=100, standing_still_penalty=5,
                            ice_probability=0.5, street_damage_probability=0.2, traffic_density=0.02,
                            ignore_traffic_collisions=True), None, 8, 40, "uniform"),
    "s10_obstacles": (dict(random_map_width=10, random_map_height=10, random_map_obstacle_probability=0.5,
                           use_next_subgoal_direction=True, already_visited_position_penalty=1,
                           separate_reward_cost=True), None, 6, 50, "cautious"),
    "s16_traffic": (dict(random_map_width=16, random_map_height=16, random_map_percentage_of_connections=0.7,
                         traffic_density=0.1, use_sliding_observation_window=True,
                         sliding_observation_window_size=6), None, 3, 30, "cautious"),
    "fixed_1x1_traffic": (dict(traffic_density=1, ignore_traffic_collisions=True), "1x1_map", 4, 40, "still"),
    "fixed_crossing": (dict(traffic_density=0.5), "1x1_crossing_map", 4, 40, "cautious"),
    "fixed_4x1": (dict(sum_subgoals_reward=444), "4x1_map.json", 4, 40, "cautious"),
    "fixed_deadends": (dict(traffic_density=0.3, ignore_traffic_collisions=True), "map_with_all_deadends",
                       3, 30, "cautious"),
}


# ---- the fuzz distributions of tests/fuzz_configs.py ------------------------------------------------
# wide_kwargs(k) for these k: chosen so that the recorded data meets the conditions that
# tests/test_oracle_fuzz.py asserts of the set (every case ends an episode; maps of more than 64
# tiles, strips, random start and goal, windows of 1, 6 and 7, dense traffic, braking, every obstacle
# type, a cost) and that every step-kernel instance gets several configurations.  0..40 but for 4, 8,
# 10 and 37 (the reference takes more than 5 s for each: large maps with large windows); 43 and 50 for
# the map-queue kernels on maps of up to 64 tiles, 76 for a map above 64 tiles with lane channels.  No
# k was left out because the reference raised.
WIDE_KS = [k for k in range(41) if k not in (4, 8, 10, 37)] + [43, 50, 76]
FUZZ_STEPS = 25


def _fuzz_cases():
    """name: (kwargs, map_path, n_envs, steps, action_mode); by k, so that a case does not depend on
    which others are in the table: 4, 4, 3, 3 envs and uniform, cautious actions in turn"""
    draws = [(f"fuzz_{k:02d}", k, fuzz_configs.random_kwargs(k)) for k in range(40)]
    draws += [(f"wide_{k:02d}", k, fuzz_configs.wide_kwargs(k)) for k in WIDE_KS]
    return {name: (kw, None, 4 if k % 4 < 2 else 3, FUZZ_STEPS, "uniform" if k % 2 == 0 else "cautious")
            for name, k, kw in draws}


FUZZ_CASES = _fuzz_cases()


# ---- cases with their own traffic rules ------------------------------------------------------------
AGENTS4 = ["south_to_north", "west_to_east", "north_to_south", "east_to_west"]
AGENTS6 = AGENTS4 + ["stationary", "near_goal"]
SQRT2, SQRT5 = 2 ** 0.5, 5 ** 0.5


def rule(name, tile, vr, mt, mm, maneuvers):
    return {"name": name, "tile_type": tile, "velocity_range": list(vr), "min_traffic": mt,
            "min_matching_traffic": mm, "maneuvers": maneuvers}


def every(agents, routes):
    return [{"agent": a, "traffic": list(routes)} for a in agents]


EW = ["west_to_east", "east_to_west"]
NS = ["north_to_south", "south_to_north"]
FAST = [1.5, 10]  # fires from speed 2 on only, so the agent can creep through the tile at speed 1 or sqrt(2)
# (a rule that fires at the speeds one acceleration gives pins the agent for as long as the cars stay)
RULE_SETS = {
    "default": None,  # the constructor's two rules
    # thresholds above 1 on straight and corner tiles
    "thr_a": [rule("two_in_0101", "0101", FAST, 2, 2, every(AGENTS6, ROUTES)),
              rule("three_in_0101", "0101", FAST, 3, 2, every(AGENTS6, ROUTES)),
              rule("two_in_1010", "1010", FAST, 2, 1, every(AGENTS6, ROUTES)),
              rule("three_in_1010", "1010", FAST, 3, 3, every(AGENTS6, ROUTES))] +
             [rule(f"two_in_{t}", t, FAST, 2, 2, every(AGENTS6, ROUTES)) for t in ("1100", "0110", "0011", "1001")],
    # ... and on T-junctions and the crossing, some matching only part of the routes
    "thr_b": [rule("two_in_1110", "1110", FAST, 2, 2, every(AGENTS6, ROUTES)),
              rule("three_ns_in_1010", "1010", FAST, 3, 3, every(AGENTS6, NS)),
              rule("two_ew_in_0101", "0101", FAST, 2, 2, every(AGENTS6, EW)),
              rule("three_of_two_ew_in_0101", "0101", FAST, 3, 2, every(AGENTS6, EW)),
              rule("two_in_1101", "1101", FAST, 2, 2, every(AGENTS6, ROUTES)),
              rule("three_in_0111", "0111", FAST, 3, 3, every(AGENTS6, ROUTES)),
              rule("two_in_1011", "1011", FAST, 2, 2, every(AGENTS6, ROUTES)),
              rule("three_in_1111", "1111", FAST, 3, 3, every(AGENTS6, ROUTES))],
    # one route named by two (three) maneuvers of one agent direction: a single such car counts twice
    "dup": [rule("twice", "1111", FAST, 1, 2, every(["west_to_east"], NS[:1]) * 2),
            rule("once", "1111", FAST, 1, 2, every(["west_to_east"], NS[:1])),
            rule("thrice", "1111", FAST, 1, 3, every(["west_to_east"], NS[1:]) * 3),
            rule("twice_in_one_list", "1111", FAST, 1, 2, every(["west_to_east"], NS[1:] * 2))],
    # agent directions 4 and 5: no goal square in compass reach, at speed 0 and above
    "still": [rule("near_goal_moving", "1111", [1, 10], 1, 1, every(["near_goal"], ROUTES)),
              rule("stationary_0", "1111", [0, 0], 1, 1, every(["stationary"], ROUTES)),
              rule("stationary_two", "1111", [0, 0.05], 2, 2, every(["stationary"], ROUTES[:10])),
              rule("near_goal_slow", "1111", [0.1, SQRT2], 2, 1, every(["near_goal"], ROUTES[10:])),
              rule("stationary_never", "1111", [0.1, 3], 0, 1, every(["stationary"], ROUTES)),
              rule("near_goal_never", "1111", [0, 0], 0, 1, every(["near_goal"], ROUTES))],
    # all eight slots, speed bounds at equality and at irrational endpoints
    "eight": [rule("v_0_0", "1111", [0, 0], 1, 1, every(["stationary"], ROUTES)),
              rule("v_0_1", "1111", [0, 1], 1, 1, every(["stationary", "near_goal"], ROUTES)),
              rule("v_1_sqrt2", "1111", [1, SQRT2], 1, 1, every(["near_goal"], ROUTES)),
              rule("v_sqrt2_sqrt2", "1111", [SQRT2, SQRT2], 1, 1, every(["near_goal"], ROUTES)),
              rule("v_1.5_sqrt5", "1111", [1.5, SQRT5], 1, 1, every(["west_to_east"], ROUTES)),
              rule("v_2_3", "1111", [2, 3], 2, 2, every(["west_to_east"], ROUTES)),
              rule("v_1.5_inf", "1111", [1.5, float("inf")], 3, 1, every(["west_to_east", "near_goal"], ROUTES)),
              rule("v_2_1e9", "1111", [2, 1e9], 4, 4, every(AGENTS6, ROUTES))],
    # names the engine never matches, beside two rules that fire
    "malformed": [rule("tile_5_chars", "11110", [0, 10], 0, 0, every(AGENTS6, ROUTES)),
                  rule("tile_letters", "1x11", [0, 10], 0, 0, every(AGENTS6, ROUTES)),
                  rule("tile_int", 1111, [0, 10], 0, 0, every(AGENTS6, ROUTES)),
                  rule("unknown_agent", "1111", [0, 10], 1, 1, every(["sideways", "north"], ROUTES)),
                  rule("unknown_routes", "1111", [0, 10], 1, 1, every(AGENTS6, ["up_to_down", "all"])),
                  rule("any_car", "1111", FAST, 1, 1, every(AGENTS6, ROUTES)),
                  rule("no_car_needed", "1111", FAST, 0, 0, [])],
    # the fixed maps' tile types
    "directions": [rule(f"{n}in_{t}", t, [2.5, 10], mt, mt, every(AGENTS6, ROUTES))
                   for t in ("1001", "1010") for n, mt in (("", 1), ("two_", 2))],
    "deadends": [rule(f"{n}in_{t}", t, [2.5, 10], mt, mt, every(AGENTS6, ROUTES))
                 for t in ("1101", "0101", "0010") for n, mt in (("", 1), ("two_", 2))],
    "straight": [rule("any", "0101", FAST, 1, 1, every(AGENTS6, ROUTES)),
                 rule("oncoming_twice", "0101", FAST, 2, 2, every(["west_to_east"], ["east_to_west"])),
                 rule("same_way_three", "0101", [1.5, 3], 3, 3, every(["west_to_east"], ["west_to_east"]))],
}
# name: (kwargs, map_path, n_envs, steps, action_mode, rule set, seed_base, action seed,
#        rules that must have fired (None: all), rules that must never have fired)
RULE_CASES = {
    "rules_default_s5": (dict(random_map_width=5, random_map_height=5, traffic_density=0.5,
                              random_map_start_position="random", random_map_goal_position="random"), None, 8, 40,
                         "cautious", "default", 400, 4, None, ()),
    "rules_thr_a_s4": (dict(random_map_width=4, random_map_height=4, traffic_density=1.0,
                            ignore_traffic_collisions=True, random_map_start_position="random",
                            random_map_goal_position="random"), None, 8, 40, "uniform", "thr_a", 0, 12345, None, ()),
    "rules_thr_b_s5": (dict(random_map_width=5, random_map_height=5, traffic_density=0.5,
                            ignore_traffic_collisions=True, random_map_start_position="random",
                            random_map_goal_position="random"), None, 8, 40, "uniform", "thr_b", 0, 12345, None, ()),
    "rules_dup_crossing": (dict(traffic_density=0.5, ignore_traffic_collisions=True), "1x1_crossing_map", 8, 40,
                           "cautious", "dup", 0, 12345, None, ()),
    "rules_still_crossing": (dict(traffic_density=0.5, ignore_traffic_collisions=True), "1x1_crossing_map", 6, 40,
                             "cautious", "still", 0, 12345, (0, 1, 2, 3), (4, 5)),
    "rules_eight_crossing": (dict(traffic_density=0.5, ignore_traffic_collisions=True), "1x1_crossing_map", 6, 40,
                             "cautious", "eight", 0, 12345, None, ()),
    "rules_malformed_crossing": (dict(traffic_density=0.5, ignore_traffic_collisions=True), "1x1_crossing_map", 4,
                                 30, "cautious", "malformed", 0, 12345, (5, 6), (0, 1, 2, 3, 4)),
    "rules_fixed_directions": (dict(traffic_density=0.7, ignore_traffic_collisions=True),
                               "map_with_all_directions", 6, 60, "uniform", "directions", 200, 2, None, ()),
    "rules_fixed_deadends": (dict(traffic_density=0.7, ignore_traffic_collisions=True), "map_with_all_deadends",
                             6, 60, "uniform", "deadends", 100, 1, None, ()),
    "rules_fixed_4x1": (dict(traffic_density=0.8, ignore_traffic_collisions=True), "4x1_map.json", 6, 40,
                        "cautious", "straight", 0, 12345, None, ()),
}
# pairs (a, b): some step must have fired rule a without rule b
FIRED_WITHOUT = {"rules_dup_crossing": [[0, 1], [2, 3]]}


def actions_for(mode, T, N, seed):
    rng = np.random.default_rng(seed)
    if mode == "uniform":
        return rng.integers(0, 9, size=(T, N)).astype(np.uint8)
    if mode == "still":
        return np.full((T, N), 4, np.uint8)
    # cautious: mostly coast, sometimes accelerate, keeps episodes alive for many ticks
    a = rng.integers(0, 9, size=(T, N)).astype(np.uint8)
    keep = rng.random((T, N)) < 0.6
    a[keep] = 4
    return a


def car_rows(env):
    return np.array([[c.id, c.position.x, c.position.y, ROUTES.index(c.route), PROFILES.index(c.driver_profile.value),
                      c.patience_counter, int(c.last_action_delay)] for c in env.cars], dtype=np.int32).reshape(-1, 7)


def digest(arr):
    return zlib.crc32(np.ascontiguousarray(arr, dtype=np.int32).tobytes())


def obs_stack(obs, keys):
    return np.stack([np.asarray(obs["map"][k], dtype=np.uint8) for k in keys])


def plan_rows(env):
    mp = env.map_plan
    ex, ot, om = [], [], []
    for y in range(mp.height):
        for x in range(mp.width):
            t = mp.tiles[y][x]
            ex.append(sum(int(b) << i for i, b in enumerate(t["exits"])))
            ot.append(const.OBSTACLE_NAMES.index(t["obstacle_type"]) if t.get("obstacle_type") else -1)
            om.append(OMASKS.index(t["obstacle_mask"]) if t.get("obstacle_mask") else -1)
    dirs = ["north", "east", "south", "west"]
    return dict(w=mp.width, h=mp.height, exits=ex, otype=ot, omask=om,
                start=[int(mp.start[0]), int(mp.start[1]), dirs.index(mp.start[2])],
                goal=[int(mp.goal[0]), int(mp.goal[1]), dirs.index(mp.goal[2])])


def run(name, write=True, seeds=None):
    rules, seed_base, act_seed = None, 0, 12345
    if name in RULE_CASES:
        kwargs, map_file, N, T, mode, rule_set, seed_base, act_seed, expect, never = RULE_CASES[name]
        if seeds:  # (a seed search, write=False)
            seed_base, act_seed = seeds
        rules = RULE_SETS[rule_set]
    elif name in FUZZ_CASES:
        kwargs, map_file, N, T, mode = FUZZ_CASES[name]
    else:
        kwargs, map_file, N, T, mode = CONFIGS[name]
    map_path = os.path.join(TESTDATA, map_file) if map_file else None
    acts = actions_for(mode, T, N, act_seed)
    cwd = os.getcwd()
    os.chdir(REPO)
    envs = [env_mod.PGTGEnv(map_path, **kwargs) for _ in range(N)]
    os.chdir(cwd)
    if rules is not None:
        for e in envs:
            for r in list(e.rule_engine.rules):
                e.remove_traffic_rule(r.name)
            for r in rules:
                e.add_traffic_rule(copy.deepcopy(r))
    rule_names = [r.name for r in envs[0].rule_engine.rules]
    first = [e.reset(seed=seed_base + i)[0] for i, e in enumerate(envs)]
    keys = list(first[0]["map"].keys())
    # The reference adds the generic features by iterating over a set of their names, so their order
    # changes with the interpreter's string hashing: record them in the order of the feature list
    # instead (a regenerated fixture is then the same file; the tests map keys to channels by name).
    feats = list(envs[0].features_to_include_in_observation)
    lights = [f"traffic_light_{c}" for c in ("green", "yellow", "red")] if "traffic_light" in feats else []
    generic = [k for k in keys if k in feats and k not in ["walls", "goals", "traffic"] + lights]
    keys = [k for k in keys if k not in generic] + sorted(generic, key=feats.index)
    W =np.asarray(first[0]["map"][keys[0]]).shape[0]
    C = len(keys)
    init_obs = np.stack([obs_stack(o, keys) for o in first])
    init_pos = np.array([o["position"] for o in first], np.int32)
    init_nsd = np.array([o.get("next_subgoal_direction", -1) for o in first], np.int32)
    obs = np.zeros((T, N, C, W, W), np.uint8)
    pos = np.zeros((T, N, 2), np.int32)
    vel = np.zeros((T, N, 2), np.int32)
    rew = np.zeros((T, N), np.float64)
    cost = np.zeros((T, N), np.float64)
    term = np.zeros((T, N), np.uint8)
    nsd = np.zeros((T, N), np.int32)
    brake = np.zeros((T, N), np.uint8)
    trig = np.zeros((T, N), np.uint8)
    cars_dig = np.zeros((T, N), np.uint32)
    ncars = np.zeros((T, N), np.int32)
    reset_obs, reset_idx, reset_pos, reset_nsd, reset_dig = [], [], [], [], []
    plans = [[plan_rows(e)] for e in envs]
    init_cars = [car_rows(e) for e in envs]
    cars_final = []
    for t in range(T):
        for i, e in enumerate(envs):
            o, r, te, tr, info = e.step(int(acts[t, i]))
            obs[t, i] = obs_stack(o, keys)
            pos[t, i] = o["position"]
            vel[t, i] = o["velocity"]
            rew[t, i] = float(r)
            cost[t, i] = float(info.get("cost", 0))
            term[t, i] = bool(te)
            nsd[t, i] = o.get("next_subgoal_direction", -1)
            brake[t, i] = bool(e.braking_applied)
            trig[t, i] = sum(1 << k for k, n in enumerate(rule_names) if n in e.rule_engine.rule_triggers)
            cr = car_rows(e)
            cars_dig[t, i] = digest(cr)
            ncars[t, i] = len(cr)
            if te:
                o2, _ = e.reset()
                reset_obs.append(obs_stack(o2, keys))
                reset_idx.append((t, i))
                reset_pos.append(o2["position"])
                reset_nsd.append(o2.get("next_subgoal_direction", -1))
                reset_dig.append(digest(car_rows(e)))
                plans[i].append(plan_rows(e))
    for e in envs:
        cars_final.append(car_rows(e))
    meta = dict(name=name, kwargs=kwargs, map_file=map_file, N=N, T=T, seed_base=seed_base, keys=keys,
                action_mode=mode, plans=plans)
    if name in RULE_CASES:
        meta.update(action_seed=act_seed, rule_names=rule_names, never_fired=list(never),
                    expect_fired=list(range(len(rule_names))) if expect is None else list(expect),
                    fired_without=FIRED_WITHOUT.get(name, []))
        if rules is not None:
            meta["rules"] = rules
    R = len(reset_idx)
    if not write:
        return trig
    np.savez_compressed(
        os.path.join(FUZZ_OUT if name in FUZZ_CASES else OUT, f"traj_{name}.npz"),
        meta=np.frombuffer(json.dumps(meta).encode(), np.uint8), actions=acts,
        init_obs=init_obs, init_pos=init_pos, init_nsd=init_nsd,
        init_cars_dig=np.array([digest(c) for c in init_cars], np.uint32),
        obs=obs, pos=pos, vel=vel, reward=rew, cost=cost, terminated=term, nsd=nsd, braking=brake,
        cars_dig=cars_dig, ncars=ncars,
        reset_idx=np.array(reset_idx, np.int32).reshape(R, 2),
        reset_obs=np.array(reset_obs, np.uint8).reshape(R, C, W, W),
        reset_pos=np.array(reset_pos, np.int32).reshape(R, 2),
        reset_nsd=np.array(reset_nsd, np.int32).reshape(R),
        reset_cars_dig=np.array(reset_dig, np.uint32).reshape(R),
        cars_final=np.concatenate(cars_final) if cars_final else np.zeros((0, 7), np.int32),
        cars_final_n=np.array([len(c) for c in cars_final], np.int32), triggered=trig,
    )
    return R, int(term.sum())


def reproducibility_fixture():
    """The reference's own golden trajectory (tests/test_data/reproducibility_data.py) as data."""
    import importlib.util
    sp = importlib.util.spec_from_file_location("repro", os.path.join(TESTDATA, "reproducibility_data.py"))
    m = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(m)
    fx = m.COMPLICATED_ENVIRONMENT
    keys = list(fx["observation_list"][0]["map"].keys())
    obs = np.stack([obs_stack(o, keys) for o in fx["observation_list"]])
    np.savez_compressed(
        os.path.join(OUT, "ref_complicated_environment.npz"),
        meta=np.frombuffer(json.dumps(dict(kwargs=fx["environment_arguments"], seed=fx["seed"], keys=keys)).encode(),
                           np.uint8),
        actions=np.array(fx["action_list"], np.int32), obs=obs,
        pos=np.array([o["position"] for o in fx["observation_list"]], np.int32),
        vel=np.array([o["velocity"] for o in fx["observation_list"]], np.int32),
        reward=np.array(fx["reward_list"], np.float64),
        terminated=np.array(fx["terminated_list"], np.uint8),
        truncated=np.array(fx["truncated_list"], np.uint8))


def rng_vectors():
    """numpy Generator known answers for the restated primitives (numpy 2.2.6 here; locked 1.26.4)."""
    out = {}
    seeds = np.array([0, 1, 7, 123456789, 2**32 + 5, 2**63 + 11], np.uint64)
    keys = np.array([0, 1, 4, 5, 9, 1000], np.uint32)
    st = np.zeros((len(seeds), len(keys), 4), np.uint64)
    raw = np.zeros((len(seeds), len(keys), 8), np.uint64)
    for a, s in enumerate(seeds):
        for b, k in enumerate(keys):
            g = np.random.PCG64(np.random.SeedSequence(int(s), spawn_key=(int(k),)))
            sd = g.state["state"]
            st[a, b] = [sd["state"] >> 64, sd["state"] & (2**64 - 1), sd["inc"] >> 64, sd["inc"] & (2**64 - 1)]
            raw[a, b] = g.random_raw(8)
    out["seeds"], out["keys"], out["pcg_state"], out["pcg_raw"] = seeds, keys, st, raw
    # mixed draw script on one stream
    g = np.random.Generator(np.random.PCG64(np.random.SeedSequence(42, spawn_key=(3,))))
    script, vals = [], []
    prng = np.random.default_rng(7)
    for t in range(2000):
        kind = int(prng.integers(0, 4))
        if kind == 0:
            script.append((0, 0)); vals.append(g.random())
        elif kind == 1:
            n = int(prng.integers(1, 3000)); script.append((1, n)); vals.append(float(g.integers(0, n)))
        elif kind == 2:
            script.append((2, 0)); vals.append(float(g.choice(5, p=[0.25, 0.35, 0.2, 0.15, 0.05])))
        else:
            script.append((3, 0)); vals.append(float(g.integers(1, 4)))
    out["script"] = np.array(script, np.int64)
    out["script_vals"] = np.array(vals, np.float64)
    g = np.random.Generator(np.random.PCG64(np.random.SeedSequence(9, spawn_key=(1,))))
    nr = []
    for pop, k in [(10, 3), (474, 237), (18, 18), (5, 1), (2025, 1012), (1, 1), (729, 100)]:
        nr.append(np.array([pop, k] + list(g.choice(pop, size=k, replace=False)), np.int64))
    out["noreplace"] = np.concatenate(nr)
    np.savez_compressed(os.path.join(OUT, "rng_numpy.npz"), **out)


if __name__ == "__main__":
    os.makedirs(FUZZ_OUT, exist_ok=True)
    every = list(CONFIGS) + list(RULE_CASES) + list(FUZZ_CASES)
    names = []
    for a in sys.argv[1:]:  # a name, or a prefix with a trailing *
        hit = [n for n in every if n.startswith(a[:-1])] if a.endswith("*") else [a]
        if not hit or hit[0] not in every:
            sys.exit(f"no case {a!r}")
        names += hit
    names = names or list(CONFIGS) + list(RULE_CASES)
    if not sys.argv[1:]:
        rng_vectors()
        reproducibility_fixture()
    for n in names:
        import time
        t0 = time.time()
        R, nt = run(n)
        print(f"{n}: resets={R} terminations={nt} {time.time() - t0:.1f}s", flush=True)
