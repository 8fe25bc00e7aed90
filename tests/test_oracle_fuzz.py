"""The CPU oracle against the reference on the fuzz distributions (tests/fuzz_configs.py), from recorded
data alone: tests/golden/fuzz/traj_fuzz_NN.npz is random_kwargs(NN) run by the reference, the very
configuration tests/test_gpu_config_fuzz.py holds the HIP kernels to the oracle on; traj_wide_NN.npz
is wide_kwargs(NN), the rest of the constructor's surface (tools/gen_golden.py FUZZ_CASES).

The first tests are about the fixture set, not the code under test: a fuzz that never ends an episode
or never meets a car proves little, so what the set must contain is asserted from the recorded
arrays and `meta`.  Then every fixture is replayed through the oracle (helpers.replay_oracle:
observations, position and velocity, reward and cost, termination, next-subgoal direction, the
braking mask and car digests at the reset, every step and every auto-reset)."""
import numpy as np
import pytest

import fuzz_configs
import helpers

SUB = "fuzz"
NAMES = helpers.traj_names(SUB)
NARROW = [n for n in NAMES if n.startswith("fuzz_")]
WIDE = [n for n in NAMES if n.startswith("wide_")]
_cache: dict = {}


def load(name):
    if name not in _cache:
        _cache[name] = helpers.load_traj(name, SUB)
    return _cache[name]


def kwargs_of(name):
    return load(name)["meta"]["kwargs"]


def _jsonable(v):
    return list(v) if isinstance(v, tuple) else v


def test_the_set_is_the_fuzz_tests_own_configurations_and_about_forty_wide_ones():
    assert NARROW == [f"fuzz_{k:02d}" for k in range(40)]
    assert 36 <= len(WIDE) <= 48 and len(NARROW) + len(WIDE) == len(NAMES)
    for name in NAMES:
        k = int(name[5:])
        want = fuzz_configs.random_kwargs(k) if name.startswith("fuzz_") else fuzz_configs.wide_kwargs(k)
        assert kwargs_of(name) == {a: _jsonable(v) for a, v in want.items()}, name
        meta = load(name)["meta"]
        assert meta["N"] in (3, 4) and meta["T"] == 25 and meta["map_file"] is None
    modes = [load(n)["meta"]["action_mode"] for n in NAMES]
    assert min(modes.count("uniform"), modes.count("cautious")) >= len(NAMES) // 3


@pytest.mark.parametrize("name", NAMES)
def test_every_case_ends_an_episode_and_starts_another(name):
    d = load(name)
    assert d["terminated"].sum() >= 1 and len(d["reset_idx"]) >= 1
    assert len(d["reset_idx"]) == int(d["terminated"].sum())


def _tiles(kw):
    return kw["random_map_width"] * kw["random_map_height"]


def _both_random(kw):
    return kw.get("random_map_start_position") == "random" and kw.get("random_map_goal_position") == "random"


def test_wide_set_covers_what_the_narrow_distribution_never_draws():
    kws = [kwargs_of(n) for n in WIDE]

    def count(pred):
        return sum(1 for kw in kws if pred(kw))

    assert count(lambda kw: _tiles(kw) > 64) >= 4
    assert count(lambda kw: max(kw["random_map_width"], kw["random_map_height"]) > 8) >= 4
    assert count(lambda kw: min(kw["random_map_width"], kw["random_map_height"]) == 1) >= 3
    assert count(_both_random) >= 10
    assert count(lambda kw: _both_random(kw)
                 and kw.get("random_map_minimum_distance_between_start_and_goal") is not None) >= 4
    windows = lambda kw: kw["sliding_observation_window_size"] if kw["use_sliding_observation_window"] else None  # noqa: E731
    assert count(lambda kw: windows(kw) in (1, 6, 7)) >= 4
    assert count(lambda kw: kw["traffic_density"] >= 0.5) >= 4
    # start and goal given as tuples: with and without a direction, with a negative index
    tuples = [tuple(kw[a]) for kw in kws for a in ("random_map_start_position", "random_map_goal_position")
              if isinstance(kw.get(a), list)]
    assert {len(t) for t in tuples} == {2, 3} and any(-1 in t[:2] for t in tuples)
    assert count(lambda kw: any(float(kw[f"random_map_{o}_probability_weight"]) % 1 != 0 and
                                kw["random_map_obstacle_probability"] > 0
                                for o in ("ice", "broken_road", "sand", "traffic_light"))) >= 4
    assert count(lambda kw: max(kw["traffic_light_phases_duration"]) > 7) >= 4
    for colour in ("green", "yellow", "red"):
        assert count(lambda kw: f"traffic_light_{colour}" in kw["features_to_include_in_observation"]) >= 2
    # every parameter the narrow distribution leaves alone takes at least two values
    for a in ("random_map_start_position", "random_map_goal_position",
              "random_map_minimum_distance_between_start_and_goal", "max_allowed_deviation",
              "random_map_ice_probability_weight", "sliding_observation_window_size", "random_map_width",
              "random_map_height", "traffic_density", "traffic_light_phases_duration"):
        assert len({repr(kw.get(a)) for kw in kws}) >= 2, a
    assert {kw["max_allowed_deviation"] for kw in kws} >= {0, 3, 10, 25}
    assert {windows(kw) for kw in kws} >= {None, 1, 2, 3, 4, 5, 6, 7}
    assert {kw["traffic_density"] for kw in kws if _tiles(kw) <= 30} >= {0.0, 0.5, 1.0}
    # traffic stays on small maps, but for the sparse traffic on maps of more than 64 tiles
    for kw in kws:
        assert kw["traffic_density"] == 0 or _tiles(kw) <= 30 or (_tiles(kw) > 64 and kw["traffic_density"] <= 0.05)


def test_traffic_cases_have_cars_and_some_brake():
    traffic = [n for n in NAMES if helpers.has_traffic(load(n)["meta"])]
    assert len(traffic) >= 10
    for n in traffic:
        assert load(n)["ncars"].max() > 0, n
    assert sum(1 for n in traffic if load(n)["braking"].any()) >= 5
    for n in set(NAMES) - set(traffic):
        assert load(n)["ncars"].max() == 0 and not load(n)["braking"].any(), n


def test_every_obstacle_type_is_in_some_recorded_plan():
    seen = set()
    for n in NAMES:
        for episodes in load(n)["meta"]["plans"]:
            for plan in episodes:
                seen |= set(plan["otype"])
    assert seen >= {0, 1, 2, 3}, seen  # ice, broken road, sand, traffic light


def test_cost_cases_record_a_cost():
    cost = [n for n in NAMES if kwargs_of(n)["separate_reward_cost"]]
    assert len(cost) >= 10
    assert any(np.any(load(n)["cost"] != 0) for n in cost if n.startswith("fuzz_"))
    assert any(np.any(load(n)["cost"] != 0) for n in cost if n.startswith("wide_"))
    for n in set(NAMES) - set(cost):
        assert not np.any(load(n)["cost"] != 0), n


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_on_fuzz_configuration(name):
    bad = helpers.replay_oracle(load(name))
    assert not bad, bad[:10]
