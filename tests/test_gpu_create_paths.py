"""The host seams of the C ABI layer, at tiny sizes: which step-kernel instance a handle gets and
what it reports about it, a create that fails after its device allocations have begun, and the shape
check of state blobs and snapshots.

Every step-kernel case creates a handle at the smallest shape that selects its instance, asserts the
exact step_kernel() string and launch_info(), and steps it 10 ticks against per-env oracles
(helpers.vec_vs_oracle).  launch_info() is host arithmetic over the configuration and the batch size
alone (the LDS layout), so the pinned pairs hold on every device.  Every refusal checked here is a
host-side error code: nothing is launched for it."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import helpers
from digest_parity import _spec
from pgtg_amd import _abi
from pgtg_amd import config as cfg

pytestmark = pytest.mark.gpu

CFG3 = dict(random_map_width=3, random_map_height=3, random_map_obstacle_probability=0.5)
CFG5 = dict(random_map_width=5, random_map_height=5)
BIG = dict(random_map_width=9, random_map_height=8)  # 72 tiles: the BIG instances
TRAFFIC3 = dict(CFG3, traffic_density=0.2)
TRAFFIC5 = dict(random_map_width=5, random_map_height=5, traffic_density=0.5)
# lane channels keep the map queue off: k_env<false> where a random map without traffic would get k_envb
LANE_FEATURES = dict(features_to_include_in_observation=["walls", "goals", "car_spawner", "car_lane all right",
                                                         "traffic_light", "ice", "start", "final goal"])
LANES3 = dict(CFG3, **LANE_FEATURES)
# a rule that needs no traffic: the handle runs the rules' kernel without cars
RULE = {"name": "crossing", "tile_type": "1111", "velocity_range": [0, math.inf], "min_traffic": 0,
        "min_matching_traffic": 0, "maneuvers": []}
QUEUE, BLOCK = dict(queue_mode=1), dict(queue_mode=2)

K_TRAFFIC = " + pgtg::k_traffic"
ROWS = {
    # name: (config, envs, tune, rule at create, rule after the reset, step_kernel(), launch_info()
    #        [, step_kernel() and launch_info() once the rule is in])
    "no_traffic": (CFG3, 40, None, False, False, "pgtg::k_envb<false>", (16, 7340)),
    "env_lanes": (LANES3, 40, None, False, False, "pgtg::k_env<false, false>", (16, 15648)),
    "env_rules": (CFG3, 40, None, True, False, "pgtg::k_env<true, false>", (16, 15804)),
    "env_traffic": (TRAFFIC3, 40, None, False, False, "pgtg::k_env<true, false>" + K_TRAFFIC, (128, 44720)),
    "env_big": (dict(BIG, **LANE_FEATURES), 40, None, False, False, "pgtg::k_env<false, true>", (16, 17696)),
    "env_big_traffic": (dict(BIG, traffic_density=0.1), 40, None, False, False,
                        "pgtg::k_env<true, true>" + K_TRAFFIC, (32, 57648)),
    "envb": (CFG5, 256, BLOCK, False, False, "pgtg::k_envb<false>", (16, 9900)),
    "envq": (CFG5, 256, QUEUE, False, False, "pgtg::k_envq<false>", (16, 9900)),
    "envb_big": (BIG, 40, BLOCK, False, False, "pgtg::k_envb<true>", (16, 17580)),
    "envq_big": (BIG, 40, QUEUE, False, False, "pgtg::k_envq<true>", (16, 17580)),
    # k_envq handles given a rule afterwards: the instances that find the plan in the ring slot report
    # the name of their counterpart with plan rows
    "envq_then_rules": (CFG5, 256, QUEUE, False, True, "pgtg::k_envq<false>", (16, 9900),
                        "pgtg::k_env<true, false>", (16, 16316)),
    "envq_big_then_rules": (BIG, 40, QUEUE, False, True, "pgtg::k_envq<true>", (16, 17580),
                            "pgtg::k_env<true, true>", (16, 17852)),
    # a sub-batch LDS size above 64 KiB (tests/test_gpu_truncation.py traffic_wg256_L2): the launch needs
    # the raised dynamic-LDS limit of its instance
    "env_traffic_wg256": (TRAFFIC5, 2 * 256 + 40, dict(envs_per_block=256), False, False,
                          "pgtg::k_env<true, false>" + K_TRAFFIC, (256, 149680)),
}


def _case_spec(conf, rules=None):
    """rules: None the default rule list, else RULE alone that many times (0: an empty list)"""
    spec = _spec(conf)
    if rules is not None:
        spec.rules = []
        for _ in range(rules):
            cfg.add_rule(spec, RULE)
    return spec


def _make(n, spec, tune=None, min_car_capacity=0):
    from pgtg_amd.vector import PGTGVecEnv
    return PGTGVecEnv(n, spec=copy.deepcopy(spec), device=0, autoreset=True, tune=tune, min_car_capacity=min_car_capacity)


def _ten_ticks(vec, spec_orc, n, seed, tag):
    """10 ticks against per-env oracles: every env of a small batch, 64 spread over the blocks of a larger one"""
    envs = list(range(n)) if n <= 256 else sorted(set(np.linspace(0, n - 1, 64).astype(int).tolist()))
    helpers.vec_vs_oracle(vec, spec_orc, n, 10, seed, np.random.default_rng(seed), tag, envs)
    assert vec.error_count()[0] == 0, tag


@pytest.mark.parametrize("name", list(ROWS))
def test_step_kernel_instance(name):
    conf, n, tune, rule_first, rule_after, kernel, launch = ROWS[name][:7]
    with_rule = _case_spec(conf, 1) if rule_first or rule_after else _case_spec(conf)
    vec = _make(n, _case_spec(conf, 0) if rule_after else with_rule, tune)
    try:
        print(name, vec.step_kernel(), vec.launch_info(), vec.occupancy())
        assert vec.step_kernel() == kernel
        assert vec.launch_info() == launch
        assert vec.occupancy() >= 1
        if name == "env_traffic_wg256":
            assert vec.launch_info()[1] > 64 * 1024
        vec.reset(seed=300)
        if rule_after:
            vec.add_traffic_rule(RULE)
            print(name, "with the rule", vec.step_kernel(), vec.launch_info(), vec.occupancy())
            assert vec.step_kernel() == ROWS[name][7]
            assert vec.launch_info() == ROWS[name][8]
            assert vec.occupancy() >= 1
        _ten_ticks(vec, with_rule, n, 300, name)
    finally:
        vec.close()


def test_failed_create_after_the_allocations_and_a_good_one_right_after():
    """A car capacity whose reset scratch exceeds the LDS: choose_launch refuses it ("LDS budget exceeded"),
    after every state array of the handle has been allocated and the tables uploaded.  The create returns
    its code, pgtg_last_error(NULL) its message, and the next create steps bit-exactly."""
    L = _abi.lib()
    spec = _spec(TRAFFIC3)
    conf = _abi.config_struct(spec, True, None, 12000, None)
    h = C.c_void_p()
    rc = L.pgtg_create(C.byref(conf), 8, 0, C.byref(h))
    assert rc == _abi.PGTG_E_UNSUPPORTED and not h.value, (rc, h.value)
    assert L.pgtg_last_error(None).decode() == "LDS budget exceeded (traffic reset scratch)"
    vec = _make(40, spec)
    try:
        vec.reset(seed=77)
        _ten_ticks(vec, spec, 40, 77, "after the failed create")
    finally:
        vec.close()


# ---- the shape record of state blobs and snapshots -------------------------------------------------------

N_STATE = 24


def _state_handles(*more):
    """Two traffic handles of one shape and configuration, reset with different seeds, then `more`"""
    spec = _spec(TRAFFIC3)
    out = [_make(N_STATE, spec), _make(N_STATE, spec)]
    for kw in more:
        out.append(_make(N_STATE, _spec(dict(TRAFFIC3, **kw.get("conf", {}))), min_car_capacity=kw.get("cars", 0)))
    for k, e in enumerate(out):
        e.reset(seed=1000 * k)
    return out


def _outputs_equal(a, ia, b, ib, tag, stepped=True):
    """envs ia of a against envs ib of b: observation, position and cars; after a step of both also its results"""
    pairs = [(a.obs_map, b.obs_map), (a.position, b.position), (a.velocity, b.velocity), (a.car_digest(), b.car_digest())]
    if stepped:
        pairs += [(a.reward, b.reward), (a.terminated, b.terminated), (a.braking, b.braking)]
    for x, y in pairs:
        assert torch.equal(x[ia], y[ib]), tag


def test_blob_and_snapshot_round_trips_between_two_handles_of_equal_shape():
    a, b = _state_handles()
    snap = None
    try:
        acts = a.random_actions(16, 0xC0DE)
        for t in range(4):
            a.step_actions(acts[t])
        b.load_state(a.dump_state())
        every = slice(None)
        _outputs_equal(a, every, b, every, "observation after the load", stepped=False)
        for t in range(4, 8):
            a.step_actions(acts[t])
            b.step_actions(acts[t])
            _outputs_equal(a, every, b, every, f"blob: tick {t}")
        # envs 0..7 of a into envs 8..15 of b through a snapshot, then the same actions for both
        src, dst = list(range(8)), list(range(8, 16))
        b.reset(seed=4242)
        snap = a.snapshot(8)
        snap.save(a, env_idx=src, slot_idx=list(range(8)))
        snap.load(b, slot_idx=list(range(8)), env_idx=dst)
        _outputs_equal(a, src, b, dst, "observation after the snapshot load", stepped=False)
        for t in range(8, 16):
            row = torch.full((N_STATE,), 4, dtype=torch.uint8, device=a.device)
            row[dst] = acts[t][src]
            a.step_actions(acts[t])
            b.step_actions(row)
            _outputs_equal(a, src, b, dst, f"snapshot: tick {t}")
        assert a.error_count()[0] == 0 and b.error_count()[0] == 0
    finally:
        if snap is not None:
            snap.close()
        a.close()
        b.close()


def test_another_shape_and_another_configuration_are_refused():
    """A handle that differs in one shape field (the car capacity: 57 from the density, 64 asked for) and
    one that differs only in a probability: the blob and the snapshot name which it is."""
    a, b, shape, conf = _state_handles(dict(cars=64), dict(conf=dict(ice_probability=0.3)))
    snap = None
    try:
        blob = a.dump_state()
        snap = a.snapshot(4)
        snap.save(a, env_idx=[0, 1, 2, 3], slot_idx=[0, 1, 2, 3])
        dumped, made = "the state was dumped from a handle of ", "the snapshot was created from a handle of "
        for env, what in ((shape, "another shape"), (conf, "another configuration")):
            with pytest.raises(ValueError, match="^pgtg_load_state: " + dumped + what + "$"):
                env.load_state(blob)
            with pytest.raises(ValueError, match="^pgtg_snapshot_load: " + made + what + "$"):
                snap.load(env, slot_idx=[0, 1, 2, 3], env_idx=[0, 1, 2, 3])
            with pytest.raises(ValueError, match="^pgtg_snapshot_save: " + made + what + "$"):
                snap.save(env, env_idx=[0, 1, 2, 3], slot_idx=[0, 1, 2, 3])
        b.load_state(blob)  # (the blob and the snapshot themselves are good)
        snap.load(b, slot_idx=[0, 1, 2, 3], env_idx=[0, 1, 2, 3])
    finally:
        if snap is not None:
            snap.close()
        for e in (a, b, shape, conf):
            e.close()
