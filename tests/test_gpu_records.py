"""The packed state words (pgtg_amd/csrc/pgtg_records.h) where the host's packing, the device's unpacking and
the independent Python restatement (pgtg_amd/digest.py car_term) meet on extreme field values: agent fields
at +-30000 written by set_to_state and read back through env_state, and a car at (W-1, H-1) with the last
route and profile written by add_car / set_to_state, read back through cars() and digested on the device."""
import warnings

import numpy as np
import pytest

import helpers  # noqa: F401

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def env():
    from pgtg_amd import config as cfg
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec = cfg.make_spec(random_map_width=4, random_map_height=4, traffic_density=0.3)
    e = PGTGVecEnv(4, spec=spec, device=0, min_car_capacity=200)  # (above the 153 cars the density allows: room for add_car)
    e.reset(seed=77)
    yield e
    e.close()


def test_agent_fields_round_trip_at_the_16_bit_limits(env):
    untouched = ("phase", "terminated", "path_len", "elapsed", "spawn_counter", "used_subgoals", "seed", "n_cars",
                 "n_spawners", "next_car_id")
    # (envs 1 and 2: the host writes their cars to the slot rows; 0 and 3 keep their staging blocks for the test below)
    for i, (x, y, vx, vy) in [(1, (30000, -30000, -30000, 30000)), (2, (-30000, 30000, 30000, -30000)),
                              (1, (-1, 0, 0, -1)), (2, (35, 35, 1, -1))]:
        cars = [tuple(int(v) for v in c[:5]) for c in env.cars(i)]
        before = env.env_state(i)
        for flat in (True, False):
            env.set_to_state(i, x, y, vx, vy, flat, cars)
            st = env.env_state(i)
            assert (st["x"], st["y"], st["vx"], st["vy"], st["flat_tire"]) == (x, y, vx, vy, int(flat)), (i, flat, st)
            assert {k: st[k] for k in untouched} == {k: before[k] for k in untouched}, (i, flat)


def test_car_fields_host_pack_device_unpack_python_digest(env):
    from pgtg_amd.digest import car_term
    W = H = 4 * 9
    n0 = len(env.cars(1))
    env.add_car(1, W - 1, H - 1, 19, 4)  # the last square, route and driver profile: every field at its maximum
    c1 = env.cars(1)
    assert len(c1) == n0 + 1 and c1[-1, 1:].tolist() == [W - 1, H - 1, 19, 4, 0, 0]
    assert c1[-1, 0] == env.env_state(1)["next_car_id"] - 1
    env.set_to_state(2, 4, 4, 0, 0, False, [(0xFFFF, W - 1, 0, 19, 4), (7, 0, H - 1, 0, 0)])
    assert env.cars(2).tolist() == [[0xFFFF, W - 1, 0, 19, 4, 0, 0], [7, 0, H - 1, 0, 0, 0, 0]]
    # envs 0 and 3 still hold k_traffic's initial cars (their staging blocks), 1 and 2 the host's slot rows
    dg = env.car_digest().cpu().numpy().view(np.uint64)
    for i in range(4):
        assert int(dg[i]) == car_term(env.cars(i)) & M64, f"env {i}"
