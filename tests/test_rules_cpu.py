"""Traffic rules on the host: `config.compile_rule` against numpy's norm, the compiled fields against
the struct fields that carry them to the device and to the oracle, and what the rule fixtures
(tests/golden/traj_rules_*.npz, tools/gen_golden.py RULE_CASES) recorded from the reference."""
import ctypes
import math

import numpy as np
import pytest

import helpers
from oracle import oracle as orc
from pgtg_amd import _abi
from pgtg_amd import config as C

SQRT2, SQRT5 = math.sqrt(2.0), math.sqrt(5.0)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
SPEED_SQ_TOP = 2 * 30000 ** 2  # the step refuses |vx| or |vy| > 30 000, so the device compares no larger s
ENDPOINTS = [0, 0.1, 0.5, 1, SQRT2, 1.5, 2, SQRT5, 3, 10, 1e9, math.inf]
V = np.arange(-64, 65)
S2 = (V[:, None] ** 2 + V[None, :] ** 2).astype(np.int64)  # [vx, vy]
NORM = np.linalg.norm(np.stack(np.meshgrid(V, V, indexing="ij"), -1).astype(np.int64), axis=-1)
assert NORM[64 + 3, 64 + 4] == 5.0


def _rule(lo=0.5, hi=10.0, mt=1, mm=1, maneuvers=(), tile="1111", name="r"):
    return {"name": name, "tile_type": tile, "velocity_range": [lo, hi], "min_traffic": mt,
            "min_matching_traffic": mm, "maneuvers": list(maneuvers)}


def _struct(rule):
    arr = (_abi.PgtgRule * _abi.MAX_RULES)()
    assert _abi.fill_rules(arr, [rule]) == 1
    return arr[0]


def _fits(value, ctype):
    return ctype(value).value == value


RANGES = [(lo, hi) for lo in ENDPOINTS for hi in ENDPOINTS if lo <= hi] + [(2.0, 1.0), (10.0, 0.5), (math.inf, 0.0)]


@pytest.mark.parametrize("lo,hi", RANGES)
def test_speed_window_equals_numpy_norm_for_every_velocity_up_to_64(lo, hi):
    """speed_sq_min <= vx^2 + vy^2 <= speed_sq_max, read back from the device's struct, exactly when
    lo <= np.linalg.norm([vx, vy]) <= hi (pgtg/environment.py:245-246)."""
    r = _struct(C.compile_rule(_rule(lo, hi)))
    got = (r.speed_sq_min <= S2) & (S2 <= r.speed_sq_max)
    want = (lo <= NORM) & (NORM <= hi)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5] - 64


@pytest.mark.parametrize("lo,hi", [(0, math.inf), (0.5, 46340.95), (0, 46341), (0, 1e9), (1e9, math.inf),
                                   (46341, 1e6), (math.inf, math.inf), (0, math.nan), (math.nan, 10)])
def test_compiled_fields_fit_the_struct_fields(lo, hi):
    """ctypes wraps an out-of-range int without complaint: [0, inf] used to reach the device as
    speed_sq_max = -2^31, "never" instead of "always"."""
    c = C.compile_rule(_rule(lo, hi, mt=2 ** 40, mm=-2 ** 40, maneuvers=[{"agent": "stationary", "traffic": C.ROUTES}] * 300))
    fields = dict(_abi.PgtgRule._fields_)
    for f in ("tile_exits", "speed_sq_min", "speed_sq_max", "min_traffic", "min_matching_traffic"):
        assert _fits(getattr(c, f), fields[f]), (f, getattr(c, f))
    for f in ("tile_exits", "min_traffic", "min_matching_traffic"):
        assert _fits(getattr(c, f), dict(orc.OrcRule._fields_)[f]), (f, getattr(c, f))
    assert all(_fits(w, ctypes.c_uint8) for row in c.weight for w in row)
    r = _struct(c)
    top = SPEED_SQ_TOP
    for s in (0, 1, 2, 30000 ** 2, 42426 ** 2, top):
        want = bool(lo <= math.sqrt(s) <= hi)
        assert (r.speed_sq_min <= s <= r.speed_sq_max) == want, s
    assert (r.min_traffic, r.min_matching_traffic) == (INT32_MAX, INT32_MIN)


@pytest.mark.parametrize("v,want", [(0, 0), (1, 1), (3, 3), (-2, -2), (1.5, 2), (0.2, 1), (-0.5, 0), (2.0, 2),
                                    (math.inf, INT32_MAX), (-math.inf, INT32_MIN), (2 ** 31, INT32_MAX)])
def test_thresholds_decide_like_the_reference_on_every_count(v, want):
    """`count < threshold` (pgtg/environment.py:253, 270) for the counts a tile can hold."""
    c = C.compile_rule(_rule(mt=v, mm=v))
    assert c.min_traffic == c.min_matching_traffic == want
    for n in range(0, 90):
        assert (n < c.min_traffic) == (n < v)


MANEUVERS = [
    {"agent": "south_to_north", "traffic": ["west_to_east"]},
    {"agent": "south_to_north", "traffic": ["west_to_east", "north_to_south"]},  # a second maneuver: weight 2
    {"agent": "stationary", "traffic": ["north_to_south", "north_to_south"]},     # `in`: once per maneuver
    {"agent": "near_goal", "traffic": ["west_to_east"]},
    {"agent": "sideways", "traffic": ["west_to_east"]},                          # unknown agent: ignored
    {"agent": "near_goal", "traffic": ["up_to_down", "all", "car_lane west_to_east right"]},  # unknown routes
]


def test_weight_table_counts_a_route_once_per_naming_maneuver():
    W2E, N2S = C.ROUTES.index("west_to_east"), C.ROUTES.index("north_to_south")
    sn, st, ng = (C.AGENT_DIRECTIONS.index(a) for a in ("south_to_north", "stationary", "near_goal"))
    c = C.compile_rule(_rule(maneuvers=MANEUVERS))
    want = np.zeros((6, 20), int)
    want[sn, W2E], want[sn, N2S], want[st, N2S], want[ng, W2E] = 2, 1, 1, 1
    assert np.array_equal(np.array(c.weight), want)
    assert np.array_equal(np.array([list(row) for row in _struct(c).weight]), want)
    # the reference's own loop over the same rule (evaluate_rule, pgtg/environment.py:259-267)
    for d, agent in enumerate(C.AGENT_DIRECTIONS):
        for k, route in enumerate(C.ROUTES):
            assert want[d, k] == sum(1 for m in MANEUVERS if m["agent"] == agent and route in m["traffic"])


@pytest.mark.parametrize("tile,mask", [("0000", 0), ("1000", 1), ("0100", 2), ("0010", 4), ("0001", 8), ("1010", 5),
                                       ("0101", 10), ("1100", 3), ("0110", 6), ("0011", 12), ("1001", 9),
                                       ("1110", 7), ("0111", 14), ("1011", 13), ("1101", 11), ("1111", 15),
                                       ("11110", -1), ("111", -1), ("1x11", -1), ("", -1), (1111, -1), (None, -1),
                                       ("TrueTrueTrueTrue", -1), ("１１１１", -1)])
def test_every_exit_mask_and_names_that_match_no_tile(tile, mask):
    assert C.compile_rule(_rule(tile=tile)).tile_exits == mask


def test_eight_rules_fit_and_the_ninth_is_refused():
    spec = C.make_spec()
    spec.rules = []
    for k in range(8):
        C.add_rule(spec, _rule(name=f"r{k}"))
    assert len(spec.rules) == 8 == C.MAX_RULES == _abi.MAX_RULES == orc.MAX_RULES
    with pytest.raises(ValueError, match="at most 8"):
        C.add_rule(spec, _rule(name="r8"))
    with pytest.raises(ValueError, match="already exists"):
        C.add_rule(spec, _rule(name="r3"))
    arr = (_abi.PgtgRule * _abi.MAX_RULES)()
    assert _abi.fill_rules(arr, spec.rules) == 8
    with pytest.raises(ValueError):
        _abi.fill_rules(arr, spec.rules + [C.compile_rule(_rule(name="r8"))])
    assert orc.config_from_spec(spec).n_rules == 8


# ---- what the rule fixtures recorded from the reference -------------------------------------------------
RULE_FIXTURES = [n for n in helpers.traj_names() if n.startswith("rules_")]


def test_the_rule_fixtures_are_there():
    assert len(RULE_FIXTURES) == 10


@pytest.mark.parametrize("name", RULE_FIXTURES)
def test_rule_fixture_fired_what_it_is_meant_to_exercise(name):
    d = helpers.load_traj(name)
    meta, trig = d["meta"], d["triggered"].astype(np.int64)
    names = meta["rule_names"]
    assert names == [r.name for r in helpers.spec_for(meta).rules]
    assert np.array_equal(trig != 0, d["braking"] != 0)
    assert not (trig >> len(names)).any()
    count = [int(((trig >> k) & 1).sum()) for k in range(len(names))]
    print(name, dict(zip(names, count)))
    for k in meta["expect_fired"]:
        assert count[k] > 0, f"{names[k]} never fired"
    for k in meta["never_fired"]:
        assert count[k] == 0, f"{names[k]} fired"
    for a, b in meta["fired_without"]:
        assert (((trig >> a) & 1) & ~((trig >> b) & 1)).any(), f"{names[a]} never fired without {names[b]}"
    together = int((np.vectorize(lambda x: bin(x).count("1"))(trig) >= 2).sum())
    if name == "rules_default_s5":  # "1111" and "1110": one tile cannot be both (tests/golden/README.md)
        assert together == 0
    else:
        assert together > 0


def test_eight_slot_fixture_uses_every_bit():
    d = helpers.load_traj("rules_eight_crossing")
    assert np.bitwise_or.reduce(d["triggered"].reshape(-1)) == 0xFF
