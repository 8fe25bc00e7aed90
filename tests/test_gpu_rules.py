"""Traffic-rule braking on the device beyond the two default rules: `braking_query`, `braking_decide`
and the route histogram `move_cars` fills, in `k_env<TR=true>`.

Directed single-tick cases on the fixed maps (agent and cars placed through set_agent / add_car,
mirrored on the oracle), each compared with the oracle (mask byte, velocity, position, reward,
termination, car list) and with `_reference_mask`, the reference's evaluate_rule restated on the rule
dicts themselves (no compile_rule, no weight table), fed with the tile, direction and speed the case
places by construction and the oracle's car list after the tick.  Then seeded random rule sets on random
maps at three launch shapes, applied at creation and through pgtg_set_rules."""
import copy
import math
import os
import warnings

import numpy as np
import pytest

import helpers
from oracle.oracle import OracleEnv
from pgtg_amd import config as cfg

pytestmark = pytest.mark.gpu

R = cfg.ROUTES.index
W2E, E2W, N2S, S2N = R("west_to_east"), R("east_to_west"), R("north_to_south"), R("south_to_north")
NORMAL = cfg.DRIVER_PROFILES.index("normal")
AGENTS4 = cfg.AGENT_DIRECTIONS[:4]
AGENTS6 = cfg.AGENT_DIRECTIONS
SQRT2, SQRT5 = math.sqrt(2.0), math.sqrt(5.0)
CROSSING, STRAIGHT4 = "1x1_crossing_map", "4x1_map"


def _rule(name, tile, vr, mt, mm, maneuvers=()):
    return {"name": name, "tile_type": tile, "velocity_range": list(vr), "min_traffic": mt,
            "min_matching_traffic": mm, "maneuvers": list(maneuvers)}


def _every(agents, routes):
    return [{"agent": a, "traffic": [cfg.ROUTES[r] if isinstance(r, int) else r for r in routes]} for a in agents]


def _spec(map_name, rules, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec = cfg.make_spec(os.path.join(helpers.TESTDATA, map_name) if map_name else None, **kw)
    spec.rules = []
    for r in rules:
        cfg.add_rule(spec, r)
    return spec


def _reference_mask(rules, tile_type, vx, vy, direction, routes_in_tile):
    """TrafficRuleEngine.evaluate_all_rules (pgtg/environment.py:226-283) on plain values."""
    speed = float(np.linalg.norm([vx, vy]))
    mask = 0
    for k, r in enumerate(rules):
        if tile_type != r["tile_type"]:
            continue
        if not (r["velocity_range"][0] <= speed <= r["velocity_range"][1]):
            continue
        if len(routes_in_tile) < r["min_traffic"]:
            continue
        match = 0
        for m in r["maneuvers"]:
            if m["agent"] == direction:
                for route in routes_in_tile:
                    if cfg.ROUTES[route] in m["traffic"]:
                        match += 1
        if match < r["min_matching_traffic"]:
            continue
        mask |= 1 << k
    return mask


class Batch:
    """n envs on the device and their oracles, reset with seed + i."""

    def __init__(self, spec, n, seed, car_capacity=8, **vec_kw):
        from pgtg_amd.vector import PGTGVecEnv
        self.spec, self.n = spec, n
        self.vec = PGTGVecEnv(n, spec=copy.deepcopy(spec), autoreset=False, min_car_capacity=car_capacity, device=0,
                              **vec_kw)
        self.vec.reset(seed=seed)
        self.orcs = [OracleEnv(spec) for _ in range(n)]
        for i, o in enumerate(self.orcs):
            o.reset(seed + i)

    def agent(self, i, x, y, vx, vy):
        self.vec.set_agent(i, x, y, vx, vy)
        self.orcs[i].set_agent(x, y, vx, vy)

    def car(self, i, x, y, route, profile=NORMAL):
        self.vec.add_car(i, x, y, route, profile)
        self.orcs[i].add_car(x, y, route, profile)

    def step(self, actions, where=""):
        """One launch; every env against its oracle.  Returns the mask bytes."""
        import torch
        acts = np.broadcast_to(np.asarray(actions, np.uint8), (self.n,)).copy()
        self.vec.step(torch.as_tensor(acts))
        torch.cuda.synchronize()
        mask, vel, pos = (t.cpu().numpy() for t in (self.vec.braking, self.vec.velocity, self.vec.position))
        rew, term = self.vec.reward.cpu().numpy(), self.vec.terminated.cpu().numpy()
        for i, o in enumerate(self.orcs):
            r = o.step(int(acts[i]))
            tag = f"{where} env{i}"
            assert int(mask[i]) == int(r["braking"]), f"{tag}: mask {int(mask[i]):#04x} vs oracle {int(r['braking']):#04x}"
            assert tuple(vel[i]) == tuple(r["vel"]) and tuple(pos[i]) == tuple(r["pos"]), tag
            assert rew[i] == r["reward"] and bool(term[i]) == r["terminated"], tag
            assert np.array_equal(self.vec.cars(i), o.cars()), f"{tag}: cars"
        return [int(m) for m in mask]

    def close(self):
        self.vec.close()


def _in_tile(cars, tx, ty=0):
    return [int(c[3]) for c in cars if int(c[1]) // 9 == tx and int(c[2]) // 9 == ty]


@pytest.fixture(scope="module")
def lanes():
    """Squares that carry each route, per fixed map: read off the oracle's initial traffic at density 1."""
    out = {}
    for name in (CROSSING, STRAIGHT4):
        o = OracleEnv(_spec(name, [], traffic_density=1.0))
        sq = {}
        for seed in range(4):
            o.reset(seed)
            for c in o.cars():
                sq.setdefault(int(c[3]), set()).add((int(c[1]), int(c[2])))
        out[name] = {k: sorted(v) for k, v in sq.items()}
    for r in (W2E, E2W, N2S, S2N):
        assert len(out[CROSSING][r]) >= 3
    return out


# ---- speed ------------------------------------------------------------------------------------------------
def test_speed_at_the_bounds_is_the_speed_after_the_acceleration():
    """s = 2 against lo = sqrt(2) and hi = sqrt(2), the integers on either side, sqrt(5) from both sides;
    no cars needed.  One env per (start velocity, action)."""
    rules = [_rule("from_sqrt2", "1111", [SQRT2, 10], 0, 0), _rule("to_sqrt2", "1111", [0, SQRT2], 0, 0),
             _rule("only_sqrt2", "1111", [SQRT2, SQRT2], 0, 0), _rule("above_1.5_to_2", "1111", [1.5, 2], 0, 0),
             _rule("to_sqrt5", "1111", [0.1, SQRT5], 0, 0), _rule("from_sqrt5", "1111", [SQRT5, 3], 0, 0),
             _rule("zero", "1111", [0, 0], 0, 0), _rule("to_1", "1111", [0.5, 1], 0, 0)]
    combos = [(vx, vy, a) for vx, vy in ((0, 0), (1, 0), (1, 1), (0, -1), (2, 0), (1, 2)) for a in range(9)]
    b = Batch(_spec(CROSSING, rules), len(combos), 40)
    try:
        for i, (vx, vy, a) in enumerate(combos):
            b.agent(i, 1, 4, vx, vy)
        got = b.step([a for _, _, a in combos], "speed")
        seen = set()
        for i, (vx, vy, a) in enumerate(combos):
            s = (vx + a // 3 - 1) ** 2 + (vy + a % 3 - 1) ** 2  # the integer the bounds are about
            lit = ((s >= 2 and s <= 100) << 0 | (s <= 2) << 1 | (s == 2) << 2 | (s in (3, 4)) << 3
                   | (1 <= s <= 5) << 4 | (5 <= s <= 9) << 5 | (s == 0) << 6 | (s == 1) << 7)
            assert got[i] == lit, (vx, vy, a, s)
            assert lit == _reference_mask(rules, "1111", vx + a // 3 - 1, vy + a % 3 - 1, "west_to_east", [])
            seen.add(s)
        assert {0, 1, 2, 4, 5, 8, 9, 10} <= seen
    finally:
        b.close()


def test_unbounded_and_very_large_upper_bounds(lanes):
    """velocity_range [0, inf] used to reach the device as speed_sq_max = -2^31 and never fire."""
    rules = [_rule("any_speed", "1111", [0, math.inf], 0, 0), _rule("moving", "1111", [0.5, math.inf], 1, 1,
                                                                     _every(AGENTS6, range(20))),
             _rule("to_1e9", "1111", [0, 1e9], 0, 0), _rule("to_46341", "1111", [1, 46341], 0, 0),
             _rule("to_46340", "1111", [1, 46340], 0, 0), _rule("from_46341", "1111", [46341, math.inf], 0, 0),
             _rule("from_inf", "1111", [math.inf, math.inf], 0, 0), _rule("to_65", "1111", [64.5, 65], 0, 0)]
    vels = [(0, 0), (1, 0), (0, 3), (64, 0), (-65, 0), (64, 64), (300, -200), (0, 0)]
    b = Batch(_spec(CROSSING, rules), 4 * len(vels), 41)
    try:
        x, y = lanes[CROSSING][N2S][0]
        for i in range(b.n):
            b.agent(i, 1, 4, *vels[i % len(vels)])
            b.car(i, x, y, N2S)
        got = b.step(4, "unbounded")
        for i in range(b.n):
            vx, vy = vels[i % len(vels)]
            s = vx * vx + vy * vy
            lit = 1 | (s > 0) << 1 | 1 << 2 | (s >= 1) << 3 | (s >= 1) << 4 | (s == 65 * 65) << 7
            assert got[i] == lit, (vx, vy)
            assert lit == _reference_mask(rules, "1111", vx, vy, "west_to_east", [N2S])
    finally:
        b.close()


# ---- thresholds and weights ----------------------------------------------------------------------------------
def test_thresholds_at_equality_and_one_below_with_weights_one_and_two(lanes):
    """Env i holds i % 5 cars of the matching route and i // 5 % 3 others: n_in and the weighted match
    meet every threshold from below, at equality and from above."""
    one = _every(["west_to_east"], [N2S])
    two = one + _every(["west_to_east"], [N2S, S2N])  # north_to_south named by two maneuvers
    rules = [_rule("n2", "1111", [0, 10], 2, 0), _rule("n3", "1111", [0, 10], 3, 0),
             _rule("m1", "1111", [0, 10], 0, 1, one), _rule("m2", "1111", [0, 10], 0, 2, one),
             _rule("m3", "1111", [0, 10], 0, 3, one), _rule("w2_m2", "1111", [0, 10], 0, 2, two),
             _rule("w2_m4", "1111", [0, 10], 0, 4, two), _rule("w2_m5", "1111", [0, 10], 5, 5, two)]
    b = Batch(_spec(CROSSING, rules), 30, 42)
    try:
        for i in range(b.n):
            b.agent(i, 1, 4, 0, 0)
            for k in range(i % 5):
                b.car(i, *lanes[CROSSING][N2S][k % 3], N2S)  # (cars may share a square)
            for k in range(i // 5 % 3):
                b.car(i, *lanes[CROSSING][E2W][k], E2W)
        got = b.step(4, "thresholds")
        seen = set()
        for i, o in enumerate(b.orcs):
            routes = _in_tile(o.cars(), 0)  # a 1x1 map: every car, respawned or not, is in the tile
            assert len(routes) == i % 5 + i // 5 % 3
            assert got[i] == _reference_mask(rules, "1111", 0, 0, "west_to_east", routes), routes
            seen.add((len(routes), routes.count(N2S)))
        # literals where no car can have left the list: none at all; two matching cars that did not respawn
        assert got[0] == 0
        for need in ((1, 1), (2, 2), (3, 3), (2, 1), (3, 2), (4, 2), (5, 3)):  # below, at and above each threshold
            assert need in seen, need
    finally:
        b.close()


def test_mask_bits_all_eight_and_the_last_alone():
    full = [_rule(f"r{k}", "1111", [0, 10], 0, 0) for k in range(8)]
    last = [_rule(f"r{k}", "0101" if k < 7 else "1111", [0, 10], 0, 0) for k in range(8)]
    odd = [_rule(f"r{k}", "1111" if k % 2 else "1110", [0, 10], 0, 0) for k in range(8)]
    for rules, lit in ((full, 0xFF), (last, 0x80), (odd, 0xAA)):
        b = Batch(_spec(CROSSING, rules), 24, 43)
        try:
            for i in range(b.n):
                b.agent(i, 1, 3 + i % 3, 0, 0)
            assert b.step(4, f"bits {lit:#x}") == [lit] * b.n
            assert b.vec.step_kernel().split(" + ")[0] == "pgtg::k_env<true, false>"
        finally:
            b.close()


def test_directions_4_and_5_without_a_goal_square_in_compass_reach(lanes):
    """The goal squares are (8, 3..5): from x >= 4 none is in compass reach, so the direction is
    "stationary" at speed 0 and "near_goal" above; from x = 3 it is "west_to_east"."""
    rules = [_rule("w2e", "1111", [0, 10], 1, 1, _every(["west_to_east"], [N2S])),
             _rule("stationary", "1111", [0, 10], 1, 1, _every(["stationary"], [N2S])),
             _rule("near_goal", "1111", [0, 10], 1, 1, _every(["near_goal"], [N2S])),
             _rule("stationary_moving", "1111", [0.1, 10], 0, 1, _every(["stationary"], [N2S])),
             _rule("near_goal_still", "1111", [0, 0], 0, 1, _every(["near_goal"], [N2S])),
             _rule("both_twice", "1111", [0, 10], 0, 2, _every(["stationary", "near_goal", "stationary", "near_goal"], [N2S]))]
    cases = [(3, 4, 0, 0, 4, 0b000001), (3, 4, 0, 0, 7, 0b000001), (4, 4, 0, 0, 4, 0b100010), (4, 4, 0, 0, 7, 0b100100),
             (5, 3, 0, 0, 4, 0b100010), (5, 5, 1, 0, 1, 0b100010), (6, 4, 0, 0, 5, 0b100100), (4, 4, 1, 1, 4, 0b100100),
             (7, 4, 0, 1, 4, 0b100100), (2, 4, 1, 0, 4, 0b000001)]
    b = Batch(_spec(CROSSING, rules), 3 * len(cases), 44)
    try:
        for i in range(b.n):
            x, y, vx, vy, _, _ = cases[i % len(cases)]
            b.agent(i, x, y, vx, vy)
            b.car(i, *lanes[CROSSING][N2S][0], N2S)
        got = b.step([cases[i % len(cases)][4] for i in range(b.n)], "directions")
        for i in range(b.n):
            assert got[i] == cases[i % len(cases)][5], cases[i % len(cases)]
    finally:
        b.close()


# ---- which cars the histogram counts ---------------------------------------------------------------------------
def _count_rules(tile):
    ew = _every(AGENTS6, [W2E, E2W])
    return [_rule("any", tile, [0, 10], 1, 0), _rule("two", tile, [0, 10], 2, 0), _rule("three", tile, [0, 10], 3, 0),
            _rule("w2e_or_e2w", tile, [0, 10], 0, 1, ew), _rule("two_ew", tile, [0, 10], 0, 2, ew),
            _rule("w2e", tile, [0, 10], 0, 1, _every(AGENTS6, [W2E])), _rule("e2w", tile, [0, 10], 0, 1, _every(AGENTS6, [E2W])),
            _rule("four", tile, [0, 10], 4, 4, ew + ew)]


def test_cars_entering_leaving_and_respawning_into_the_agents_tile(lanes):
    """4x1 strip, the agent standing in tile 1 (envs 0..23) or in tile 3, whose east edge despawns
    west_to_east cars (envs 24..47).  Cars sit on the last square before and the last square inside the
    tile; the draws decide which of them move.  What counts is where they are after the move."""
    rules = _count_rules("0101")
    sq = lanes[STRAIGHT4]
    y_e = next(y for x, y in sq[W2E] if x == 8)   # the eastbound lane's row
    y_w = next(y for x, y in sq[E2W] if x == 8)
    b = Batch(_spec(STRAIGHT4, rules), 48, 45)
    try:
        before = []
        for i in range(b.n):
            if i < 24:
                b.agent(i, 13, y_e, 0, 0)
                b.car(i, 8, y_e, W2E)    # may enter tile 1
                b.car(i, 17, y_e, W2E)   # may leave it
                b.car(i, 18, y_w, E2W)   # may enter from the east
                if i % 2:
                    b.car(i, 9, y_w, E2W)  # may leave to the west
            else:
                b.agent(i, 31, y_e, 0, 0)
                b.car(i, 35, y_e, W2E)   # leaves the map when it moves: a respawn on some spawner
                b.car(i, 26, y_e, W2E)
                if i % 2:
                    b.car(i, 0, y_w, E2W)  # leaves the map in tile 0
            before.append(b.orcs[i].cars())
        got = b.step(4, "entering")
        entered = left = respawned_in = respawned_out = 0
        for i, o in enumerate(b.orcs):
            tx = 1 if i < 24 else 3
            after = o.cars()
            assert got[i] == _reference_mask(rules, "0101", 0, 0, "west_to_east", _in_tile(after, tx)), i
            was = {int(c[0]): int(c[1]) // 9 for c in before[i]}
            for c in after:
                cid, t = int(c[0]), int(c[1]) // 9
                if cid in was:
                    entered += was[cid] != tx and t == tx
                    left += was[cid] == tx and t != tx
                else:
                    respawned_in += t == tx
                    respawned_out += t != tx
        # every kind happened in this batch (the draws are the seeds'; the oracle says which)
        assert entered > 0 and left > 0 and respawned_in > 0 and respawned_out > 0, (entered, left, respawned_in, respawned_out)
    finally:
        b.close()


def test_counts_through_the_fresh_block_unpacked_slots_and_the_packing_pass():
    """Dense traffic on the 4x1 strip for a dozen ticks, the agent put back into tile i % 4 before every
    tick.  The first tick reads the cars from the reset's staging block; later ticks leave empty slots
    (unpacked path) until some env holds more than four, when the wave packs.  Thresholds sit around
    the counts a tile holds, so one car miscounted flips a bit."""
    rules = [_rule(f"n{k}", "0101", [0, 10], k, 0) for k in (3, 5, 7, 9)] + \
            [_rule(f"e{k}", "0101", [0, 10], 0, k, _every(AGENTS6, [W2E])) for k in (2, 4)] + \
            [_rule(f"w{k}", "0101", [0, 10], 0, k, _every(AGENTS6, [E2W]) * 2) for k in (4, 8)]
    spec = _spec(STRAIGHT4, rules, traffic_density=0.6, ignore_traffic_collisions=True)
    b = Batch(spec, 32, 46, car_capacity=0)
    try:
        kinds, masks = set(), set()
        for t in range(14):
            st = [b.vec.env_state(i) for i in range(b.n)]
            holes = [s["car_tail"] - s["n_cars"] for s in st]
            kind = "fresh" if t == 0 else "pack" if max(holes) > 4 else "holes" if max(holes) > 0 else "dense"
            for i in range(b.n):
                b.agent(i, 9 * (i % 4) + 4, 4, 0, 0)
            got = b.step(4, f"tick {t} ({kind})")
            for i, o in enumerate(b.orcs):
                direction = "west_to_east" if i % 4 < 3 else "near_goal"  # tile 3: the goal squares are 4 away
                want = _reference_mask(rules, "0101", 0, 0, direction, _in_tile(o.cars(), i % 4))
                assert got[i] == want, (t, kind, i)
                masks.add(got[i])
            kinds.add(kind)
        assert {"fresh", "holes", "pack"} <= kinds, kinds
        assert len(masks) >= 8, masks  # the counts straddle the thresholds
    finally:
        b.close()


def test_every_tile_type_of_the_fixed_maps_and_dead_ends(lanes):
    """The agent set into each tile of map_with_all_directions and map_with_all_deadends in turn, one
    rule per tile type the map holds (at most eight per handle), dense traffic from the reset."""
    import json
    for name in ("map_with_all_directions", "map_with_all_deadends"):
        with open(os.path.join(helpers.TESTDATA, name + ".json")) as f:
            plan = json.load(f)
        types = ["".join(str(int(e)) for e in t["exits"]) for row in plan["map"] for t in row]
        kinds = sorted(set(types) - {"0000"})
        for part in (kinds[:8], kinds[8:]):
            if not part:
                continue
            rules = [_rule(f"in_{t}", t, [0, 10], k % 2, 0) for k, t in enumerate(part)]
            spec = _spec(name, rules, traffic_density=0.7, ignore_traffic_collisions=True)
            w, h = plan["width"], plan["height"]
            b = Batch(spec, w * h, 47, car_capacity=0)
            try:
                for i in range(b.n):
                    b.agent(i, 9 * (i % w) + 4, 9 * (i // w) + 4, 0, 0)
                got = b.step(4, name)
                fired = 0
                for i, o in enumerate(b.orcs):
                    n_in = len(_in_tile(o.cars(), i % w, i // w))
                    lit = sum(1 << k for k, t in enumerate(part) if t == types[i] and n_in >= k % 2)
                    assert got[i] == lit, (name, i, types[i], n_in)
                    fired |= got[i]
                for k in range(0, len(part), 2):  # (the rules that need no car fire wherever their tile is)
                    assert fired >> k & 1, (name, part[k])
                assert bin(fired).count("1") > len(part) // 2, (name, part, bin(fired))
            finally:
                b.close()


# ---- rule-set fuzz -----------------------------------------------------------------------------------------
TILES_COMMON = ["0101", "1001", "1101", "0111", "1011", "1111", "1010", "0011", "1100", "0110", "1110"]
TILES_RARE = ["0001", "0010", "0100", "1000", "0000", "11110", "1x11", 1111]
LOS = [0, 0, 0, 0.1, 0.5, 1, SQRT2, 1.5, 2, SQRT5]
HIS = [0, 1, SQRT2, 1.5, 2, SQRT5, 3, 10, 10, 1e9, math.inf]


def random_rules(rng, n):
    rules = []
    for k in range(n):
        tile = TILES_COMMON[rng.integers(len(TILES_COMMON))] if rng.random() < 0.85 else TILES_RARE[rng.integers(len(TILES_RARE))]
        lo, hi = LOS[rng.integers(len(LOS))], HIS[rng.integers(len(HIS))]
        if rng.random() < 0.8 and lo > hi:
            lo, hi = hi, lo
        mans = []
        for _ in range(int(rng.integers(1, 7))):
            agent = AGENTS6[rng.integers(6)] if rng.random() < 0.9 else "sideways"
            routes = [cfg.ROUTES[r] for r in rng.integers(0, 20, int(rng.integers(1, 13)))]  # (repeats allowed)
            if rng.random() < 0.1:
                routes.append("up_to_down")
            mans.append({"agent": agent, "traffic": routes})
        if rng.random() < 0.5:  # every direction, so that a rule does not hinge on where the goal lies
            mans += _every(AGENTS6, rng.integers(0, 20, int(rng.integers(2, 9))).tolist())
        rules.append(_rule(f"fuzz{k}", tile, [lo, hi], int(rng.choice([0, 1, 1, 2, 3])), int(rng.choice([0, 1, 1, 2, 3])), mans))
    return rules


# name: (kwargs, envs, compared envs, seed, kernel, rule-set seeds); four rule sets per shape, a dozen in all: the
# first two of eight rules, the others of 1 to 8.  The set seeds were chosen with the oracle alone so that every
# slot fires at every shape.
FUZZ = {
    "small_workgroup_64": (dict(random_map_width=5, random_map_height=5, traffic_density=0.5,
                                random_map_start_position="random", random_map_goal_position="random"),
                           64, 64, 1000, "pgtg::k_env<true, false>", (24, 15, 31, 32)),
    "multi_workgroup_3000": (dict(random_map_width=4, random_map_height=4, traffic_density=0.8,
                                  random_map_start_position="random", random_map_goal_position="random"),
                             3000, 32, 2000, "pgtg::k_env<true, false>", (19, 21, 33, 34)),
    "big_map_9x9": (dict(random_map_width=9, random_map_height=9, traffic_density=0.3,
                         random_map_start_position="random", random_map_goal_position="random"),
                    64, 32, 3000, "pgtg::k_env<true, true>", (7, 5, 35, 36)),
}
FUZZ_STEPS = 25


def fuzz_rule_set(set_seed, k):
    rng = np.random.default_rng(set_seed)
    return random_rules(rng, 8 if k < 2 else int(rng.integers(1, 9)))


@pytest.mark.parametrize("way", ["at_creation", "set_rules"])
@pytest.mark.parametrize("shape", list(FUZZ))
def test_random_rule_sets(shape, way):
    from pgtg_amd.vector import PGTGVecEnv
    kw, n, n_cmp, seed, kernel, set_seeds = FUZZ[shape]
    envs = sorted(set(np.linspace(0, n - 1, n_cmp).astype(int).tolist()))
    slots, multi = [0] * 8, 0
    for k, set_seed in enumerate(set_seeds):
        rules = fuzz_rule_set(set_seed, k)
        spec = _spec(None, rules, **kw)
        tag = f"{shape} set {set_seed} {way}"
        stats, orcs = {}, {}
        rng = np.random.default_rng(set_seed)
        if way == "at_creation":
            vec = PGTGVecEnv(n, spec=copy.deepcopy(spec), device=0)
        else:  # a decoy in slot 0 and the rules added one by one after the reset; removing the decoy shifts every slot
            bare = _spec(None, [_rule("decoy", "1111", [0, math.inf], 0, 0)], **kw)
            vec = PGTGVecEnv(n, spec=bare, device=0)
        try:
            vec.reset(seed=seed)
            if way == "set_rules":
                for r in rules[:7]:
                    vec.add_traffic_rule(r)
                assert vec.remove_traffic_rule("decoy")
                for r in rules[7:]:
                    vec.add_traffic_rule(r)
                assert vec.rule_names() == [r["name"] for r in rules]
            assert vec.step_kernel().split(" + ")[0] == kernel  # (resets with traffic add k_traffic)
            helpers.vec_vs_oracle(vec, spec, n, 10, seed, rng, tag, envs, stats, orcs)
            if way == "set_rules":  # mid-episode: the same rules taken out and put back (tables rewritten)
                for r in rules:
                    assert vec.remove_traffic_rule(r["name"])
                for r in rules:
                    vec.add_traffic_rule(r)
            helpers.vec_vs_oracle(vec, spec, n, FUZZ_STEPS - 10, seed, rng, tag, envs, stats, orcs)
        finally:
            vec.close()
        print(tag, len(rules), "rules, fired per slot", stats["rule"], "steps with two or more", stats["multi"])
        slots = [a + b for a, b in zip(slots, stats["rule"])]
        multi += stats["multi"]
    assert all(s > 0 for s in slots), f"{shape}: a rule slot never fired: {slots}"
    assert multi > 0, f"{shape}: no step fired two rules"
