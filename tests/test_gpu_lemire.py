"""Lemire rejections on the device: the directed seeds of tests/golden/lemire_rejections.json
(tools/find_rejection_seeds.py; checked on the CPU by tests/test_lemire_fixture.py) through every
launch shape of k_traffic.

A reset whose choice of car squares rejects a draw makes choice_draws_group re-evaluate every later
draw one half further on; a reset whose initial route draw has left < n makes cars_group hand its
cars to cars_serial.  Neither happens in a small batch of consecutive seeds (a few resets in 10^5
meet one), so here the fixture's seeds are cycled over the whole batch: every group position of
every wave holds each of them, at 16, 12, 8, 4, 3 and 2 lanes per env and in the one-env rounds, and
every env is compared with the oracle of its seed: observation and full car list after the reset,
and again after each of four steps (the car stream handed on must be right, not only the cars).

k_traffic reports its launch shape nowhere (the ABI is left as it is), so the shape of every case
is derived here by the library's own rule (traffic_shape below: the envs a wave's LDS holds, kt_cap,
from the per-env scratch of the configuration and sizeof(Tables), which the probe library reports
from the same header; then the kernel's rounds and envs per wave), and each case asserts the lanes
per env it is named for.  The LDS does not admit every group size in every configuration: at the
default two workgroups per CU a wave of the 5x5 density-0.5 maps holds 7 envs, so the small groups
run with tune_kt_wpc = 1 (17 envs per wave there), and 2 lanes per env (22 or more envs per wave)
exist only on the 2x9 maps, 4 and 3 lanes not at density 1.0 (9 envs per wave).  REACHABLE lists
what runs; the rows of test_gpu_traffic_groups.py also run as they are, under the shape the rule
gives them (several rounds of 9 to 16 lanes for the rows above 256 envs)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers
from oracle.oracle import OracleEnv
from test_lemire_fixture import entries, load_fixture, spec_of

pytestmark = pytest.mark.gpu
ROOT = helpers.ROOT

DOC = load_fixture()
TABLES_BYTES = 13200  # sizeof(pgtg::Tables); checked against the probe library's value in every case
LDS_BYTES = 160 * 1024
GRID = 8  # workgroups of four waves: 32 waves

# the rows of test_gpu_traffic_groups.py: (envs, grid, cap)
ROWS = {
    "g16_e3": (96, 8, None),
    "g12_e5": (160, 8, None),
    "g8_e8": (256, 8, None),
    "quads_e16": (512, 8, None),
    "triples_e20": (640, 8, None),
    "pairs_e25": (800, 8, None),
    "rounds_cap1": (96, 4, 1),
}
ACTIONS = (4, 4, 4, 4)  # fixed: idle (on the two-tile-wide maps an accelerating agent is in a wall at once)


def reset_seeds(name: str) -> list[int]:
    """the configuration's reset entries: Floyd, shuffle and initial-route hits, in seed order"""
    return sorted({e["seed"] for e in entries(DOC, name) if e["step"] == 0})


def kt_cap(name: str, wpc: int) -> int:
    """envs per wave that k_traffic's LDS holds (pgtg_create: per-env tile plan + reset scratch, four
    waves per workgroup, wpc workgroups per CU and the constant tables in each)"""
    kw = DOC["configs"][name]["kwargs"]
    tw, th = kw["random_map_width"], kw["random_map_height"]
    nt, W = tw * th, 9 * tw
    cap = max(1, int(nt * 32 * kw["traffic_density"]))
    jj = (2 * cap + 3) // 4 * 4
    pre = 2 * jj + 4 * nt
    rs = max((pre + 2 * (W + 1) + 3) // 4 * 4, jj + 16 * nt)
    if th <= 7:
        rs += 8 * W
    per_env = 4 * (((nt + 1) // 2 | 1) + (rs // 4 | 1))
    while True:
        c = 32
        while c > 1 and wpc * (4 * c * per_env + TABLES_BYTES + 256) > LDS_BYTES:
            c -= 1
        if wpc == 1 or wpc * (4 * c * per_env + TABLES_BYTES + 256) <= LDS_BYTES:
            return c
        wpc -= 1


def traffic_shape(name: str, n: int, grid: int, tune_cap=None, wpc: int = 2):
    """(rounds, envs per wave and round, lanes per env) of k_traffic for a work list of n envs"""
    cap = kt_cap(name, wpc)
    if tune_cap is not None and 1 <= tune_cap <= cap:
        cap = tune_cap
    waves = 4 * grid
    rounds = -(-n // (waves * cap))
    e = -(-n // (waves * rounds))
    assert e <= cap
    return rounds, e, min(16, 64 // e)


# lanes per env -> envs per wave that give them (the fewest: the largest stretches per lane)
E_FOR_LANES = {16: 3, 12: 5, 8: 8, 4: 16, 3: 17, 2: 22}
# (configuration, lanes) that the LDS admits at one workgroup per CU
REACHABLE = [(name, g) for name in sorted(DOC["configs"]) for g, e in E_FOR_LANES.items() if kt_cap(name, 1) >= e]


def check_tables_bytes():
    import rng_probe_build
    assert rng_probe_build.lib().rng_probe_tables_bytes() == TABLES_BYTES  # traffic_shape's premise


class Oracles:
    """one OracleEnv per distinct seed, stepped alongside the batch (auto-reset like it; `done`: the
    seeds whose first episode ended)"""

    def __init__(self, spec, seeds):
        self.envs = {s: OracleEnv(spec) for s in seeds}
        self.res = {s: o.reset(s) for s, o in self.envs.items()}
        self.done = set()

    def step(self, action: int):
        for s, o in self.envs.items():
            self.res[s] = o.step(action)
            if self.res[s]["terminated"]:  # (a car on the idle agent's square: common at these densities)
                self.done.add(s)
                self.res[s] = o.reset(None)  # the batch resets in the same step, unseeded: follow it

    def compare(self, env, seeds_of_env, tag: str, idx=None):
        m = env.obs_map.cpu().numpy()
        cars = {s: o.cars() for s, o in self.envs.items()}
        for i in (range(len(seeds_of_env)) if idx is None else idx):
            s = seeds_of_env[i]
            assert np.array_equal(m[i], self.res[s]["obs"]), f"{tag} env {i} seed {s}: observation"
            assert np.array_equal(env.cars(i), cars[s]), f"{tag} env {i} seed {s}: cars"


def run_batch(name: str, n: int, e: int, tune: dict, steps=ACTIONS):
    from pgtg_amd.vector import PGTGVecEnv
    spec = spec_of(DOC, name)
    hits = reset_seeds(name)
    assert 9 <= len(hits) <= n // e, hits
    # env j of the work list is slot j % e of wave-round j // e (when the list holds the envs in index
    # order): slot q sees the seeds q, q + 1, ... in turn, so every seed meets every group position of
    # a wave; every env is compared whatever its place
    seeds = [hits[(j % e + j // e) % len(hits)] for j in range(n)]
    env = PGTGVecEnv(n, spec=spec, device=0, tune=tune)
    try:
        env.reset(seed=seeds)
        torch.cuda.synchronize()
        assert env.error_count()[0] == 0
        orc = Oracles(spec, hits)
        orc.compare(env, seeds, f"{name} reset")
        for t, a in enumerate(steps):
            env.step_actions(torch.full((n,), a, dtype=torch.uint8, device="cuda"))
            torch.cuda.synchronize()
            orc.step(a)
            orc.compare(env, seeds, f"{name} t{t}")
    finally:
        env.close()


def test_reachable_group_sizes():
    """what the LDS rule admits, spelled out: a change of the scratch layout shows here, not as a
    silently different shape"""
    assert {name: kt_cap(name, 2) for name in DOC["configs"]} == {"cfg3": 7, "dense5x5": 4, "tall_map": 13, "wide_map": 8}
    assert {name: kt_cap(name, 1) for name in DOC["configs"]} == {"cfg3": 17, "dense5x5": 9, "tall_map": 28, "wide_map": 18}
    assert sorted(g for name, g in REACHABLE if name == "cfg3") == [3, 4, 8, 12, 16]
    assert sorted(g for name, g in REACHABLE if name == "tall_map") == [2, 3, 4, 8, 12, 16]


@pytest.mark.parametrize("name,lanes", REACHABLE)
def test_rejection_seeds_in_every_group_size(name, lanes):
    """one round of full waves with exactly the named lanes per env"""
    check_tables_bytes()
    e = E_FOR_LANES[lanes]
    n = 4 * GRID * e
    assert traffic_shape(name, n, GRID, wpc=1) == (1, e, lanes)
    run_batch(name, n, e, {"kt_grid": GRID, "kt_wpc": 1})


@pytest.mark.parametrize("name", sorted(DOC["configs"]))
@pytest.mark.parametrize("row", list(ROWS))
def test_rejection_seeds_in_the_traffic_group_rows(row, name):
    """the rows of test_gpu_traffic_groups.py as they are (default workgroups per CU): rounds and
    groups as the rule gives them; rounds_cap1 is one env per wave in several rounds"""
    check_tables_bytes()
    n, grid, cap = ROWS[row]
    rounds, e, lanes = traffic_shape(name, n, grid, cap)
    if row == "rounds_cap1":
        assert (rounds, e, lanes) == (6, 1, 16)
    run_batch(name, n, e, {"kt_grid": grid} if cap is None else {"kt_grid": grid, "kt_cap": cap})


@pytest.mark.parametrize("name,lanes", [(n_, g) for n_, g in REACHABLE if g in (16, 4, 2)])
def test_rejection_seeds_on_the_serial_loop(name, lanes):
    """tune_kt_serial: the one-lane car loop (its own ahead_draw rejection loop) after the group's choice"""
    check_tables_bytes()
    e = E_FOR_LANES[lanes]
    n = 4 * GRID * e
    assert traffic_shape(name, n, GRID, wpc=1) == (1, e, lanes)
    run_batch(name, n, e, {"kt_grid": GRID, "kt_wpc": 1, "kt_serial": 1})


@pytest.mark.parametrize("name", sorted(DOC["configs"]))
def test_rejection_seeds_in_a_masked_reset(name):
    """The steady-state shape: a stepped 4 096-env batch of which five envs are reset (a work list of
    five: one env per wave, 16 lanes each) with the rejection seeds."""
    from pgtg_amd.vector import PGTGVecEnv
    spec = spec_of(DOC, name)
    hits = reset_seeds(name)
    n = 4096
    where = [0, 1, 2047, 4094, 4095]
    env = PGTGVecEnv(n, spec=spec, device=0)
    try:
        env.reset(seed=3)
        idle = torch.full((n,), 4, dtype=torch.uint8, device="cuda")
        for _ in range(3):
            env.step_actions(idle)
        for rnd in range(-(-len(hits) // len(where))):  # every reset seed once, five at a time
            part = [hits[(rnd * len(where) + j) % len(hits)] for j in range(len(where))]
            seeds = [0] * n
            mask = torch.zeros(n, dtype=torch.uint8)
            for i, s in zip(where, part):
                seeds[i] = s
                mask[i] = 1
            env.reset(seed=seeds, mask=mask)
            torch.cuda.synchronize()
            assert env.error_count()[0] == 0
            orc = Oracles(spec, sorted(set(part)))
            orc.compare(env, seeds, f"{name} masked reset {rnd}", idx=where)
            for t, a in enumerate(ACTIONS):
                env.step_actions(torch.full((n,), a, dtype=torch.uint8, device="cuda"))
                torch.cuda.synchronize()
                orc.step(a)
                orc.compare(env, seeds, f"{name} masked reset {rnd} t{t}", idx=where)
    finally:
        env.close()


def car_pass_entries():
    return [e for e in entries(DOC) if e["step"] > 0 and "car_pass" in e["tags"]]


def run_car_pass(tune: dict) -> int:
    """the recorded (seed, step) pairs with a (possible) rejection in the car pass: idle to the step,
    car lists against the oracle at that step and the next three; returns the entries run"""
    from pgtg_amd.vector import PGTGVecEnv
    done = 0
    for name in DOC["configs"]:
        es = [e for e in car_pass_entries() if e["config"] == name]
        if not es:
            continue
        spec = spec_of(DOC, name)
        n = 256 + 3  # more than one workgroup at either size, the last one partial
        seeds = [es[i % len(es)]["seed"] for i in range(n)]
        last = max(e["step"] for e in es) + 3
        env = PGTGVecEnv(n, spec=spec, device=0, tune=tune)
        try:
            if "envs_per_block" in tune:
                assert env.launch_info()[0] == tune["envs_per_block"]
            assert "k_env<true" in env.step_kernel()
            env.reset(seed=seeds)
            orc = Oracles(spec, sorted({e["seed"] for e in es}))
            idle = torch.full((n,), 4, dtype=torch.uint8, device="cuda")
            for t in range(1, last + 1):
                env.step_actions(idle)
                orc.step(4)
                if any(e["step"] <= t <= e["step"] + 3 for e in es):
                    torch.cuda.synchronize()
                    idx = [i for i in range(n) if any(e["seed"] == seeds[i] and e["step"] <= t <= e["step"] + 3 for e in es)]
                    orc.compare(env, seeds, f"{name} car pass t{t}", idx=idx)
            for e in es:
                assert e["seed"] not in orc.done, e  # the fixture's episodes outlive their entries
            done += len(es)
        finally:
            env.close()
    return done


# A site that the fixture's scan did not reach (its 'not_reached' list) has no case: omitted, not faked.
if car_pass_entries():

    @pytest.mark.parametrize("epb", [256, 128])
    def test_car_pass_rejections(epb):
        assert run_car_pass({"envs_per_block": epb}) == len(car_pass_entries())

    def test_car_pass_rejections_with_saturating_counters():
        """the same through the occsat build (one library per process, so in a child)"""
        from pgtg_amd.build import build, variant_path
        build(variant="occsat")
        code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
                "import test_gpu_lemire as T\n"
                "print('ran', T.run_car_pass({'envs_per_block': 256}))\n"
                "print('occsat loaded', any('libpgtg_hip_occsat.so' in l for l in open('/proc/self/maps')), "
                "any('libpgtg_hip.so' in l for l in open('/proc/self/maps')))\n")
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PGTG_LIB=variant_path("occsat")),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert f"ran {len(car_pass_entries())}\n" in p.stdout, p.stdout[-2000:]
        assert "occsat loaded True False" in p.stdout, p.stdout[-2000:]  # the variant, and not the product library
