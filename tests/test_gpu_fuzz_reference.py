"""The HIP step kernels against the reference on the fuzz distributions, from recorded data alone
(tests/golden/fuzz, tools/gen_golden.py FUZZ_CASES; tests/test_oracle_fuzz.py holds the CPU oracle to
the same files).

A fixture has 3 or 4 envs.  They are planted in a larger batch (helpers.replay_vec n_batch, at): the
batch is reset with one seed per env, the fixture's at the planted indices and filler seeds elsewhere,
so the auto-reset of a planted env has to follow the env's own seed, not its index.  The two shapes
are the smallest that reach a full wave and a partial last workgroup on both sides of the 64- and
256-env boundaries.  Every fixture runs under the step kernel its configuration selects; where the
configuration admits the map queue (no traffic, no lane or spawner channels; pgtg_env.hip
choose_launch) it also runs under tune queue_mode 1 (k_envq) and 2 (k_envb).  The last test asserts
that the set stepped every step-kernel instance of tests/test_gpu_create_paths.py ROWS."""
import pytest

import helpers
from test_gpu_create_paths import ROWS

pytestmark = pytest.mark.gpu

SUB = "fuzz"
NAMES = helpers.traj_names(SUB)
SHAPES = [(64, (0, 31, 63)), (300, (0, 63, 64, 255, 256, 299))]
MODES = {"default": None, "envq": dict(queue_mode=1), "envb": dict(queue_mode=2)}
INSTANCES = sorted({k.split(" + ")[0] for row in ROWS.values() for k in row[5:8:2]})


def admits_queue(meta: dict) -> bool:
    feats = meta["kwargs"]["features_to_include_in_observation"]
    return not helpers.has_traffic(meta) and not any(f == "car_spawner" or f.startswith("car_lane") for f in feats)


def _shape(name: str, mode: str, n_envs: int):
    """Cycle the two shapes over the cases (and over the forced kernels of a case); the planted indices
    of the batch of 300 are taken in turn as well.  A fixture of 4 envs goes to the batch of 300, which
    has room for all of them."""
    n = NAMES.index(name) + list(MODES).index(mode)
    n_batch, at = SHAPES[1] if n_envs > len(SHAPES[0][1]) else SHAPES[n % 2]
    return n_batch, sorted(at[(n // 2 + j) % len(at)] for j in range(n_envs))


RUNS = [(name, mode) for name in NAMES for mode in MODES
        if mode == "default" or admits_queue(helpers.load_traj(name, SUB)["meta"])]
_done: dict = {}


def _run(name: str, mode: str):
    """(mismatches, info) of one replay, run once per session"""
    if (name, mode) not in _done:
        d = helpers.load_traj(name, SUB)
        n_batch, at = _shape(name, mode, d["meta"]["N"])
        info: dict = {}
        bad = helpers.replay_vec(d, n_batch=n_batch, at=at, tune=MODES[mode], info=info)
        print(f"{name} {mode}: n={n_batch} at={at} {info.get('step_kernel')}")
        _done[(name, mode)] = (bad, info)
    return _done[(name, mode)]


def test_shapes_and_instances():
    """the 64-env shape needs 3 envs at most; both shapes and every planted index are used"""
    used = {(n, b) for name, mode in RUNS for n, at in [_shape(name, mode, helpers.load_traj(name, SUB)["meta"]["N"])]
            for b in at}
    assert used >= {(n, b) for n, at in SHAPES for b in at}
    assert len(INSTANCES) == 8 and all(k.startswith("pgtg::k_env") for k in INSTANCES), INSTANCES


@pytest.mark.parametrize("name,mode", RUNS)
def test_fuzz_fixture_planted_in_a_larger_batch(name, mode):
    bad, info = _run(name, mode)
    assert not bad, (info.get("step_kernel"), bad[:10])
    assert info["errors"] == 0
    if mode != "default" and info["step_kernel"].startswith("pgtg::k_envq"):
        assert MODES[mode]["queue_mode"] == 1
    if mode != "default" and info["step_kernel"].startswith("pgtg::k_envb"):
        assert MODES[mode]["queue_mode"] == 2


def test_every_step_kernel_instance_was_stepped_by_a_fuzz_fixture():
    runs = {k: 0 for k in INSTANCES}
    for name, mode in RUNS:
        bad, info = _run(name, mode)  # (run already when the whole file runs)
        kernel = info["step_kernel"].split(" + ")[0]
        assert kernel in runs, kernel
        runs[kernel] += 1
    print({k: n for k, n in runs.items()})
    assert all(n >= 1 for n in runs.values()), runs
