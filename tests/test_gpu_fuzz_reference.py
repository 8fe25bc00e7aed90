"""The HIP step kernels against the reference on the fuzz distributions, from recorded data alone
(tests/golden/fuzz, tools/gen_golden.py FUZZ_CASES; tests/test_oracle_fuzz.py holds the CPU oracle to
the same files).

A fixture has 3 or 4 envs.  They are planted in a larger batch (helpers.replay_vec n_batch, at): the
batch is reset with one seed per env, the fixture's at the planted indices and filler seeds elsewhere,
so the auto-reset of a planted env has to follow the env's own seed, not its index.  The two shapes
are the smallest that reach a full wave and a partial last workgroup on both sides of the 64- and
256-env boundaries.  Every fixture runs under the step kernel its configuration selects; where the
configuration admits the map queue (no traffic, no lane or spawner channels; pgtg_env.hip
choose_launch) it also runs under tune queue_mode 1 (k_envq) and 2 (k_envb), and under mode envq_many:
pgtg_step_many over resident action rows, several ticks per launch of k_envq<BIG, true>, on the
batch of 300 envs in 19 blocks of 16 (the last one of 12) on 4 workgroups, 5 or 4 blocks each; the reference's
recorded outputs are compared after the last tick of every call (helpers.replay_vec chunks).  The last
test asserts that the set stepped every step-kernel instance of tests/test_gpu_create_paths.py ROWS and
both instances of the kernel of several ticks.

The call lengths of envq_many are CHUNKINGS, cycled over the fixtures that admit the queue; every further
pass through the list rotates each chunking by one more place, so that the calls end at many different
ticks (as given, the five end at nine distinct ticks only).  A call of one tick is a launch per tick, and
the call after it begins with a launch of one tick that serves its requests (pgtg_step_many, `q_static`):
_launches counts what the calls must take, one launch per call except there."""
import pytest

import helpers
from test_gpu_create_paths import ROWS

pytestmark = pytest.mark.gpu

SUB = "fuzz"
NAMES = helpers.traj_names(SUB)
SHAPES = [(64, (0, 31, 63)), (300, (0, 63, 64, 255, 256, 299))]
MODES = {"default": None, "envq": dict(queue_mode=1), "envb": dict(queue_mode=2),
         "envq_many": dict(queue_mode=1, envs_per_block=16, queue_grid=4)}
CHUNKINGS = [[1, 24], [2, 3, 20], [5, 7, 13], [4, 4, 4, 4, 4, 5], [12, 13]]  # (the 1: a single-tick call after the reset)
INSTANCES = sorted({k.split(" + ")[0] for row in ROWS.values() for k in row[5:8:2]})


def admits_queue(meta: dict) -> bool:
    feats = meta["kwargs"]["features_to_include_in_observation"]
    return not helpers.has_traffic(meta) and not any(f == "car_spawner" or f.startswith("car_lane") for f in feats)


def _shape(name: str, mode: str, n_envs: int):
    """Cycle the two shapes over the cases (and over the forced kernels of a case); the planted indices
    of the batch of 300 are taken in turn as well.  A fixture of 4 envs goes to the batch of 300, which
    has room for all of them."""
    n = NAMES.index(name) + list(MODES).index(mode)
    n_batch, at = SHAPES[1] if n_envs > len(SHAPES[0][1]) or mode == "envq_many" else SHAPES[n % 2]
    return n_batch, sorted(at[(n // 2 + j) % len(at)] for j in range(n_envs))


RUNS = [(name, mode) for name in NAMES for mode in MODES
        if mode == "default" or admits_queue(helpers.load_traj(name, SUB)["meta"])]
MANY = [name for name, mode in RUNS if mode == "envq_many"]
_done: dict = {}


def _chunks(name: str):
    """(index into CHUNKINGS, the call lengths) of a fixture's envq_many replay"""
    k = MANY.index(name)
    c = CHUNKINGS[k % len(CHUNKINGS)]
    r = (k // len(CHUNKINGS)) % len(c)
    return k % len(CHUNKINGS), c[r:] + c[:r]


def _launches(chunks) -> int:
    """step-kernel launches of the calls after a reset (which leaves no request pending): a call of one tick
    is one launch of the single-step kernel, any other call one launch, or two after a call of one tick"""
    n, static = 0, True
    for k in chunks:
        n += 1 if k == 1 or static else 2
        static = k > 1
    return n


def _big(name: str) -> bool:
    kw = helpers.load_traj(name, SUB)["meta"]["kwargs"]
    return kw["random_map_width"] * kw["random_map_height"] > 64


def _run(name: str, mode: str):
    """(mismatches, info) of one replay, run once per session"""
    if (name, mode) not in _done:
        d = helpers.load_traj(name, SUB)
        n_batch, at = _shape(name, mode, d["meta"]["N"])
        info: dict = {}
        chunks = _chunks(name)[1] if mode == "envq_many" else None
        bad = helpers.replay_vec(d, n_batch=n_batch, at=at, tune=MODES[mode], info=info, chunks=chunks)
        print(f"{name} {mode}: n={n_batch} at={at} {info.get('step_kernel')}" +
              (f" calls {chunks}: {info.get('step_launches')} launches" if chunks else ""))
        _done[(name, mode)] = (bad, info)
    return _done[(name, mode)]


def test_shapes_and_instances():
    """the 64-env shape needs 3 envs at most; both shapes and every planted index are used"""
    used = {(n, b) for name, mode in RUNS for n, at in [_shape(name, mode, helpers.load_traj(name, SUB)["meta"]["N"])]
            for b in at}
    assert used >= {(n, b) for n, at in SHAPES for b in at}
    assert len(INSTANCES) == 8 and all(k.startswith("pgtg::k_env") for k in INSTANCES), INSTANCES


def test_chunkings_cover_the_ticks_and_both_instances():
    """18 fixtures admit the queue, seven of them with more than 64 tiles; the calls of their envq_many replays
    end at 12 or more distinct ticks, and the BIG and the small fixtures each run under three or more of
    CHUNKINGS"""
    assert len(MANY) == 18 and sorted(n for n in MANY if _big(n)) == [
        "wide_03", "wide_09", "wide_11", "wide_12", "wide_15", "wide_33", "wide_39"], MANY
    ends, used = set(), {True: set(), False: set()}
    for name in MANY:
        k, chunks = _chunks(name)
        assert sorted(chunks) == sorted(CHUNKINGS[k]) and sum(chunks) == 25, (name, chunks)
        ends |= {sum(chunks[:j + 1]) - 1 for j in range(len(chunks))}
        used[_big(name)].add(k)
    print(sorted(ends), used)
    assert len(ends) >= 12, sorted(ends)
    assert len(used[True]) >= 3 and len(used[False]) >= 3, used
    assert {tuple(_chunks(n)[1]) for n in MANY[:len(CHUNKINGS)]} == {tuple(c) for c in CHUNKINGS}  # (as given)
    assert [_launches(c) for c in ([1, 24], [24, 1], [2, 3, 20], [1, 1, 23])] == [3, 2, 3, 4]


@pytest.mark.parametrize("name,mode", RUNS)
def test_fuzz_fixture_planted_in_a_larger_batch(name, mode):
    bad, info = _run(name, mode)
    assert not bad, (info.get("step_kernel"), bad[:10])
    assert info["errors"] == 0
    if mode != "default" and info["step_kernel"].startswith("pgtg::k_envq"):
        assert MODES[mode]["queue_mode"] == 1
    if mode != "default" and info["step_kernel"].startswith("pgtg::k_envb"):
        assert MODES[mode]["queue_mode"] == 2
    if mode == "envq_many":
        # step_kernel() names the single-step instance; the launch count shows that the calls ran several
        # ticks per launch (25 launches otherwise)
        chunks = _chunks(name)[1]
        assert info["step_kernel"] == ("pgtg::k_envq<true>" if _big(name) else "pgtg::k_envq<false>"), info
        assert info["calls"] == len(chunks) and info["end_ticks"][-1] == 24, info
        assert info["step_launches"] == _launches(chunks), (chunks, info)


def test_every_step_kernel_instance_was_stepped_by_a_fuzz_fixture():
    runs = {k: 0 for k in INSTANCES}
    many = {True: 0, False: 0}  # replays of several ticks per launch: more than 64 tiles, at most 64
    for name, mode in RUNS:
        bad, info = _run(name, mode)  # (run already when the whole file runs)
        kernel = info["step_kernel"].split(" + ")[0]
        assert kernel in runs, kernel
        runs[kernel] += 1
        if mode == "envq_many" and kernel.startswith("pgtg::k_envq") and info["step_launches"] < info["end_ticks"][-1] + 1:
            many[_big(name)] += 1
    print({k: n for k, n in runs.items()}, many)
    assert all(n >= 1 for n in runs.values()), runs
    assert many[True] >= 1 and many[False] >= 1, many
