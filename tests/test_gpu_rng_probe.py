"""The device RNG (pgtg_amd/csrc/pgtg_device.h) against live numpy, without the env kernels around it:
tests/csrc/rng_probe.hip runs one lane per Generator(PCG64(SeedSequence(seed, spawn_key=(key,))))
stream through a host-given script of draws and returns every value and the final stream state.

What the env tests cannot reach: Lemire's rejection loop (left < 2^32 mod n) of pcg_int, pcg_draw,
ahead_draw and ahead_int with n where most draws reject (so the lanes of the wave diverge in it),
with and without a buffered half; pcg_advance for every table entry and its compositions against
PCG64.advance; the seeding of 64-bit seeds and large spawn keys.  Everything is integer-exact: the
comparison is equality, there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import helpers  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu

OP_PCG_INT, OP_DRAW_INT, OP_DRAW_DBL, OP_AHEAD_DRAW_INT, OP_AHEAD_DRAW_DBL, OP_AHEAD_INT = 0, 1, 2, 3, 4, 5
OP_NEXT32, OP_ADVANCE_NEXT64, OP_ADVANCE = 6, 7, 8
INT_KINDS = (OP_PCG_INT, OP_DRAW_INT, OP_AHEAD_DRAW_INT, OP_AHEAD_INT)
DBL_KINDS = (OP_DRAW_DBL, OP_AHEAD_DRAW_DBL)
# the double draw that belongs to an integer kind's family
DBL_OF = {OP_PCG_INT: OP_DRAW_DBL, OP_DRAW_INT: OP_DRAW_DBL, OP_AHEAD_DRAW_INT: OP_AHEAD_DRAW_DBL,
          OP_AHEAD_INT: OP_AHEAD_DRAW_DBL}
# bounds with a large rejection zone 2^32 mod n: 2^30 (25 %), 2^31 - 1 (50 %), 1, 2^16, 1, 7296 ... 3 539
BIG_N = (3 * 2**30, 2**31 + 1, 2**32 - 1, 2**32 - 2**16, 65535, 10007)

SEEDS = [0, 1, 5, 2**32 - 1, 2**32, 2**40 + 3, 2**63 + 5, 2**64 - 1]
KEYS = [0, 1, 2, 3, 4, 1000, 2**31, 2**32 - 1]
STREAMS = [(s, k) for s in SEEDS for k in KEYS]  # 64: one wave


def device_run(streams, script, persist=False):
    """script: [n_ops, 2] (shared) or [n_streams, n_ops, 2]; -> init [S, 6], values [S, n_ops], final [S, 6]"""
    import rng_probe_build
    L = rng_probe_build.lib()
    seeds = np.array([s for s, _ in streams], dtype=np.uint64)
    keys = np.array([k for _, k in streams], dtype=np.uint32)
    sc = np.ascontiguousarray(script, dtype=np.uint32)
    per_stream = sc.ndim == 3
    n_ops = sc.shape[-2]
    S = len(streams)
    init = np.zeros((S, 6), np.uint64)
    vals = np.zeros((S, n_ops), np.uint64)
    fin = np.zeros((S, 6), np.uint64)
    rc = L.rng_probe_run(seeds.ctypes.data, keys.ctypes.data, S, sc.ctypes.data, n_ops, int(per_stream), int(persist),
                         init.ctypes.data, vals.ctypes.data, fin.ctypes.data)
    assert rc == 0, f"rng_probe_run: HIP error {rc}"
    return init, vals, fin


def _state6(bg):
    st = bg.state
    s, inc = st["state"]["state"], st["state"]["inc"]
    m = 2**64 - 1
    return [s >> 64, s & m, inc >> 64, inc & m, st["uinteger"], st["has_uint32"]]


def numpy_run(seed, key, script):
    """the same script on numpy's Generator: (initial state, values, final state)"""
    bg = np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(key,)))
    gen = np.random.Generator(bg)
    init = _state6(bg)
    vals = []
    for kind, n in script:
        kind, n = int(kind), int(n)
        if kind in INT_KINDS:
            vals.append(0 if n <= 1 else int(gen.integers(0, n)))
        elif kind in DBL_KINDS:
            vals.append(int(gen.random() * 2.0**53))
        elif kind == OP_NEXT32:
            vals.append(int(gen.integers(0, 2**32)))
        else:  # PCG64.advance drops the buffered half; pcg_advance documents that it keeps it
            st = bg.state
            bg.advance(n)
            st2 = bg.state
            st2["has_uint32"], st2["uinteger"] = st["has_uint32"], st["uinteger"]
            bg.state = st2
            vals.append(int(bg.random_raw()) if kind == OP_ADVANCE_NEXT64 else 0)
    return init, vals, _state6(bg)


def check(streams, script, persist=False):
    """device == numpy for every stream: seeding, every value, final state (the buffered half only
    where one is held).  Returns the device's final states."""
    sc = np.asarray(script)
    init, vals, fin = device_run(streams, sc, persist)
    for i, (seed, key) in enumerate(streams):
        ri, rv, rf = numpy_run(seed, key, sc[i] if sc.ndim == 3 else sc)
        assert [int(x) for x in init[i, :4]] == ri[:4], f"stream {i} ({seed}, {key}): seeding"
        got = [int(x) for x in vals[i]]
        if got != rv:
            j = next(j for j in range(len(rv)) if got[j] != rv[j])
            op = (sc[i] if sc.ndim == 3 else sc)[j]
            raise AssertionError(f"stream {i} ({seed}, {key}) op {j} kind {op[0]} n {op[1]}: {got[j]} != numpy {rv[j]}")
        f = [int(x) for x in fin[i]]
        assert f[:4] == rf[:4] and f[5] == rf[5], f"stream {i} ({seed}, {key}): final state"
        if rf[5]:
            assert f[4] == rf[4], f"stream {i} ({seed}, {key}): buffered half"
    return fin


def oracle_rejections(seed, key, script):
    """(draws that rejected, most halves one draw rejected, rejections met with a buffered half) of
    the script's integer draws on the CPU oracle"""
    L = O.lib()
    g = O.OrcPcg()
    L.orc_pcg64_from_seed(int(seed), int(key), 1, C.byref(g))
    with O.Trace(cap=len(script) + 8) as tr:
        for kind, n in script:
            if int(kind) in INT_KINDS:
                L.orc_integers(C.byref(g), 0, int(n))
            else:
                L.orc_random(C.byref(g))
        recs = [r for r in tr.records() if r["rejects"] > 0]
    return len(recs), max([r["rejects"] for r in recs], default=0), sum(r["buffered"] for r in recs)


def big_script(kind, n_ops=240):
    """BIG_N in turn, a double before every third and every seventh draw: the integer draws meet the
    buffer in both states"""
    sc, j = [], 0
    while len(sc) < n_ops:
        if j % 3 == 0 or j % 7 == 0:
            sc.append((DBL_OF[kind], 0))
        sc.append((kind, BIG_N[j % len(BIG_N)]))
        j += 1
    return sc[:n_ops]


@pytest.mark.parametrize("kind", INT_KINDS, ids=["pcg_int", "pcg_draw", "ahead_draw", "ahead_int"])
def test_large_bounds_reject_divergently(kind):
    sc = big_script(kind)
    rej = [oracle_rejections(s, k, sc) for s, k in STREAMS]
    # the script does what it is for: every lane rejects many draws (at its own places), some draw
    # rejects twice or more, and rejections happen with and without a buffered half
    assert all(r[0] >= 10 for r in rej), min(r[0] for r in rej)  # (about 22 expected per lane)
    assert max(r[1] for r in rej) >= 2
    assert sum(r[2] for r in rej) > 0 and sum(r[0] - r[2] for r in rej) > 0
    assert len({r[0] for r in rej}) > 8  # the lanes' loop counts differ
    check(STREAMS, sc)


@pytest.mark.parametrize("hi", [28, 600])
def test_small_bounds_per_lane_scripts(hi):
    """n in 2..hi (the routes of a square / the squares of a map), every lane its own script of all
    four integer draws and doubles; two blocks (70 streams: the kernel's bounds guard)"""
    rng = np.random.default_rng(hi)
    streams = STREAMS + [(77 + i, 6) for i in range(6)]
    n_ops = 300
    sc = np.zeros((len(streams), n_ops, 2), np.uint32)
    kinds = np.array(INT_KINDS + DBL_KINDS + (OP_NEXT32,))
    sc[:, :, 0] = kinds[rng.integers(0, len(kinds), size=sc.shape[:2])]
    sc[:, :, 1] = rng.integers(2, hi + 1, size=sc.shape[:2])
    one = (sc[:, :, 0] == OP_PCG_INT) | (sc[:, :, 0] == OP_AHEAD_INT)
    sc[:, :, 1] = np.where(one & (rng.random(sc.shape[:2]) < 0.1), 1, sc[:, :, 1])  # n == 1 draws nothing
    check(streams, sc)


def test_persistent_lookahead_equals_plain():
    """One PcgAhead kept over the whole script (as the car loops keep it) draws what numpy draws and
    leaves the state that the plain functions leave after the same script."""
    sc_a, sc_p = [], []
    rng = np.random.default_rng(3)
    for j in range(300):
        r = int(rng.integers(0, 3))
        n = int(BIG_N[j % len(BIG_N)] if j % 2 else rng.integers(2, 29))
        sc_a.append([(OP_AHEAD_DRAW_INT, n), (OP_AHEAD_DRAW_DBL, 0), (OP_AHEAD_INT, n)][r])
        sc_p.append([(OP_DRAW_INT, n), (OP_DRAW_DBL, 0), (OP_PCG_INT, n)][r])
    fa = check(STREAMS, sc_a, persist=True)
    fp = check(STREAMS, sc_p)
    has = fp[:, 5] == 1
    assert np.array_equal(fa[:, :4], fp[:, :4]) and np.array_equal(fa[:, 5], fp[:, 5])
    assert np.array_equal(fa[has, 4], fp[has, 4])


def test_advance_matches_numpy():
    """pcg_advance(d) for every table entry d = 2^b, d = 0, 1, 65 535 and 200 random d per lane, each
    followed by an output, with next_uint32 draws between so that the jump meets the buffer in both
    states (it must leave the buffer as it is)."""
    rng = np.random.default_rng(16)
    S = len(STREAMS)
    fixed = [2**b for b in range(16)] + [0, 1, 65535]
    ds = np.concatenate([np.tile(np.array(fixed), (S, 1)), rng.integers(0, 65536, size=(S, 200))], axis=1)
    ops = []
    for j in range(ds.shape[1]):
        ops.append(np.stack([np.full(S, OP_ADVANCE_NEXT64), ds[:, j]], axis=1))
        if j % 3 != 2:
            ops.append(np.tile([OP_NEXT32, 0], (S, 1)))
        if j % 5 == 0:  # a jump straight after a jump, no output between
            ops.append(np.stack([np.full(S, OP_ADVANCE), ds[:, (j * 7) % ds.shape[1]]], axis=1))
    check(STREAMS, np.stack(ops, axis=1))
