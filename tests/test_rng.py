"""CPU oracle's numpy Generator restatement vs numpy itself and vs the committed numpy vectors."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
from oracle import oracle as O


def _gen(seed, key):
    g = O.OrcPcg()
    O.lib().orc_pcg64_from_seed(int(seed), int(key), 1, C.byref(g))
    return g


def test_seed_sequence_children_match_committed_vectors():
    z = np.load(os.path.join(helpers.GOLDEN, "rng_numpy.npz"))
    for a, s in enumerate(z["seeds"]):
        for b, k in enumerate(z["keys"]):
            g = _gen(s, k)
            st = z["pcg_state"][a, b]
            assert (g.st_hi, g.st_lo, g.inc_hi, g.inc_lo) == tuple(int(x) for x in st)
            raw = [O.lib().orc_next64(C.byref(g)) for _ in range(8)]
            assert raw == [int(x) for x in z["pcg_raw"][a, b]]


def test_mixed_draw_script_matches_committed_vectors():
    z = np.load(os.path.join(helpers.GOLDEN, "rng_numpy.npz"))
    g = _gen(42, 3)
    L = O.lib()
    p = np.array([0.25, 0.35, 0.2, 0.15, 0.05])
    for (kind, n), want in zip(z["script"], z["script_vals"]):
        if kind == 0:
            got = L.orc_random(C.byref(g))
        elif kind == 1:
            got = float(L.orc_integers(C.byref(g), 0, int(n)))
        elif kind == 2:
            got = float(L.orc_choice_p(C.byref(g), p.ctypes.data_as(C.POINTER(C.c_double)), 5))
        else:
            got = float(L.orc_integers(C.byref(g), 1, 4))
        assert got == want


def test_choice_without_replacement_matches_committed_vectors():
    z = np.load(os.path.join(helpers.GOLDEN, "rng_numpy.npz"))
    g = _gen(9, 1)
    flat, i = z["noreplace"], 0
    while i < len(flat):
        pop, k = int(flat[i]), int(flat[i + 1])
        want = flat[i + 2:i + 2 + k]
        out = (C.c_int64 * k)()
        O.lib().orc_choice_noreplace(C.byref(g), pop, k, out)
        assert list(out) == [int(x) for x in want], (pop, k)
        i += 2 + k


@pytest.mark.parametrize("seed", [0, 5, 2**40 + 3])
def test_live_numpy_generator(seed):
    g = _gen(seed, 7)
    ref = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(7,))))
    L = O.lib()
    for t in range(500):
        if t % 3 == 0:
            assert L.orc_random(C.byref(g)) == ref.random()
        elif t % 3 == 1:
            n = 2 + t % 97
            assert L.orc_integers(C.byref(g), 0, n) == ref.integers(0, n)
        else:
            assert L.orc_integers(C.byref(g), 0, 9) == ref.choice(9)


# ---- Lemire's rejection loop (left < 2^32 mod n: one more 32-bit half) pinned to live numpy ----
# 2^32 mod n: 2^30 (a quarter of the draws reject), 2^31 - 1 (half), 1, 2^16, 1, 7296, and n = 2^32, which
# numpy serves with a plain next_uint32
BIG_N = (3 * 2**30, 2**31 + 1, 2**32 - 1, 2**32, 2**32 - 2**16, 65535, 10007)


@pytest.mark.parametrize("seed,key", [(0, 7), (5, 1), (2**40 + 3, 4)])
def test_large_bounds_reject_like_numpy(seed, key):
    g = _gen(seed, key)
    ref = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(key,))))
    L = O.lib()
    plain32 = 0
    with O.Trace(cap=8192) as tr:
        for t in range(4000):
            if t % 3 == 0 or t % 7 == 0:  # doubles leave the buffered half alone: both parities occur
                assert L.orc_random(C.byref(g)) == ref.random()
                continue
            n = BIG_N[t % len(BIG_N)] if t % 5 else 2 + t % 97
            had = g.has32
            before = tr.count()
            assert L.orc_integers(C.byref(g), 0, n) == ref.integers(0, n), (t, n)
            if n == 2**32:  # no Lemire: exactly one half taken, nothing for the trace to see
                assert tr.count() == before and g.has32 == 1 - had
                plain32 += 1
        recs = tr.records()
    st = ref.bit_generator.state
    assert (g.st_hi << 64 | g.st_lo) == st["state"]["state"] and g.has32 == st["has_uint32"]
    rej = [r for r in recs if r["rejects"] > 0]
    assert plain32 > 100 and all(r["n"] != 0 for r in recs)
    assert len(rej) > 100, len(rej)
    assert any(r["rejects"] >= 2 for r in rej)  # two halves in a row rejected by one draw
    assert any(r["buffered"] for r in rej) and any(not r["buffered"] for r in rej)
    assert any(r["rejects"] == 0 for r in recs)  # left < n but not < 2^32 mod n: accepted
    assert all(r["site"] == "other" for r in recs)


def _choice_trace(seed, pop, k):
    g = _gen(seed, 1)
    out = (C.c_int64 * k)()
    with O.Trace(cap=64) as tr:
        O.lib().orc_choice_noreplace(C.byref(g), pop, k, out)
        recs = [r for r in tr.records() if r["rejects"] > 0]
    return list(out), recs


def _find_choice_seeds(pop, k, budget):
    """the first seeds whose choice(pop, k, replace=False) rejects a draw in Floyd's loop / in the
    shuffle, searched with the oracle (numpy cannot tell) and then verified against numpy"""
    found = {}
    for seed in range(budget):
        for r in _choice_trace(seed, pop, k)[1]:
            found.setdefault(r["site"], seed)
        if len(found) == 2:
            break
    return found


# (pop, k, seeds to search): a rejection per call has a chance of about k * n / 2^33, so the search is a few
# thousand calls for the large populations and some ten thousand for the small one (a second in all)
CHOICE_CASES = [(10000, 5000, 20000), (10000, 10000, 20000), (2500, 700, 300000)]
CHOICE_SEEDS = {(pop, k): _find_choice_seeds(pop, k, budget) for pop, k, budget in CHOICE_CASES}


@pytest.mark.parametrize("pop,k", [c[:2] for c in CHOICE_CASES])
@pytest.mark.parametrize("site", ["floyd", "shuffle"])
def test_choice_without_replacement_rejections_match_numpy(pop, k, site):
    assert site in CHOICE_SEEDS[(pop, k)], f"no {site} rejection found for choice({pop}, {k})"
    seed = CHOICE_SEEDS[(pop, k)][site]
    out, recs = _choice_trace(seed, pop, k)
    hit = [r for r in recs if r["site"] == site]
    assert hit, recs
    for r in hit:  # the trace's ordinal is the draw's index: Floyd 0 .. k-1 with n = pop-k+d+1, shuffle k .. 2k-2
        assert r["n"] == (pop - k + r["ord"] + 1 if site == "floyd" else 2 * k - r["ord"])
    ref = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(1,))))
    assert out == [int(x) for x in ref.choice(pop, k, replace=False)]
