"""The block-share rule of k_envq<BIG, true> (pgtg_amd/csrc/pgtg_shares.h) on the host.

The header has no HIP in it: a small stand-alone program around shares_assign() is compiled with the host
compiler, once plainly and once with -fsanitize=address,undefined, and fed cases on its standard input
(`n nblk cap_blocks` then n estimates per case; it prints the return code and the counts)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = r"""
#include <cstdio>
#include <vector>
#include "pgtg_shares.h"
int main() {
  unsigned n;
  unsigned long long nblk, cap;
  while (scanf("%u %llu %llu", &n, &nblk, &cap) == 3) {
    std::vector<uint32_t> est(n), count(n);
    std::vector<uint64_t> rem(n), key(n);
    for (auto& e : est) if (scanf("%u", &e) != 1) return 2;
    const int rc = shares_assign(est.data(), n, nblk, cap, count.data(), rem.data(), key.data());
    printf("%d", rc);
    for (auto c : count) printf(" %u", c);
    printf("\n");
  }
  return 0;
}
"""


def _compile(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = os.path.join(tmp, "shares_main.cpp")
    with open(src, "w") as f:
        f.write(MAIN)
    exe = os.path.join(tmp, name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", *extra, "-I", os.path.join(ROOT, "pgtg_amd", "csrc"), "-o", exe, src],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("shares"))
    return _compile(tmp, "shares", []), _compile(tmp, "shares_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, cases):
    text = "".join(f"{len(e)} {nblk} {cap}\n{' '.join(str(int(x)) for x in e)}\n" for e, nblk, cap in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    res = []
    for line in out:
        v = [int(x) for x in line.split()]
        res.append((v[0], np.array(v[1:], np.int64)))
    return res


def _clamps(n, nblk, cap):
    base = nblk // n
    return max(1, base - 2), min(base + 2, cap)


def _cases():
    rng = np.random.default_rng(5)
    cases = []
    for n, nblk in [(8, 71), (64, 71), (4, 4), (4, 19), (1024, 8192), (1024, 4096), (37, 1000), (1, 9), (4096, 65536)]:
        cap = 3 * -(-nblk // n)
        cases.append((np.full(n, 600), nblk, cap))  # equal speeds
        cases.append((rng.integers(300, 900, n), nblk, cap))
        cases.append((np.where(np.arange(n) % 3 == 0, 1, 0x7fffffff), nblk, cap))  # every clamp binds
        cases.append((np.sort(rng.integers(500, 700, n)), nblk, cap))  # monotone speeds
    return cases


def test_invariants_on_both_builds(exes):
    """Sum, clamps, equal shares for equal speeds, monotone in speed, ties to the lower index, and the same
    answers from the sanitizer build (which aborts on any finding)."""
    cases = _cases()
    plain, san = _run(exes[0], cases), _run(exes[1], cases)
    for (est, nblk, cap), (rc, c), (rc2, c2) in zip(cases, plain, san):
        n = len(est)
        lo, hi = _clamps(n, nblk, cap)
        assert rc == 0 and rc2 == 0 and np.array_equal(c, c2), (n, nblk)
        assert c.sum() == nblk and c.min() >= lo and c.max() <= hi, (n, nblk, c.min(), c.max(), lo, hi)
        if np.all(est == est[0]):  # equal speeds: equal shares, the remainder to the lowest indices
            assert np.array_equal(c, nblk // n + (np.arange(n) < nblk % n)), (n, nblk)
        # a workgroup that is no slower never gets fewer blocks, save for the one block of rounding;
        # at equal estimates the lower index has at least as many
        order = np.argsort(est, kind="stable")
        cs = c[order]
        assert np.all(np.maximum.accumulate(cs[::-1])[::-1][1:] <= cs[:-1] + 1), (n, nblk)
        same = est[order][1:] == est[order][:-1]
        assert np.all(cs[1:][same] <= cs[:-1][same]), (n, nblk)
    # the same input twice: the same output
    again = _run(exes[0], cases[:8])
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(again, plain[:8]))


def test_infeasible_clamps_are_refused(exes):
    (rc, _), = _run(exes[0], [(np.full(4, 600), 19, 4)])  # 4 x min(6, 4) < 19
    assert rc == -1


def test_measured_split_of_1024_workgroups_is_levelled(exes):
    """profiles/level/placement.txt: workgroups 512..1023 of the 1 048 576-env launch run a tick of 8 blocks in
    366.6 us, workgroups 0..511 in 297.3 us.  With the rule's shares the slowest workgroup's predicted tick is
    below the equal-share one's."""
    per_block = np.where(np.arange(1024) >= 512, 366.6, 297.3) / 8  # us
    est = np.round(per_block * 100 * 16).astype(np.int64)  # 100 MHz ticks in 1/16
    (rc, c), = _run(exes[1], [(est, 8192, 24)])
    assert rc == 0 and c.sum() == 8192
    assert set(c[:512]) == {9} and set(c[512:]) == {7}, np.unique(c, return_counts=True)
    assert (c * per_block).max() < (8 * per_block).max() - 25  # 334.5 against 366.6 us
