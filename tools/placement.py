"""Diagnostic: does a workgroup's speed in k_envq<BIG, true> repeat from launch to launch?  (-DPGTG_STAMPS build.)

Build: python -m pgtg_amd.build --tools=stamps
Usage: python tools/placement.py [case] [launches]      (case: a key of CASES below, default cfg5big; launches >= 3)
After the single steps and the hand-over tick, `launches` consecutive pgtg_step_many calls of T = PGTG_STAMP_TICKS
(default 64) ticks, one launch each, the per-tick wall-clock stamps of wave 0 (STAMPT) read back after each.  Per
launch: every workgroup's mean tick (ticks 1.., tick 0 holds the ramp) and its time per block; between launch k and
k + 1: the correlation of the workgroups' mean ticks.  Then the split the share rule has to level: the workgroups more
than 5 % above the mean against the rest.  PGTG_SHARES=0 freezes equal block shares where the library has the hook."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pgtg_amd import _abi  # noqa: E402

_abi.LIB_PATH = os.environ.get("PGTG_STAMPS_LIB") or os.path.join(os.path.dirname(_abi.LIB_PATH), "libpgtg_hip_stamps.so")
from pgtg_amd.vector import PGTGVecEnv  # noqa: E402
from stamp_layout import REAL_BASE, REAL_ROW, TICK_BASE, TICK_ROW  # noqa: E402

CASES = {"cfg5big": (1048576, dict(random_map_width=5, random_map_height=5)),
         "cfg5half": (524288, dict(random_map_width=5, random_map_height=5)),
         "cfg5": (131072, dict(random_map_width=5, random_map_height=5))}
name = sys.argv[1] if len(sys.argv) > 1 else "cfg5big"
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 4
T = int(os.environ.get("PGTG_STAMP_TICKS", "64"))
N, kw = CASES[name]
env = PGTGVecEnv(N, device=0, **kw)
E, _ = env.launch_info()
env.reset(seed=0)
for k in range(30):
    env.step_random(1, k)
env.step_many(env.random_actions(2, 2))  # (the hand-over tick and one more: the lists are static from here)
torch.cuda.synchronize()
blocks = (N + E - 1) // E
nw = blocks * 4
lib = _abi.lib()
lib.pgtg_read_stamps.argtypes = [C.c_void_p, C.c_uint64]
frozen = os.environ.get("PGTG_SHARES") == "0" and hasattr(env, "set_block_shares")
means, ends_all, counts_all = [], [], []
for k in range(launches):
    base = env.step_launches()
    if frozen and k == 0:
        g = env.block_shares().size
        eq = np.full(g, blocks // g, np.uint32)
        eq[:blocks % g] += 1
        env.set_block_shares(eq, freeze=True)
    counts_all.append(env.block_shares().copy() if hasattr(env, "block_shares") else None)
    env.step_many(env.random_actions(T, 3 + k))
    torch.cuda.synchronize()
    assert env.step_launches() == base + 1, "one launch per call"
    buf = np.zeros(REAL_BASE + REAL_ROW * nw, np.uint64)
    lib.pgtg_read_stamps(buf.ctypes.data, buf.size)
    rt = buf[REAL_BASE:REAL_BASE + REAL_ROW * nw].reshape(nw, REAL_ROW).astype(np.int64)
    wgs = int(np.nonzero(rt[:, 2] > 0)[0].max()) // 4 + 1
    tt = buf[TICK_BASE:TICK_BASE + TICK_ROW * wgs].reshape(wgs, TICK_ROW)[:, :T].astype(np.int64)
    beg0 = rt[0:4 * wgs:4, 2]
    t0 = beg0.min()
    d = np.diff(tt, axis=1)  # ticks 1..
    m = d.mean(1) / 100  # us
    means.append(m)
    last = tt[:, -1] - t0
    ends_all.append(last)
    print(f"launch {k}: workgroups {wgs}, ticks {T}; us: mean tick {m.mean():.1f}, std between workgroups {m.std():.2f}, "
          f"slowest {m.max() - m.mean():.2f} above the mean, p99 {np.percentile(m, 99) - m.mean():.2f}; launch end: last "
          f"{last.max() / 100:.1f}, average {last.mean() / 100:.1f}, tail per tick {(last.max() - last.mean()) / 100 / T:.2f}",
          flush=True)
    c = counts_all[-1]
    if c is not None:
        print(f"  block shares of this launch (count: workgroups): {dict(zip(*[x.tolist() for x in np.unique(c, return_counts=True)]))}")
for k in range(launches - 1):
    r = np.corrcoef(means[k], means[k + 1])[0, 1]
    print(f"correlation of the workgroups' mean tick, launch {k} against {k + 1}: {r:.3f}")
m = np.mean(means, axis=0)
slow = m > 1.05 * m.mean()
print(f"over {launches} launches: {int(slow.sum())} of {m.size} workgroups more than 5 % above the mean tick "
      f"({m.mean():.1f} us); their mean tick {m[slow].mean() if slow.any() else 0:.1f} us, the others' {m[~slow].mean():.1f} us")
idx = np.nonzero(slow)[0]
print(f"  slow workgroups by index mod 8: {np.bincount(idx % 8, minlength=8).tolist()}; by index // 128: "
      f"{np.bincount(idx // 128, minlength=(m.size + 127) // 128).tolist()}")
env.close()
