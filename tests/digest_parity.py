"""Driver of the every-env, every-step parity tests (tests/test_gpu_exhaustive.py,
tests/test_gpu_truncation.py): a seeded random-action rollout of a whole batch on the GPU, condensed
per (step, env) into the digest of pgtg_amd/digest.py, against the CPU restatement's digests of the
same rollout (oracle.rollout_digest; tests/test_digest.py pins the two formulas to each other)."""
import warnings
from types import SimpleNamespace

import numpy as np

import helpers  # noqa: F401
from oracle import oracle
from pgtg_amd import config as cfg

ACT_SEED = 0xA11CE


def _spec(kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cfg.make_spec(**kw)


def _gpu_digests(spec, n, T, tune=None, max_episode_steps=0):
    from pgtg_amd.digest import Digest
    from pgtg_amd.vector import PGTGVecEnv
    env = PGTGVecEnv(n, spec=spec, device=0, autoreset=True, max_episode_steps=max_episode_steps or None, tune=tune)
    try:
        env.reset(seed=0)
        dg = Digest(env)
        out = np.zeros((T, n), dtype=np.uint64)
        for t in range(T):
            env.step_random(ACT_SEED, t)
            out[t] = dg.step_digest().cpu().numpy().view(np.uint64)
        return out, env.step_kernel(), env.launch_info(), env.queue_overflow()
    finally:
        env.close()


def _compare_run(spec, n, T, tune=None, tag="", min_distinct=1000, max_episode_steps=0):
    """The comparison; returns what the rollout ran as (kernel name, launch_info, overflow requests
    served) and the restatement's flags [T, n] (bit 0 terminated, bit 1 truncated)."""
    got, kern, shape, ovf = _gpu_digests(spec, n, T, tune, max_episode_steps)
    ref, flags = oracle.rollout_digest(spec, n, T, ACT_SEED, max_episode_steps=max_episode_steps, flags_out=True)
    # the comparison has teeth: the rollout visits many distinct outputs.  Observations are local
    # 9x9 windows, so envs on small maps share digests (3x3 maps: 4 096 envs x 100 steps give 7 326
    # distinct ones, 262 144 x 20 give 13 072)
    assert len(np.unique(ref)) >= min(ref.size // 4, min_distinct), "degenerate digests"
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (f"{tag} {kern} {shape}: {len(bad)} (step, env) digests differ, first {bad[:8].tolist()}")
    return SimpleNamespace(kernel=kern, launch=shape, overflow=ovf, flags=flags)


def _compare(spec, n, T, tune=None, tag="", min_distinct=1000):
    return _compare_run(spec, n, T, tune, tag, min_distinct).overflow
