"""Seeded random configurations (map size, connections, obstacles and their weights, feature lists
in random order, sliding windows, next-subgoal direction, rewards and penalties, obstacle effect
probabilities, traffic density, light phases, driver mix, cost channel) on maps of up to 64 tiles
and batches of 64-3000 envs, every step compared with the CPU oracle on a sample of envs: observations, reward, cost,
termination, position, next-subgoal direction and cars.  The oracle is pinned to the reference on
these very 40 configurations by the fuzz fixtures (tests/golden/fuzz/traj_fuzz_NN.npz is
random_kwargs(NN) run by the reference; tests/test_oracle_fuzz.py) besides the hand-picked ones
(tests/test_oracle_golden.py); this widens the feature combinations the HIP path is held to.  The
distribution itself lives in tests/fuzz_configs.py, which the fixture generator imports too."""
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
from fuzz_configs import FEATURES, random_kwargs  # noqa: F401
from oracle.oracle import OracleEnv
from pgtg_amd import config as cfg

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("k", range(40))
def test_random_config_parity(k):
    from pgtg_amd.vector import PGTGVecEnv
    kw = random_kwargs(k)
    # batch sizes across the launch shapes (small workgroups, map queue, several workgroups)
    n, T = int(np.random.default_rng(k).choice([64, 200, 768, 3000])), 25
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec = cfg.make_spec(**kw)
    rng = np.random.default_rng(k)
    fixed = [i for i in (0, 1, 63, 64, 255, 256, n - 1) if i < n]
    idx = np.unique(np.concatenate([fixed, rng.choice(n, 9, replace=False)]))
    tix = torch.as_tensor(idx, device="cuda")
    env = PGTGVecEnv(n, spec=spec, device=0)
    try:
        env.reset(seed=100 + k)
        orcs = {int(i): OracleEnv(spec) for i in idx}
        m0 = env.obs_map.index_select(0, tix).cpu().numpy()
        for j, i in enumerate(idx):
            r = orcs[int(i)].reset(100 + k + int(i))
            assert np.array_equal(m0[j], r["obs"]), f"case {k} reset obs env {int(i)}: {kw}"
        acts = env.random_actions(T, 77 + k)
        for t in range(T):
            env.step_actions(acts[t])
            torch.cuda.synchronize()
            a = acts[t].index_select(0, tix).cpu().numpy()
            m = env.obs_map.index_select(0, tix).cpu().numpy()
            fm = env.final_map.index_select(0, tix).cpu().numpy()
            rew = env.reward.index_select(0, tix).cpu().numpy()
            term = env.terminated.index_select(0, tix).cpu().numpy()
            pos = env.position.index_select(0, tix).cpu().numpy()
            cost = env.cost.index_select(0, tix).cpu().numpy() if env.cost is not None else None
            nsd = env.nsd.index_select(0, tix).cpu().numpy() if env.nsd is not None else None
            for j, i in enumerate(idx):
                o = orcs[int(i)]
                r = o.step(int(a[j]))
                tag = f"case {k} t{t} env{int(i)}"
                assert rew[j] == r["reward"] and bool(term[j]) == r["terminated"], tag + f" reward/terminated {kw}"
                if cost is not None:
                    assert cost[j] == r["cost"], tag + " cost"
                if r["terminated"]:
                    assert np.array_equal(fm[j], r["obs"]), tag + " terminal obs"
                    r = o.reset(None)
                assert np.array_equal(m[j], r["obs"]), tag + f" obs {kw}"
                assert tuple(pos[j]) == tuple(r["pos"]), tag + " position"
                if nsd is not None:
                    assert int(nsd[j]) == int(r["nsd"]), tag + " next subgoal direction"
                if spec.traffic_density > 0:
                    assert np.array_equal(env.cars(int(i)), o.cars()), tag + " cars"
    finally:
        env.close()


# Batches above the small-workgroup sizes: the 32/64/128/256-env layouts, the map queue and the
# sub-batched observation pass under random feature combinations.  Every env at every step is
# compared through the output digest (tests/test_gpu_exhaustive.py); traffic configurations are
# capped at 40 000 envs to keep the restatement's share of the test in seconds.
BIG = {  # fuzz seed: batch size
    3: 12000, 7: 40000, 11: 140000, 17: 20000, 23: 70000, 29: 300000,
}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("k", sorted(BIG))
def test_random_config_every_env_large_batches(k):
    from test_gpu_exhaustive import _compare, _spec
    kw = random_kwargs(k)
    n = BIG[k]
    if kw["traffic_density"] > 0:
        n = min(n, 40000)
    # (few feature channels on small maps give few distinct observations)
    _compare(_spec(kw), n, 10, None, f"fuzz {k} n={n} {kw}", min_distinct=200)
