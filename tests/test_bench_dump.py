"""bench.py --dump-outputs: the files are float32/float64, within the byte budget, the same sample of
envs from run to run, and the terminal rows are kept only for the envs that finished."""
import os

import numpy as np
import torch

import bench


def _arrays(n):
    g = torch.Generator().manual_seed(3)
    return {"obs_map": torch.randint(1, 255, (n, 9, 9, 9), dtype=torch.uint8, generator=g),
            "position": torch.randint(0, 45, (n, 2), dtype=torch.int32, generator=g),
            "reward": torch.randn(n, dtype=torch.float64, generator=g),
            "terminated": torch.rand(n, generator=g) > 0.5,
            "cost": None,
            "final_obs_map": torch.randint(1, 255, (n, 9, 9, 9), dtype=torch.uint8, generator=g)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_batch_is_dumped_whole(tmp_path):
    n = 37
    a = _arrays(n)
    bench.dump_outputs(str(tmp_path), a, n, env_offset=100, valid=a["terminated"])
    d = _load(tmp_path)
    assert sorted(d) == ["env_index", "final_obs_map", "obs_map", "position", "reward", "terminated"]
    assert np.array_equal(d["env_index"], np.arange(100, 100 + n))
    assert d["reward"].dtype == np.float64 and np.array_equal(d["reward"], a["reward"].numpy())
    for k in ("obs_map", "position", "terminated", "final_obs_map"):
        assert d[k].dtype == np.float32
    assert np.array_equal(d["obs_map"], a["obs_map"].numpy())
    assert np.array_equal(d["position"], a["position"].numpy())
    done = a["terminated"].numpy()
    assert np.array_equal(d["final_obs_map"][done], a["final_obs_map"].numpy()[done])
    assert not d["final_obs_map"][~done].any()


def test_large_batch_is_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 200_000)
    n = 500
    a = _arrays(n)
    bench.dump_outputs(str(tmp_path / "a"), a, n, valid=a["terminated"])
    bench.dump_outputs(str(tmp_path / "b"), a, n, valid=a["terminated"])
    d, e = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in d.values()) <= 200_000
    idx = d["env_index"].astype(np.int64)
    assert 1 <= len(idx) < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(d["obs_map"], a["obs_map"].numpy()[idx])
    assert np.array_equal(d["reward"], a["reward"].numpy()[idx])
    for k in d:
        assert np.array_equal(d[k], e[k]), k


def test_sharded_run_names_the_rank_and_splits_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 400_000)
    n = 500
    a = _arrays(n)
    bench.dump_outputs(str(tmp_path), a, n, env_offset=n, rank=1, world=2, valid=a["terminated"])
    files = sorted(os.listdir(tmp_path))
    assert files and all(f.endswith(".rank1.npy") for f in files)
    assert sum(np.load(tmp_path / f).nbytes for f in files) <= 200_000
    assert np.load(tmp_path / "env_index.rank1.npy").min() >= n
