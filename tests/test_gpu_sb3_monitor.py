"""PGTGSB3VecEnv(monitor=True): SB3's VecMonitor (pgtg/train.py:55) inside the adapter.  A finished
env's info carries "episode": {"r", "l", "t"} from the device accumulators (k_episode), on the host path
and on the device path, against a numpy restatement of VecMonitor fed with the step's rewards and dones."""
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401

pytestmark = pytest.mark.gpu

KW = dict(random_map_width=3, random_map_height=3, standing_still_penalty=0.3)
N, L, T = 8, 6, 20


def _env(**kw):
    from pgtg_amd.sb3 import PGTGSB3VecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PGTGSB3VecEnv(N, max_episode_steps=L, seed=70, **KW, **kw)


def _actions():
    rng = np.random.default_rng(9)
    return [np.where(rng.random(N) < 0.6, 4, rng.integers(0, 9, N)) for _ in range(T)]


def test_monitor_infos_on_the_host_and_device_paths():
    host, dev = _env(monitor=True), _env(monitor=True, device_obs=True)
    host.reset()
    dev.reset()
    ret, ln = np.zeros(N, np.float32), np.zeros(N, np.int32)
    last_t = {"host": 0.0, "dev": 0.0}
    finished = inexact = 0
    ret64 = np.zeros(N)
    for a in _actions():
        _, rew, dones, inf_h = host.step(a)
        _, rew_d, dones_d, inf_d = dev.step(torch.as_tensor(a, device="cuda"))
        assert np.array_equal(rew, rew_d.cpu().numpy()) and np.array_equal(dones, dones_d.cpu().numpy())
        ret = ret + rew.astype(np.float32)
        ln = ln + np.int32(1)
        ret64 += rew.astype(np.float64)
        inexact += int((ret.astype(np.float64) != ret64).sum())
        # the device path's batch tensors: every env's running values, fresh for this step
        assert inf_d.episode_return.is_cuda and inf_d.episode_return.dtype == torch.float32
        assert inf_d.episode_length.dtype == torch.int32
        assert np.array_equal(inf_d.episode_return.cpu().numpy().view(np.uint32), ret.view(np.uint32))
        assert np.array_equal(inf_d.episode_length.cpu().numpy(), ln)
        for i in range(N):
            for name, inf in (("host", inf_h), ("dev", inf_d)):
                if not dones[i]:
                    assert "episode" not in inf[i] and inf[i] == {}
                    continue
                ep = inf[i]["episode"]
                assert set(ep) == {"r", "l", "t"}
                assert type(ep["r"]) is np.float32 and type(ep["l"]) is np.int32 and type(ep["t"]) is float
                assert ep["r"] == ret[i] and ep["l"] == ln[i], (name, i, ep, ret[i], ln[i])
                assert ep["t"] >= last_t[name]
                last_t[name] = ep["t"]
            if dones[i]:
                assert inf_h[i]["episode"]["r"] == inf_d[i]["episode"]["r"] and inf_h[i]["episode"]["l"] == inf_d[i]["episode"]["l"]
                assert inf_h[i]["TimeLimit.truncated"] == inf_d[i]["TimeLimit.truncated"]
                finished += 1
        ret[dones] = 0
        ln[dones] = 0
        ret64[dones] = 0
    assert finished > 0 and inexact > 0
    sh, sd = host.episode_summary(), dev.episode_summary()
    assert sh == sd and sh["episodes"] == finished
    assert host.episode_summary()["episodes"] == 0
    host.close()
    dev.close()


def test_without_monitor_the_infos_are_what_they_were():
    host, dev = _env(), _env(device_obs=True)
    host.reset()
    dev.reset()
    finished = 0
    for a in _actions():
        _, _, dones, inf_h = host.step(a)
        _, _, _, inf_d = dev.step(torch.as_tensor(a, device="cuda"))
        assert inf_d.episode_return is None and inf_d.episode_length is None
        for i in range(N):
            for inf in (inf_h, inf_d):
                assert set(inf[i]) == ({"terminal_observation", "TimeLimit.truncated"} if dones[i] else set())
            finished += int(dones[i])
    assert finished > 0
    with pytest.raises(ValueError):
        host.episode_summary()  # statistics were never bound
    host.close()
    dev.close()
