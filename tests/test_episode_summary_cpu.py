"""The host side of the episode statistics, no GPU: VecInfos' lazy "episode" entry (pgtg_amd/sb3.py) and
the reduction of batch summaries over ranks (pgtg_amd/dist.py reduce_episode_summary; gloo, world size 2,
like tests/test_dist.py)."""
import ctypes as C
import os
import socket

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

from pgtg_amd import _abi
from pgtg_amd.dist import reduce_episode_summary
from pgtg_amd.sb3 import VecInfos

INT32_MAX = 2**31 - 1
EMPTY = {"episodes": 0, "truncated_only": 0, "length_sum": 0, "length_min": INT32_MAX, "length_max": 0,
         "return_sum": 0.0, "return_min": float("inf"), "return_max": float("-inf"),
         "return_mean": None, "length_mean": None}


def _summary(rank):
    n, ls, rs = 3 + rank, 40 + 10 * rank, -12.5 + 100.25 * rank
    return {"episodes": n, "truncated_only": 1 + rank, "length_sum": ls, "length_min": 4 - rank, "length_max": 20 + 5 * rank,
            "return_sum": rs, "return_min": -100.0 + rank, "return_max": 20.0 * (rank + 1),
            "return_mean": rs / n, "length_mean": ls / n}


def test_summary_struct_matches_the_header():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pgtg.h")).read()
    assert "#define PGTG_ABI_VERSION %d\n" % _abi.PGTG_ABI_VERSION in src
    assert C.sizeof(_abi.PgtgEpisodeSummary) == 48
    assert _abi.PgtgEpisodeSummary.return_sum.offset == 32 and _abi.PgtgEpisodeSummary.return_max.offset == 44


def test_vecinfos_builds_the_episode_entry_lazily():
    dones = np.array([0, 1, 0, 1], bool)
    trunc = np.array([0, 0, 0, 1], bool)
    final = np.arange(8, dtype=np.float32).reshape(4, 2)
    ep_r = np.array([0.5, -100.3, 1.0, 19.7], np.float32)
    ep_l = np.array([3, 7, 1, 100], np.int32)
    inf = VecInfos(dones, trunc, final, None, ep_return=ep_r, ep_length=ep_l, ep_time=1.25)
    assert inf._cache == {} and inf._all is None  # nothing built yet
    first = inf[3]
    assert set(first) == {"terminal_observation", "TimeLimit.truncated", "episode"}
    assert first["episode"] == {"r": ep_r[3], "l": 100, "t": 1.25}
    assert type(first["episode"]["r"]) is np.float32 and type(first["episode"]["l"]) is np.int32
    assert list(inf._cache) == [3]
    assert inf[0] == {} and inf[2] == {}  # unfinished envs carry no "episode"
    allv = list(inf[:])  # VecMonitor's read of every entry: the same objects as the single reads
    assert allv[3] is first and inf[3] is first and inf[1] is allv[1] and allv[0] is inf[0]
    assert allv[1]["episode"]["r"] == ep_r[1] and allv[1]["episode"]["l"] == 7
    # without the keyword arrays nothing changes
    assert set(VecInfos(dones, trunc, final, None)[1]) == {"terminal_observation", "TimeLimit.truncated"}


def test_reduce_is_the_identity_without_a_process_group():
    s = _summary(0)
    assert reduce_episode_summary(s) == s and reduce_episode_summary(s) is not s
    assert reduce_episode_summary(EMPTY) == EMPTY


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    both = reduce_episode_summary(_summary(rank))
    one = reduce_episode_summary(_summary(1) if rank == 1 else EMPTY)  # a rank without episodes
    none = reduce_episode_summary(EMPTY)
    q.put((rank, both, one, none))
    dist.destroy_process_group()


def test_two_ranks_under_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    a, b = _summary(0), _summary(1)
    want = {"episodes": 7, "truncated_only": 3, "length_sum": 90, "length_min": 3, "length_max": 25,
            "return_sum": a["return_sum"] + b["return_sum"], "return_min": -100.0, "return_max": 40.0}
    want["return_mean"], want["length_mean"] = want["return_sum"] / 7, 90 / 7
    for _, both, one, none in res:
        assert both == want
        assert one == b  # the empty rank's sentinels do not show
        assert none == EMPTY  # episodes == 0 everywhere: the sentinels
