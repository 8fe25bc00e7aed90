"""k_flatten's cost scalar (include/pgtg.h pgtg_set_flat_cost, PGTGVecEnv.set_flat_cost): binding the cost row
changes nothing else the kernel writes, and the row is (float)cost -- through PGTGVecEnv.flatten_now on chosen
cost, reward and finished flags, for float32 and int8 rows, on a full-map layout (rows of one pass) and a
sliding-window layout (rows written in passes), at one env, a wave and an env, a workgroup and an env."""
import warnings

import pytest
import torch

import helpers  # noqa: F401
from pgtg_amd.flat import flat_dim

pytestmark = pytest.mark.gpu

PAD = 16
LAYOUTS = {"full_map": dict(random_map_width=3, random_map_height=3),
           "sliding": dict(random_map_width=3, random_map_height=3, use_sliding_observation_window=True,
                           sliding_observation_window_size=8, use_next_subgoal_direction=True)}
ONE_PASS = 18 * 64  # values of a row k_flatten writes in one pass (kFlatU x 64)


def _vec(n, **kw):
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PGTGVecEnv(n, device=0, autoreset=True, **kw)


def _bufs(N, D, dtype):
    mk = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda")  # noqa: E731
    return dict(flat=mk((N, D), dtype, -3), fin=mk((N, D), dtype, -3), r32=mk((N,), torch.float32, -7.5),
                dn=mk((N,), torch.uint8, 0x5A).view(torch.bool), to=mk((N,), torch.uint8, 0x5A).view(torch.bool),
                cost=mk((N + 2 * PAD,), torch.float32, -7.5))


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("N", [1, 65, 257])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int8])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_the_cost_row_changes_nothing_else(layout, dtype, N):
    env = _vec(N, separate_reward_cost=True, standing_still_penalty=1, traffic_density=0.5, **LAYOUTS[layout])
    D = flat_dim(env.spec)
    assert (D <= ONE_PASS) == (layout == "full_map")  # (the two variants launch_flatten picks between)
    env.reset(seed=3)
    acts = env.random_actions(3, seed=5)
    for t in range(3):
        env.step_actions(acts[t])  # (observations, positions and terminal sets of a real step)
    # chosen scalars: costs that round in float32, -0.0, beyond float32's range; every way an env finishes
    g = torch.Generator().manual_seed(N)
    cost = torch.randn(N, generator=g, dtype=torch.float64).abs() * 1e3 + 1e-9
    special = torch.tensor([16777217.0, -0.0, 0.1, 1e39, 1e-30], dtype=torch.float64)[:N]
    cost[:len(special)] = special
    env.cost.copy_(cost.cuda())
    env.reward.copy_((torch.randn(N, generator=g, dtype=torch.float64) * 10).cuda())
    idx = torch.arange(N, device="cuda")
    env.terminated.copy_(idx % 3 == 1)
    env.truncated.copy_(idx % 4 == 1)
    want = cost.to(torch.float32).cuda()
    if N >= 65:
        assert bool((want.cpu().double() != cost).float().mean() > 0.9)

    plain, bound = _bufs(N, D, dtype), _bufs(N, D, dtype)
    env.set_flat_outputs(plain["flat"], plain["fin"])
    env.set_flat_scalars(plain["r32"], plain["dn"], plain["to"])
    env.flatten_now(2)
    env.set_flat_outputs(bound["flat"], bound["fin"])
    env.set_flat_scalars(bound["r32"], bound["dn"], bound["to"])
    row = bound["cost"][PAD:PAD + N]
    env.set_flat_cost(row)
    env.flatten_now(2)
    torch.cuda.synchronize()
    for k in ("flat", "fin", "r32", "dn", "to"):
        assert _same(plain[k], bound[k]), k
    assert bool((plain["cost"] == -7.5).all())
    assert torch.equal(row.view(torch.int32), want.view(torch.int32))
    assert bool((bound["cost"][:PAD] == -7.5).all()) and bool((bound["cost"][PAD + N:] == -7.5).all())
    assert torch.equal(bound["r32"].view(torch.int32), env.reward.to(torch.float32).view(torch.int32))
    assert torch.equal(bound["dn"], (env.terminated | env.truncated).to(torch.bool))
    # rebinding the three scalars keeps the cost row; the terminal pass alone does not write it
    env.set_flat_scalars(plain["r32"], plain["dn"], plain["to"])
    row.fill_(-7.5)
    env.flatten_now(1)
    assert bool((row == -7.5).all())
    env.flatten_now(0)
    assert torch.equal(row.view(torch.int32), want.view(torch.int32))
    # unbinding: by None, and with the scalars
    row.fill_(-7.5)
    env.set_flat_cost(None)
    env.flatten_now(2)
    assert bool((row == -7.5).all())
    env.set_flat_cost(row)
    env.set_flat_scalars(None, None, None)
    env.flatten_now(2)
    assert bool((row == -7.5).all())
    with pytest.raises(ValueError):
        env.set_flat_cost(row)  # (the scalars are gone)
    env.close()


def test_the_cost_row_is_refused_without_its_inputs():
    from pgtg_amd import _abi
    N = 5
    env = _vec(N, separate_reward_cost=True, random_map_width=3, random_map_height=3)
    b = _bufs(N, flat_dim(env.spec), torch.int8)
    row = b["cost"][:N]
    env.set_flat_outputs(b["flat"], b["fin"])
    with pytest.raises(ValueError, match="flat scalars"):
        env.set_flat_cost(row)  # before the flat scalars are bound
    env.set_flat_scalars(b["r32"], b["dn"], b["to"])
    for bad in (b["cost"], row.double(), row[::2]):
        with pytest.raises(ValueError):
            env.set_flat_cost(bad)
    env.set_flat_cost(row)
    env.reset(seed=1)  # (the bound row is written by the launch's own pass)
    torch.cuda.synchronize()
    assert torch.equal(row, env.cost.to(torch.float32))
    env.close()
    plain = _vec(N, random_map_width=3, random_map_height=3)  # no cost output
    assert plain.cost is None
    b = _bufs(N, flat_dim(plain.spec), torch.int8)
    plain.set_flat_outputs(b["flat"], b["fin"])
    plain.set_flat_scalars(b["r32"], b["dn"], b["to"])
    with pytest.raises(ValueError, match="separate_reward_cost"):
        plain.set_flat_cost(b["cost"][:N])
    assert plain._lib.pgtg_set_flat_cost(plain._h, None) == _abi.PGTG_OK  # (unbinding is always fine)
    plain.flatten_now(2)
    torch.cuda.synchronize()
    assert bool((b["cost"] == -7.5).all())
    plain.close()
