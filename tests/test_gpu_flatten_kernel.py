"""k_flatten alone (include/pgtg.h pgtg_flatten, PGTGVecEnv.flatten_now) against flatten_obs -- which
tests/test_flat.py pins to gymnasium's flatten -- on chosen inputs, at every row layout the kernel treats
differently (tests/flat_layouts.py; tests/test_flat_layout_classes.py proves the table reaches them) and
at every count of rows per workgroup and per wave its pipelined row loop distinguishes.

The envs are never stepped: the tests write the observation tensors, the scalars and the terminal set
directly and launch the kernel with a chosen mode and grid.  Observation bytes are a position code
1 + hash(env, channel, x, y) % 127 -- exact in int8 and float32, so a byte taken from another env, channel
or square shows -- or random 0/1; positions have x != y; the next-subgoal direction takes all of -1..7; the
velocities span the dtype's range; the terminal tensors differ from the live ones.  Every comparison is
torch.equal: both dtypes are exact.  The flat rows and the three scalar arrays are bound as the middle
[16 : 16 + N] of sentinel-filled tensors, and what a launch must not write -- the 16 rows before and after,
the terminal rows of unfinished envs, the other mode's destinations -- must still hold the sentinel."""
import warnings

import pytest
import torch

import helpers  # noqa: F401
from flat_layouts import DTYPES, LAYOUTS, classify, layout_spec
from pgtg_amd.flat import flat_dim, flatten_obs

pytestmark = pytest.mark.gpu

PAD = 16  # rows (elements) of sentinel before and after: 16 rows keep the 16-byte alignment for every D and dtype
TORCH_DT = {"float32": torch.float32, "int8": torch.int8}
SENT = {torch.float32: -7.5, torch.int8: -91}  # (no float row value is fractional)
SENT_U8 = 0x5A
KINDS = ("code", "bits")


def _code(N, C, W, salt):
    """uint8 [N, C, W, W]: 1 + hash(env, channel, x, y) % 127."""
    ar = lambda n, shape: torch.arange(n, dtype=torch.int64, device="cuda").view(shape)  # noqa: E731
    a = ar(N, (N, 1, 1, 1)) * 32768 + ar(C, (1, C, 1, 1)) * 256 + ar(W, (1, 1, W, 1)) * 16 + ar(W, (1, 1, 1, W)) + salt
    h = ((a * 2654435761) & 0xFFFFFFFF) >> 12
    return (1 + h % 127).to(torch.uint8)


class Inputs:
    """What the kernel reads, for N envs (env e's values depend on e only, so [:n] serves a smaller batch),
    and the rows flatten_obs makes of it, computed once."""

    def __init__(self, spec, N, dtype):
        g = torch.Generator().manual_seed(1000 + N)
        C, W = len(spec.channels), spec.window
        keys = [k for k, _ in spec.channels]
        ri = lambda lo, hi, shape, dt=torch.int32: torch.randint(lo, hi, shape, generator=g, dtype=torch.int64).to(dt).cuda()  # noqa: E731
        self.obs = {"code": _code(N, C, W, 0x51ED27), "bits": ri(0, 2, (N, C, W, W), torch.uint8)}
        self.fobs = {"code": _code(N, C, W, 0x2B992D), "bits": ri(0, 2, (N, C, W, W), torch.uint8)}
        self.pos, self.fpos = ri(0, 9, (N, 2)), ri(0, 9, (N, 2))  # x and y drawn independently
        if dtype == torch.int8:
            self.vel, self.fvel = ri(-128, 128, (N, 2)), ri(-128, 128, (N, 2))
            edge = [[-128, 127], [127, -128], [0, -1]]
        else:
            self.vel, self.fvel = ri(-(1 << 24), (1 << 24) + 1, (N, 2)), ri(-(1 << 24), (1 << 24) + 1, (N, 2))
            edge = [[1 << 24, -(1 << 24)], [-(1 << 24), 0], [0, 1 << 24]]
        e = torch.tensor(edge, dtype=torch.int32, device="cuda")[:N]
        self.vel[:len(e)] = e
        self.fvel[:len(e)] = e.flip(1)
        idx = torch.arange(N, device="cuda")
        self.nsd = ((idx * 5 + 3) % 9 - 1).to(torch.int32) if spec.next_subgoal else None
        self.fnsd = ((idx * 7 + 1) % 9 - 1).to(torch.int32) if spec.next_subgoal else None
        # rewards that round in float32, -0.0, magnitudes up to and past float32's range
        rew = torch.randn(N, generator=g, dtype=torch.float64) * 1e3 + 1e-9
        special = torch.tensor([-0.0, 0.1, 1 / 3, 16777217.0, -16777219.0, 3.0e38, -1e39, 1e-30, 123456789.123456789],
                               dtype=torch.float64)[:N]
        rew[:len(special)] = special
        self.want_r32 = rew.to(torch.float32).cuda()  # (rounded on the host)
        self.rew = rew.cuda()
        if N >= 64:
            assert bool((self.pos[:, 0] != self.pos[:, 1]).float().mean() > 0.7)
            assert bool((self.want_r32.cpu().double() != rew).float().mean() > 0.9)
            assert self.nsd is None or sorted(set(self.nsd.tolist())) == list(range(-1, 8))

        def rows(m, pos, vel, nsd):
            o = {"map": {k: m[:, i] for i, k in enumerate(keys)}, "position": pos, "velocity": vel}
            if nsd is not None:
                o["next_subgoal_direction"] = nsd
            return flatten_obs(spec, o, dtype=dtype)
        self.want = {k: rows(self.obs[k], self.pos, self.vel, self.nsd) for k in KINDS}
        self.want_fin = {k: rows(self.fobs[k], self.fpos, self.fvel, self.fnsd) for k in KINDS}


class Bufs:
    """The kernel's destinations: [PAD + N + PAD] sentinel-filled tensors, the middle N bound."""

    def __init__(self, N, D, dtype, final, scalars):
        self.N, self.sent = N, SENT[dtype]
        mk = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device="cuda")  # noqa: E731
        self.flat = mk((N + 2 * PAD, D), dtype, self.sent)
        self.fin = mk((N + 2 * PAD, D), dtype, self.sent) if final else None
        self.r32 = mk((N + 2 * PAD,), torch.float32, -7.5) if scalars else None
        self.dn = mk((N + 2 * PAD,), torch.uint8, SENT_U8) if scalars else None
        self.to = mk((N + 2 * PAD,), torch.uint8, SENT_U8) if scalars else None

    def all(self):
        return [t for t in (self.flat, self.fin, self.r32, self.dn, self.to) if t is not None]

    def clear(self):
        for t, v in zip((self.flat, self.fin, self.r32, self.dn, self.to), (self.sent, self.sent, -7.5, SENT_U8, SENT_U8)):
            if t is not None:
                t.fill_(v)

    def mid(self, t):
        return t[PAD:PAD + self.N]

    def untouched(self, t, rows=None):
        """The pads of t hold the sentinel, and so do the bound rows `rows` (bool [N]; None: no bound row checked)."""
        v = {id(self.flat): self.sent, id(self.fin): self.sent, id(self.r32): -7.5}.get(id(t), SENT_U8)
        ok = bool((t[:PAD] == v).all()) and bool((t[PAD + self.N:] == v).all())
        if rows is not None:
            ok = ok and bool((self.mid(t)[rows] == v).all())
        return ok


class Rig:
    """An env of N never-stepped envs with sentinel-padded flat buffers bound."""

    def __init__(self, spec, N, dtype, final=True, scalars=True, **kw):
        from pgtg_amd.vector import PGTGVecEnv
        self.spec, self.N, self.dtype = spec, N, dtype
        self.D = flat_dim(spec)
        self.env = PGTGVecEnv(N, spec=spec, device=0, autoreset=True, **kw)
        self.final, self.scalars = final, scalars
        self.b = self.bind(self.bufs())
        self.every = torch.ones(N, dtype=torch.bool, device="cuda")

    def bufs(self):
        return Bufs(self.N, self.D, self.dtype, self.final, self.scalars)

    def bind(self, b):
        self.env.set_flat_outputs(b.mid(b.flat), None if b.fin is None else b.mid(b.fin))
        if b.r32 is not None:
            self.env.set_flat_scalars(b.mid(b.r32), b.mid(b.dn).view(torch.bool), b.mid(b.to).view(torch.bool))
        self.b = b
        return b

    def load(self, inp, kind, finished):
        """The first N envs of `inp` into the env's tensors; `finished` (bool [N]) in the three ways an env
        finishes (terminated, truncated, both), the others with neither flag."""
        e, N = self.env, self.N
        e.obs_map.copy_(inp.obs[kind][:N])
        e.final_map.copy_(inp.fobs[kind][:N])
        for dst, src in ((e.position, inp.pos), (e.final_position, inp.fpos), (e.velocity, inp.vel),
                         (e.final_velocity, inp.fvel), (e.nsd, inp.nsd), (e.final_nsd, inp.fnsd), (e.reward, inp.rew)):
            if dst is not None:
                dst.copy_(src[:N])
        way = torch.arange(N, device="cuda") % 3
        e.terminated.copy_(finished & (way != 1))
        e.truncated.copy_(finished & (way != 0))
        self.inp, self.kind, self.finished = inp, kind, finished

    def run(self, mode, grid, ctx=()):
        """Clear the destinations, launch, and check everything the launch must and must not have written."""
        b, N, inp, kind, fin = self.b, self.N, self.inp, self.kind, self.finished
        ctx = (mode, grid, kind) + tuple(ctx)
        b.clear()
        self.env.flatten_now(mode, grid)
        if mode != 1:
            assert b.untouched(b.flat), ctx
            assert torch.equal(b.mid(b.flat), inp.want[kind][:N]), ctx
            if b.r32 is not None:
                assert b.untouched(b.r32) and b.untouched(b.dn) and b.untouched(b.to), ctx
                # (bit patterns: the sign of -0.0 counts)
                assert torch.equal(b.mid(b.r32).view(torch.int32), inp.want_r32[:N].view(torch.int32)), ctx
                e = self.env
                assert torch.equal(b.mid(b.dn), (e.terminated | e.truncated).to(torch.uint8)), ctx
                assert torch.equal(b.mid(b.to), (e.truncated & ~e.terminated).to(torch.uint8)), ctx
        else:  # the terminal pass leaves the observation rows and the scalars alone
            assert b.untouched(b.flat, self.every), ctx
            if b.r32 is not None:
                assert b.untouched(b.r32, self.every) and b.untouched(b.dn, self.every) and b.untouched(b.to, self.every), ctx
        if b.fin is not None:
            if mode != 0:
                assert b.untouched(b.fin, ~fin), ctx  # the unfinished envs' terminal rows too
                assert torch.equal(b.mid(b.fin)[fin], inp.want_fin[kind][:N][fin]), ctx
            else:
                assert b.untouched(b.fin, self.every), ctx

    def close(self):
        self.env.close()


def _masks(N):
    """Finished-env patterns: none, all, alternating, a random 30 %, only the first, only the last."""
    idx = torch.arange(N, device="cuda")
    g = torch.Generator().manual_seed(N)
    return {"none": idx < 0, "all": idx >= 0, "alternating": idx % 2 == 1,
            "random30": (torch.rand(N, generator=g) < 0.3).cuda(), "first": idx == 0, "last": idx == N - 1}


def _min_grid(N):
    return (N + 255) // 256


# -- every layout ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_layout(dtype, name):
    """One layout, 37 envs: the production grid (a row per workgroup), one workgroup (37 rows and as many
    terminal rows on its four waves: the pipelined loop) and three (13 + 13 + 11), both kinds of bytes,
    modes 2, 0 and 1."""
    lay = LAYOUTS[name]
    spec = layout_spec(lay)
    assert classify(lay.n, lay.w, lay.nsd, dtype).D == flat_dim(spec)
    N = 37
    rig = Rig(spec, N, TORCH_DT[dtype])
    inp = Inputs(spec, N, TORCH_DT[dtype])
    fin = _masks(N)["random30"]
    fin[0] = fin[N - 1] = True
    for kind in KINDS:
        rig.load(inp, kind, fin)
        for grid in (0, 1, 3):
            rig.run(2, grid)
    rig.run(0, 1)
    rig.run(1, 1)
    rig.load(inp, "code", _masks(N)["all"])
    rig.run(2, 1)
    rig.close()


# -- every row count ---------------------------------------------------------------------------------

# a float single-store, a float pair, an int8 and a several-pass variant
SWEEP = [("ob0_nsd", "float32", "one"), ("ob1_nsd", "float32", "pair"), ("ob3", "int8", "one"), ("first_multi", "float32", "multi")]
_CACHE = {}


def _case(case):
    """(spec, torch dtype, Inputs for 700 envs) of a sweep case, made once."""
    if case not in _CACHE:
        name, dtype, variant = case
        lay = LAYOUTS[name]
        assert classify(lay.n, lay.w, lay.nsd, dtype).variant == variant
        spec = layout_spec(lay)
        _CACHE[case] = (spec, TORCH_DT[dtype], Inputs(spec, 700, TORCH_DT[dtype]))
    return _CACHE[case]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "-".join(c))
def test_rows_per_workgroup_1_to_24(case):
    """One workgroup over K = 1..24 envs: with the finished envs' terminal rows its four waves take every
    row count from 0 to 12 each -- the peeled first row alone, every exit of the two-row loop, the re-read
    of the last row -- for every mix of the two row kinds in the list."""
    spec, dtype, inp = _case(case)
    for K in range(1, 25):
        rig = Rig(spec, K, dtype)
        for pat, fin in _masks(K).items():
            rig.load(inp, "code", fin)
            rig.run(2, 1, (K, pat))
        rig.run(1, 1, (K, "last"))
        rig.load(inp, "bits", _masks(K)["random30"])
        rig.run(2, 1, (K, "random30"))
        rig.run(0, 1, (K, "random30"))
        rig.close()


@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "-".join(c))
def test_batch_sizes_around_a_workgroup(case, N):
    """N = 1 and N on both sides of the 256 rows a workgroup lists, with the production grid and with the
    smallest legal one (255 and 256: one workgroup of K = N; 257: two of K = 129, the second partial)."""
    spec, dtype, inp = _case(case)
    rig = Rig(spec, N, dtype)
    for pat in ("random30", "all"):
        rig.load(inp, "code", _masks(N)[pat])
        for grid in (0, _min_grid(N)):
            rig.run(2, grid, (N, pat))
    rig.run(1, _min_grid(N), (N, "all"))
    rig.close()


@pytest.mark.parametrize("N,grid,pats", [
    (512, 2, ("all",)),                # K = 256, every env finished: both workgroups' row lists full (512 entries)
    (700, 3, ("random30", "all")),     # K = 234, the last workgroup partial (232 envs)
    (10, 8, ("alternating", "all")),   # K = 2: workgroups 5..7 have no rows at all
])
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "-".join(c))
def test_chosen_grids(case, N, grid, pats):
    spec, dtype, inp = _case(case)
    rig = Rig(spec, N, dtype)
    for pat in pats:
        for kind in KINDS:
            rig.load(inp, kind, _masks(N)[pat])
            rig.run(2, grid, (N, pat))
    rig.run(0, grid, (N, pats[-1]))
    rig.run(1, grid, (N, pats[-1]))
    rig.close()


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "-".join(c))
def test_mode_2_is_mode_0_then_mode_1(case):
    """Both row sets in one launch (what a step does) against the two passes on a second set of buffers:
    the same bytes everywhere, pads included."""
    spec, dtype, inp = _case(case)
    N = 300
    rig = Rig(spec, N, dtype)
    first = rig.b
    rig.load(inp, "code", _masks(N)["random30"])
    rig.run(2, 2)
    second = rig.bind(rig.bufs())
    rig.run(0, 2)
    keep = second.flat.clone()
    rig.env.flatten_now(1, 2)  # (run() would clear the observation rows first)
    torch.cuda.synchronize()
    assert torch.equal(second.flat, keep)
    for a, b in zip(first.all(), second.all()):
        assert torch.equal(a, b)
    rig.close()


# -- refusals ----------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    """A grid that would give a workgroup more than 256 rows, a grid above N, a mode outside 0..2 and a
    mode whose rows are not bound raise ValueError and write nothing."""
    lay = LAYOUTS["ob1"]
    spec = layout_spec(lay)
    N = 600
    inp = Inputs(spec, N, torch.float32)
    rig = Rig(spec, N, torch.float32)
    rig.load(inp, "code", _masks(N)["all"])
    assert _min_grid(N) == 3
    for mode, grid in ((0, 2), (2, 2), (1, 1), (0, N + 1), (2, N + 1), (0, -1), (3, 0), (-1, 0)):
        with pytest.raises(ValueError):
            rig.env.flatten_now(mode, grid)
    torch.cuda.synchronize()
    for t in rig.b.all():
        assert rig.b.untouched(t, rig.every)
    rig.run(2, 3)  # (the smallest legal grid, and the largest: a row per workgroup)
    rig.run(2, N)
    rig.close()
    # no terminal rows bound: modes 1 and 2 are refused, mode 0 runs
    rig = Rig(spec, N, torch.float32, final=False)
    rig.load(inp, "code", _masks(N)["all"])
    for mode in (1, 2):
        with pytest.raises(ValueError):
            rig.env.flatten_now(mode, 0)
    torch.cuda.synchronize()
    for t in rig.b.all():
        assert rig.b.untouched(t, rig.every)
    rig.run(0, 0)
    # no observation rows bound: modes 0 and 2 are refused
    b = rig.b
    b.clear()
    rig.env.set_flat_outputs(None, None)
    for mode in (0, 1, 2):
        with pytest.raises(ValueError):
            rig.env.flatten_now(mode, 0)
    torch.cuda.synchronize()
    for t in b.all():
        assert b.untouched(t, rig.every)
    rig.close()


# -- the production grid -----------------------------------------------------------------------------

def test_step_path_with_many_rows_per_workgroup():
    """The grid launch_flatten picks itself, at a batch where it gives every workgroup K >= 9 rows: a CU
    holds at most 32 waves, 8 workgroups of 256 lanes, so the grid is at most 8 x CUs workgroups whatever
    the occupancy query answers, and N >= 72 x CUs gives K = ceil(N / G) >= 9 -- the pipelined loop
    iterates behind real steps.  The D = 29 rows (one channel, a 3 x 3 sliding window) keep the buffers at
    a few MB.  max_episode_steps=2: the second step finishes every env (every workgroup's list holds 2 K
    rows), the others a few."""
    from pgtg_amd.vector import PGTGVecEnv
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = max(40000, 72 * cus)
    assert N >= 72 * cus
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from pgtg_amd.config import make_spec
        spec = make_spec(random_map_width=3, random_map_height=3, use_sliding_observation_window=True,
                         sliding_observation_window_size=1, features_to_include_in_observation=["walls"])
    D = flat_dim(spec)
    assert D == LAYOUTS["smallest"].D
    for dtype in (torch.float32, torch.int8):
        env = PGTGVecEnv(N, spec=spec, device=0, autoreset=True, max_episode_steps=2)
        b = Bufs(N, D, dtype, True, True)
        env.set_flat_outputs(b.mid(b.flat), b.mid(b.fin))
        env.set_flat_scalars(b.mid(b.r32), b.mid(b.dn).view(torch.bool), b.mid(b.to).view(torch.bool))
        env.reset(seed=23)
        assert torch.equal(b.mid(b.flat), flatten_obs(spec, env.observation(), dtype=dtype))
        assert b.untouched(b.flat) and b.untouched(b.fin, torch.ones(N, dtype=torch.bool, device="cuda"))
        g = torch.Generator(device="cuda").manual_seed(5)
        finished = []
        for t in range(3):
            b.fin.fill_(b.sent)
            env.step(torch.randint(0, 9, (N,), device="cuda", dtype=torch.uint8, generator=g))
            assert torch.equal(b.mid(b.flat), flatten_obs(spec, env.observation(), dtype=dtype)), t
            done = env.terminated | env.truncated
            assert torch.equal(b.mid(b.r32), env.reward.to(torch.float32)), t
            assert torch.equal(b.mid(b.dn), done.to(torch.uint8)), t
            assert torch.equal(b.mid(b.to), (env.truncated & ~env.terminated).to(torch.uint8)), t
            want = flatten_obs(spec, env.final_observation(), dtype=dtype)
            assert torch.equal(b.mid(b.fin)[done], want[done]), t
            assert b.untouched(b.fin, ~done), t
            for x in (b.flat, b.r32, b.dn, b.to):
                assert b.untouched(x), t
            finished.append(int(done.sum()))
        assert finished[1] >= N - finished[0] and finished[1] > N // 2  # (TimeLimit: every env not just reset)
        env.close()
