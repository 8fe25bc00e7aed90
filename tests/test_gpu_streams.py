"""Stream ordering: every entry point on a gated side stream against the same calls on the default stream.

The library says its work is ordered with the caller's current stream and that collect() / update() do not
synchronise with the host; on the default stream neither claim can fail.  Here run A (default stream) is the
reference -- the rest of the suite pins it to the oracle and to the float64 references -- and run B makes the
same calls on a non-blocking side stream held shut by tests/stream_gate.py, with every external input staged
through the gate: a launch on another stream, or one that does not wait for the side stream, sees sentinels or
stale state, and B's outputs differ.  Both handles go through every chain twice: the first pass (B ungated on
the side stream) absorbs first-use work and gives the hold its yardstick, the second is gated.  DESIGN.md 5v
lists what the gate cannot show (null-stream memsets, audited by reading) and one run's figures."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
from stream_gate import SENTINELS, StreamGate
from test_gpu_state import _sections

pytestmark = pytest.mark.gpu

# the training caller's settings (test_gpu_ppo.py's TRAIN), with the cost channel
TRAIN = dict(random_map_width=4, random_map_height=4, random_map_obstacle_probability=0.2,
             random_map_percentage_of_connections=0.8, traffic_density=0.2, conservative_driver_percentage=0.15,
             normal_driver_percentage=0.50, aggressive_driver_percentage=0.20, elderly_driver_percentage=0.10,
             reckless_driver_percentage=0.05, sliding_observation_window_size=5, max_allowed_deviation=15,
             use_sliding_observation_window=True, use_next_subgoal_direction=True, final_goal_bonus=200,
             standing_still_penalty=1, separate_reward_cost=True)
TRAFFIC3 = dict(random_map_width=3, random_map_height=3, traffic_density=0.3, separate_reward_cost=True)
PLAIN3 = dict(random_map_width=3, random_map_height=3)
PLAIN5 = dict(random_map_width=5, random_map_height=5, separate_reward_cost=True)
BIG = dict(random_map_width=12, random_map_height=10, separate_reward_cost=True)
N_SMALL = 96

_GATE = None


def gate() -> StreamGate:
    global _GATE
    if _GATE is None:
        _GATE = StreamGate(0)
        _GATE.calibrate()
    return _GATE


def _vec(n, conf, **kw):
    from pgtg_amd.config import make_spec
    from pgtg_amd.vector import PGTGVecEnv
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PGTGVecEnv(n, spec=make_spec(**conf), device=0, **kw)


def _actions(n, steps, seed):
    """[steps, n] uint8 device actions in Discrete(9), resident before any gate is shut."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 9, (steps, n), generator=g, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return a


def _sentinel(like, value):
    t = torch.full_like(like, value)
    torch.cuda.synchronize()
    return t


def _same_tensors(xs, ys, tag, names=None):
    torch.cuda.synchronize()
    assert len(xs) == len(ys), tag
    for k, (x, y) in enumerate(zip(xs, ys)):
        name = names[k] if names else f"output {k}"
        assert x.shape == y.shape and x.dtype == y.dtype, f"{tag}: {name}"
        same = torch.equal(x, y) if not x.dtype.is_floating_point else torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        assert same, f"{tag}: {name} differs at {torch.nonzero(x != y)[:4].tolist()}"


def _same_outputs(a, b, tag):
    _same_tensors(a._bound_tensors(), b._bound_tensors(), tag)


def _same_dict(x, y, tag):
    assert x.keys() == y.keys(), tag
    for k in x:
        u, v = x[k], y[k]
        if isinstance(u, float) and u != u:
            assert v != v, f"{tag}: {k}: {u} != {v}"
        elif isinstance(u, np.ndarray):
            assert np.array_equal(u, v), f"{tag}: {k}"
        else:
            assert u == v, f"{tag}: {k}: {u} != {v}"


def _same_host(a, b, tag, stats=True):
    assert a.error_count() == b.error_count(), (tag, a.error_count(), b.error_count())
    assert a.counters() == b.counters(), (tag, a.counters(), b.counters())
    assert a.queue_maps() == b.queue_maps(), (tag, a.queue_maps(), b.queue_maps())
    if stats:
        _same_dict(a.episode_summary(False), b.episode_summary(False), tag)


def _close(*things):
    torch.cuda.synchronize()
    for t in things:
        t.close()


# -- the controls: the gate detects what it is for ---------------------------------------------------------------
@pytest.mark.timeout(60)
def test_control_side_stream_is_unordered_with_the_null_stream():
    """With the gate shut a clone of a staged tensor on the default stream sees the sentinel, the same clone on
    the side stream the real values: the side stream is not ordered with the null stream and the spin holds."""
    G = gate()
    real = _actions(N_SMALL, 1, 1)[0]
    staged = _sentinel(real, SENTINELS["actions"])
    g = G.shut("control clone", 0.0)
    g.stage(staged, real)
    on_default = staged.clone()
    torch.cuda.current_stream().synchronize()  # (the null stream alone)
    with g.stream():
        on_side = staged.clone()
    assert g.still_shut(), "the spin ended before the default-stream clone had run"
    assert bool((on_default == SENTINELS["actions"]).all()), "the default stream waited for the side stream"
    g.open()
    assert torch.equal(on_side, real)


@pytest.mark.timeout(60)
def test_control_a_misbound_launch_is_detected():
    """The handle bound to the null stream on purpose (the C ABI, behind the binding's back) while the actions are
    staged on the side stream: the step runs at once, reads the sentinel -- the invalid action 255, an ordinary
    per-env error -- and error_count() reports all N envs; the outputs differ from the reference's."""
    from pgtg_amd import _abi
    G = gate()
    a, b = _vec(N_SMALL, TRAFFIC3), _vec(N_SMALL, TRAFFIC3)
    try:
        acts = _actions(N_SMALL, 2, 2)
        a.reset(seed=5)
        a.step_actions(acts[0])
        a.step_actions(acts[1])
        with G.on_side():
            b.reset(seed=5)
            host_s = G.warm("control misbound", lambda: b.step_actions(acts[0]))
        staged = _sentinel(acts[1], SENTINELS["actions"])
        g = G.shut("control misbound", host_s)
        g.stage(staged, acts[1])
        with g.stream():
            assert b._lib.pgtg_set_stream(b._h, None) == 0  # (b._stream still names the side stream: no rebinding)
            b.step_actions(staged)
            n, code = b.error_count()  # (drains the null stream the handle is bound to, not the side stream)
            shut = g.still_shut()
            assert b._lib.pgtg_set_stream(b._h, C.c_void_p(G.side.cuda_stream)) == 0
        g.open()
        assert shut, "the mis-bound step waited for the gate"
        assert (n, code) == (N_SMALL, _abi.PGTG_E_INVALID), (n, code)
        torch.cuda.synchronize()
        assert not torch.equal(a.position, b.position) or not torch.equal(a.obs_map, b.obs_map)
    finally:
        _close(a, b)


# -- a. resets -----------------------------------------------------------------------------------------------------
def _reset_forms(n):
    rng = np.random.default_rng(12)
    return dict(seeds=rng.integers(1, 1 << 40, n).astype(np.uint64), other=rng.integers(1 << 41, 1 << 42, n).astype(np.uint64),
                mask=torch.as_tensor((rng.random(n) < 0.4).astype(np.uint8)).cuda())


def _c_reset(env, seeds_np, mask):
    """pgtg_reset through the C ABI with a ctypes array over seeds_np (kept alive by the caller)."""
    from pgtg_amd.vector import _check
    arr = (C.c_uint64 * len(seeds_np)).from_buffer(seeds_np)
    env._bind_stream()
    _check(env._lib.pgtg_reset(env._h, C.cast(arr, C.c_void_p), 0, None if mask is None else C.c_void_p(mask.data_ptr())), env._h)
    env._seeded = True


def _run_resets(env, f, form, mask, clobber=None):
    if form == "int":
        env.reset(seed=31)
    elif form == "list":
        _c_reset(env, f["live"], None)
    elif form == "masked list":
        _c_reset(env, f["live"], mask)
    elif form == "masked int":
        env.reset(seed=47, mask=mask)
    elif form == "unseeded":
        env.reset()
    elif form == "masked unseeded":
        env.reset(mask=mask)
    if clobber is not None and "list" in form:
        f["live"][:] = clobber  # (overwritten, never freed: a late read gives other seeds and nothing worse)


FORMS = ("int", "list", "masked list", "masked int", "unseeded", "masked unseeded")


def _reset_case(n, conf, forms, sample):
    G = gate()
    a, b = _vec(n, conf), _vec(n, conf)
    try:
        f = _reset_forms(n)
        fa = dict(f, live=f["seeds"].copy())
        fb = dict(f, live=f["seeds"].copy())
        torch.cuda.synchronize()
        want_seed, holds = None, {}
        for gated in (False, True):
            for form in forms:
                _run_resets(a, fa, form, f["mask"])
                fb["live"][:] = f["seeds"]
                if not gated:
                    host_s = G.warm(f"reset {form} n={n}", lambda: _run_resets(b, fb, form, f["mask"]))
                    holds[form] = host_s
                else:
                    staged = _sentinel(f["mask"], SENTINELS["mask"])
                    g = G.shut(f"reset {form} n={n}", holds[form])
                    g.stage(staged, f["mask"])
                    with g.stream():
                        _run_resets(b, fb, form, staged, clobber=f["other"])
                        shut = g.still_shut()
                    g.open()
                    assert shut, f"reset {form}: the call waited for the device or outlasted the hold"
                tag = f"reset {form} n={n} {'gated' if gated else 'warm'}"
                _same_outputs(a, b, tag)
                mask = f["mask"].cpu().numpy() != 0
                if form == "list":
                    want_seed = f["seeds"].copy()
                elif form == "masked list":
                    want_seed = np.where(mask, f["seeds"], want_seed)
                for i in sample:
                    sa, sb = a.env_state(i), b.env_state(i)
                    assert sa == sb, (tag, i, sa, sb)
                    if "list" in form:
                        assert sb["seed"] == int(want_seed[i]), (tag, i, sb["seed"], int(want_seed[i]), int(f["other"][i]))
        _same_host(a, b, f"resets n={n}", stats=False)
    finally:
        _close(a, b)


@pytest.mark.timeout(120)
def test_resets_every_form():
    _reset_case(N_SMALL, dict(TRAFFIC3), FORMS, range(N_SMALL))


@pytest.mark.timeout(180)
def test_reset_seed_list_of_8_mb():
    """1 048 576 envs: the seed list is 8 MB, where the runtime may copy by another path than for 768 bytes."""
    n = 1 << 20
    _reset_case(n, dict(PLAIN3), ("list", "masked list"), (0, 1, 4097, n // 2 + 3, n - 1))


# -- b. every step-kernel path ------------------------------------------------------------------------------------
STEP_CASES = {
    "k_env+traffic": (N_SMALL, TRAFFIC3, None, lambda k: k == "pgtg::k_env<true, false> + pgtg::k_traffic"),
    "k_envb": (4096, PLAIN5, None, lambda k: k == "pgtg::k_envb<false>"),
    "k_envq": (4096, PLAIN5, dict(queue_mode=1), lambda k: k == "pgtg::k_envq<false>"),
    # (the BIG instance of whichever family the batch picks)
    "big": (64, BIG, None, lambda k: k in ("pgtg::k_envb<true>", "pgtg::k_envq<true>", "pgtg::k_env<false, true>")),
}


def _bind_everything(env):
    from pgtg_amd.flat import flat_dim
    n, D = env.num_envs, flat_dim(env.spec)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=env.device)  # noqa: E731
    env.set_flat_outputs(z((n, D), torch.int8), z((n, D), torch.int8))
    env.set_flat_scalars(z(n, torch.float32), z(n, torch.bool), z(n, torch.bool))
    env.set_flat_cost(z(n, torch.float32))
    env.enable_episode_stats()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_steps_on_every_kernel_path(case):
    G = gate()
    n, conf, tune, named = STEP_CASES[case]
    a, b = (_vec(n, conf, autoreset=True, max_episode_steps=3, tune=tune) for _ in range(2))
    try:
        print(f"stream-gate steps {case}: {a.step_kernel()} {a.launch_info()}")
        assert named(a.step_kernel()) and b.step_kernel() == a.step_kernel(), a.step_kernel()
        for e in (a, b):
            _bind_everything(e)
        acts = _actions(n, 12, 3)
        a.reset(seed=21)
        b.reset(seed=21)  # (on the default stream: the steps are the first calls that have to bind the side stream)
        _same_outputs(a, b, f"{case}: reset")

        def six(env, t0):
            for t in range(t0, t0 + 6):
                env.step_actions(acts[t])

        six(a, 0)
        host_s = G.warm(f"steps {case}", lambda: six(b, 0))
        _same_outputs(a, b, f"{case}: warm steps")
        _same_host(a, b, f"{case}: warm steps")
        for t in range(6, 12):
            a.step_actions(acts[t])
            staged = _sentinel(acts[t], SENTINELS["actions"])
            g = G.shut(f"steps {case} t={t}", host_s)
            g.stage(staged, acts[t])
            with g.stream():
                b.step_actions(staged)
                shut = g.still_shut()
            g.open()
            assert shut, f"{case}: step {t} waited for the device or outlasted the hold"
            _same_outputs(a, b, f"{case}: step {t}")
            _same_host(a, b, f"{case}: step {t}")
        assert a.counters()[1] > 0 and a.episode_summary(False)["truncated_only"] > 0, "no episode ended"
    finally:
        _close(a, b)


# -- c. multi-tick ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_step_many_twice_behind_one_gate():
    """Two step_many calls of K = 4 on a k_envq handle whose grid is smaller than its blocks (several ticks per
    launch): k_shares and k_drained of the first launch are queued ahead of the second."""
    G = gate()
    n, K = 4096, 4
    tune = dict(queue_mode=1, envs_per_block=16, queue_grid=96)
    a, b = (_vec(n, PLAIN5, autoreset=True, max_episode_steps=3, tune=tune) for _ in range(2))
    try:
        assert a.step_kernel() == "pgtg::k_envq<false>" and b.step_kernel() == a.step_kernel(), a.step_kernel()
        acts = _actions(n, 4 * K, 4)
        a.reset(seed=8)
        b.reset(seed=8)  # (on the default stream: step_many is the first call that has to bind the side stream)

        def twice(env, x):
            env.step_many(x[:K])
            env.step_many(x[K:])

        twice(a, acts[:2 * K])
        host_s = G.warm("step_many", lambda: twice(b, acts[:2 * K]))
        _same_outputs(a, b, "step_many: warm")
        l0 = a.step_launches()
        twice(a, acts[2 * K:])
        staged = _sentinel(acts[2 * K:], SENTINELS["actions"])
        g = G.shut("step_many", host_s)
        g.stage(staged, acts[2 * K:])
        with g.stream():
            twice(b, staged)
            shut = g.still_shut()
        g.open()
        assert shut, "step_many waited for the device or outlasted the hold"
        _same_outputs(a, b, "step_many: gated")
        _same_host(a, b, "step_many: gated", stats=False)
        assert a.step_launches() == b.step_launches() and a.step_launches() - l0 < 2 * K, (a.step_launches(), l0)
        # (the shares follow the workgroups' measured clocks, DESIGN.md 5r: two handles agree in what the table must
        # satisfy, one count per workgroup that sum to the blocks, not in the counts)
        sa, sb = a.block_shares(), b.block_shares()
        assert sa.shape == sb.shape == (96,) and int(sa.sum()) == int(sb.sum()) == n // 16, (sa, sb)
        assert a.error_count()[0] == 0
    finally:
        _close(a, b)


# -- d. snapshots ----------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_snapshot_save_load_copy_and_light_step():
    G = gate()
    n, slots = N_SMALL, 32
    a, b = (_vec(n, TRAFFIC3, autoreset=True, max_episode_steps=3) for _ in range(2))
    sa = sb = None
    try:
        rng = np.random.default_rng(6)
        idx = {k: torch.as_tensor(v).cuda() for k, v in dict(
            save_env=rng.permutation(n)[:slots], save_slot=rng.permutation(slots), load_slot=rng.integers(0, slots, 40),
            load_env=rng.permutation(n)[:40], src=rng.integers(0, n, 24), dst=rng.permutation(n)[:24]).items()}
        acts = _actions(n, 8, 7)
        a.reset(seed=5)
        sa = a.snapshot(slots)
        b.reset(seed=5)  # (on the default stream: Snapshot.save is the first call that has to bind the side stream)
        sb = b.snapshot(slots)

        def chain(env, snap, ix, x):
            snap.save(env, ix["save_env"], ix["save_slot"])
            env.step_actions(x[0])
            env.step_actions(x[1])
            snap.load(env, ix["load_slot"], ix["load_env"], check=False)
            env.copy_envs(ix["src"], ix["dst"], check=False)
            out = env.light_step(x[2])
            env.step_actions(x[3])
            return [out[0]["map"][env.keys[0]], out[0]["position"], out[0]["velocity"], out[1], out[2], out[3]]

        la = chain(a, sa, idx, acts[:4])
        lb = []
        host_s = G.warm("snapshots", lambda: lb.extend(chain(b, sb, idx, acts[:4])))
        _same_outputs(a, b, "snapshots: warm")
        _same_tensors(la, lb, "snapshots: warm light_step")
        la = chain(a, sa, idx, acts[4:])
        st_idx = {k: _sentinel(v, SENTINELS["indices"]) for k, v in idx.items()}
        st_act = _sentinel(acts[4:], SENTINELS["actions"])
        g = G.shut("snapshots", host_s)
        for k in idx:
            g.stage(st_idx[k], idx[k])
        g.stage(st_act, acts[4:])
        with g.stream():
            lb = chain(b, sb, st_idx, st_act)
            shut = g.still_shut()
        g.open()
        assert shut, "the snapshot chain waited for the device or outlasted the hold"
        _same_outputs(a, b, "snapshots: gated")
        _same_tensors(la, lb, "snapshots: gated light_step")
        _same_host(a, b, "snapshots: gated", stats=False)
        for i in (0, 17, n - 1):
            assert a.env_state(i) == b.env_state(i) and np.array_equal(a.cars(i), b.cars(i)), i
    finally:
        torch.cuda.synchronize()
        for s in (sa, sb):
            if s is not None:
                s.close()
        _close(a, b)


# -- e. the training chain and its no-synchronisation claim --------------------------------------------------------
RO_ROWS = ("advantages", "returns", "obs", "terminal_obs", "actions", "rewards", "dones", "truncated_only", "values",
           "log_probs", "terminal_values", "costs", "penalised_rewards", "ep_cost", "normalised_rewards", "ret", "ret_rms",
           "row_var")


class _Trainer:
    def __init__(self):
        from pgtg_amd import policy as P
        from pgtg_amd.flat import flat_dim
        self.env = _vec(N_SMALL, TRAIN, autoreset=True, max_episode_steps=3)
        torch.manual_seed(4)
        self.module = P.MlpPolicyReference(flat_dim(self.env.spec)).cuda()
        self.pol = P.DevicePolicy(self.env, seed=9)
        self.opt = P.DeviceAdam(self.pol, self.module)
        self.ro = self.env.rollout(5, norm_reward=True, cost_limit=0.5)

    def weights(self):
        return {k: v.detach().clone() for k, v in self.module.state_dict().items()}

    def chain(self, sd, **kw):
        """load_state_dict, collect, update: none of them is documented to synchronise (collect()'s begin()
        continues the rollout; the seeded begin() that resets the env runs before the first chain)."""
        self.pol.load_state_dict(sd)
        self.ro.collect(self.pol)
        self.ro.update(self.pol, self.module, self.opt, n_epochs=2, batch_size=120, perm_seed=3, clip_range_vf=0.2, **kw)

    def tensors(self):
        ts = [getattr(self.ro, r) for r in RO_ROWS]
        names = list(RO_ROWS)
        for k, p in self.module.named_parameters():
            ts += [p.detach(), self.opt.exp_avg[k], self.opt.exp_avg_sq[k]]
            names += [k, "exp_avg " + k, "exp_avg_sq " + k]
        return ts, names

    def close(self):
        self.ro.close()
        self.env.close()


def _same_training(a, b, tag):
    (ta, names), (tb, _) = a.tensors(), b.tensors()
    _same_tensors(ta, tb, tag, names)
    assert a.ro.lagrange_multiplier == b.ro.lagrange_multiplier, tag
    _same_dict(a.ro.train_log(), b.ro.train_log(), tag + " train_log")
    _same_dict(a.ro.cost_log(), b.ro.cost_log(), tag + " cost_log")
    _same_dict(a.ro.norm_log(), b.ro.norm_log(), tag + " norm_log")
    assert a.opt.step_count == b.opt.step_count and a.ro.n_updates == b.ro.n_updates, tag
    _same_host(a.env, b.env, tag, stats=False)


@pytest.mark.timeout(180)
def test_training_chain_is_ordered_and_does_not_synchronise():
    G = gate()
    a, b = _Trainer(), _Trainer()
    try:
        a.ro.begin(seed=11)
        a.chain(a.weights())
        with G.on_side():
            b.ro.begin(seed=11)
            sd = b.weights()
        host_s = G.warm("training chain", lambda: b.chain(sd))
        _same_training(a, b, "training: warm")
        # the gated pass: collect() continues the rollout (row T to row 0), the weights arrive through the gate
        a.chain(a.weights())
        real = b.weights()
        staged = {k: _sentinel(v, SENTINELS["weights"]) for k, v in real.items()}
        g = G.shut("training chain", host_s)
        for k in real:
            g.stage(staged[k], real[k])
        with g.stream():
            b.chain(staged)
            shut = g.still_shut()
        g.open()
        assert shut, "load_state_dict / collect / update synchronised with the host (or outlasted the hold)"
        _same_training(a, b, "training: gated")
        # target_kl: one host read at the end of update() may block, so results only
        a.chain(a.weights(), target_kl=0.01)
        real = b.weights()
        staged = {k: _sentinel(v, SENTINELS["weights"]) for k, v in real.items()}
        g = G.shut("training chain target_kl", host_s)
        for k in real:
            g.stage(staged[k], real[k])
        with g.stream():
            b.chain(staged, target_kl=0.01)
        g.open()
        _same_training(a, b, "training: gated, target_kl")
    finally:
        _close(a, b)


# -- f. evaluation -----------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_evaluation_steps_records_and_summary():
    G = gate()
    n = N_SMALL
    a, b = (_vec(n, TRAFFIC3, autoreset=True, max_episode_steps=3) for _ in range(2))
    try:
        ea, eb = a.evaluation(6 * n), b.evaluation(6 * n)
        acts = _actions(n, 16, 9)
        rng = np.random.default_rng(3)
        rec = (torch.as_tensor(rng.normal(size=n)).cuda(), torch.as_tensor(rng.random(n) < 0.3).cuda(),
               torch.as_tensor(rng.random(n) < 0.3).cuda())
        ea.begin(seed=3)
        for t in range(16):
            ea.step(acts[t])
        ea.record_from(*rec)
        with G.on_side():
            eb.begin(seed=3)

        def eight(t0):
            for t in range(t0, t0 + 8):
                eb.step(acts[t])

        host_s = G.warm("evaluation", lambda: eight(0))
        for t in range(8, 16):
            staged = _sentinel(acts[t], SENTINELS["actions"])
            g = G.shut(f"evaluation t={t}", host_s)
            g.stage(staged, acts[t])
            with g.stream():
                eb.step(staged)
            g.open()
        st = [_sentinel(x, 0) for x in rec]
        g = G.shut("evaluation record_from", host_s)
        for s, x in zip(st, rec):
            g.stage(s, x)
        with g.stream():
            eb.record_from(*st)
            sb = eb.summary()  # (host-synchronising by design)
        g.open()
        _same_dict(ea.summary(), sb, "evaluation summary")
        _same_dict(ea.records(), eb.records(), "evaluation records")
        assert sb["episodes"] > 0
        _same_outputs(a, b, "evaluation")
    finally:
        _close(a, b)


# -- g. state across a stream ------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_dump_and_load_state_across_a_stream():
    G = gate()
    n = N_SMALL
    a, b, c = (_vec(n, TRAFFIC3, autoreset=True, max_episode_steps=3) for _ in range(3))
    try:
        acts = _actions(n, 3, 10)
        a.reset(seed=14)
        a.step_actions(acts[0])
        a.step_actions(acts[1])
        blob = a.dump_state()
        with G.on_side():
            b.reset(seed=14)
            c.reset(seed=99)  # (another state; its last launches are on the side stream)
            c.step_actions(acts[2])
        host_s = G.warm("state", lambda: b.step_actions(acts[0]))
        staged = _sentinel(acts[1], SENTINELS["actions"])
        g = G.shut("state dump", host_s)
        g.stage(staged, acts[1])
        with g.stream():
            b.step_actions(staged)
            got = b.dump_state()  # (at once: the dump drains the handle's stream itself)
        assert blob.size == got.size
        for sid, (x, y) in _sections(blob, got).items():  # (the bytes between the sections are the buffers' own)
            assert np.array_equal(x, y), f"state section {sid}: the dump did not wait for the step on the side stream"
        g.open()
        a.step_actions(acts[2])
        staged = _sentinel(acts[2], SENTINELS["actions"])
        with torch.cuda.stream(G.side):
            c.load_state(blob)
        g = G.shut("state load", host_s)
        g.stage(staged, acts[2])
        with g.stream():
            c.step_actions(staged)
            shut = g.still_shut()
        g.open()
        assert shut
        torch.cuda.synchronize()
        done = a.terminated | a.truncated  # (outputs are not state: the final_* rows are written for finished envs only)
        live = lambda e: [e.obs_map, e.position, e.velocity, e.reward, e.terminated, e.truncated, e.braking, e.cost,  # noqa: E731
                          e.final_map[done], e.final_position[done], e.final_velocity[done]]
        _same_tensors(live(a), live(c), "the step after load_state")
        assert a.error_count() == c.error_count() == (0, 0)
        for i in (0, 31, n - 1):
            assert a.env_state(i) == c.env_state(i) and np.array_equal(a.cars(i), c.cars(i)), i
    finally:
        _close(a, b, c)


# -- h. host getters drain the handle's stream themselves ------------------------------------------------------------
@pytest.mark.timeout(120)
def test_host_getters_drain_the_side_stream():
    G = gate()
    n = N_SMALL
    a, b = (_vec(n, TRAFFIC3, autoreset=True, max_episode_steps=3) for _ in range(2))
    try:
        for e in (a, b):
            e.enable_episode_stats()
        getters = (("error_count", lambda e: e.error_count()), ("env_state", lambda e: e.env_state(n - 1)),
                   ("cars", lambda e: e.cars(5).tolist()), ("counters", lambda e: e.counters()),
                   ("episode_summary", lambda e: e.episode_summary(False)))
        acts = _actions(n, 1 + len(getters), 11)
        acts[1, 7] = 255  # (one invalid action, so that error_count has something to report after that step)
        torch.cuda.synchronize()
        a.reset(seed=2)
        a.step_actions(acts[0])
        with G.on_side():
            b.reset(seed=2)
        host_s = G.warm("getters", lambda: b.step_actions(acts[0]))
        for k, (name, get) in enumerate(getters, 1):
            a.step_actions(acts[k])
            staged = _sentinel(acts[k], SENTINELS["actions"])
            g = G.shut(f"getter {name}", host_s)
            g.stage(staged, acts[k])
            with g.stream():
                b.step_actions(staged)
                got = get(b)  # (no synchronisation of the caller's in between)
            g.open()
            want = get(a)
            assert got == want, (name, got, want)
            if name == "error_count":
                assert want[0] == 1, want
    finally:
        _close(a, b)


# -- i. two handles, two side streams ----------------------------------------------------------------------------------
class _Solo:
    def __init__(self, seed):
        from pgtg_amd import policy as P
        from pgtg_amd.flat import flat_dim
        self.seed = seed
        self.env = _vec(N_SMALL, TRAIN, autoreset=True, max_episode_steps=3)
        torch.manual_seed(seed)
        module = P.MlpPolicyReference(flat_dim(self.env.spec)).cuda()
        self.pol = P.DevicePolicy(self.env, seed=seed)
        self.sd = {k: v.detach().clone() for k, v in module.state_dict().items()}
        self.ro = self.env.rollout(4, cost_limit=0.5)
        self.acts = _actions(N_SMALL, 6, seed)
        self.out = []

    def calls(self):
        """The run call by call (a generator: two runs are interleaved by taking turns)."""
        self.env.reset(seed=self.seed)
        yield
        for t in range(6):
            self.env.step_actions(self.acts[t])
            self.out += [x.clone() for x in self.env._bound_tensors()]
            yield
        self.pol.load_state_dict(self.sd)
        yield
        self.ro.begin(seed=self.seed + 1)
        yield
        self.ro.collect(self.pol)
        self.out += [getattr(self.ro, r).clone() for r in RO_ROWS if hasattr(self.ro, r)]
        yield

    def close(self):
        self.ro.close()
        self.env.close()


@pytest.mark.timeout(120)
def test_two_handles_on_two_streams_interleaved():
    """No gate: two handles with different seeds on two side streams, call by call in turns; each must equal its
    solo run on the default stream (no device or host state shared between handles)."""
    G = gate()
    want = {}
    for seed in (3, 4):  # (the solo runs first: three handles at a time at the most)
        s = _Solo(seed)
        for _ in s.calls():
            pass
        torch.cuda.synchronize()
        want[seed] = [x.cpu() for x in s.out]
        s.close()
    x, y = _Solo(3), _Solo(4)
    try:
        second = torch.cuda.Stream()
        torch.cuda.synchronize()
        gx, gy = x.calls(), y.calls()
        live = [(gx, G.side), (gy, second)]
        while live:
            for pair in list(live):
                with torch.cuda.stream(pair[1]):
                    if next(pair[0], StopIteration) is StopIteration:
                        live.remove(pair)
        torch.cuda.synchronize()
        for s in (x, y):
            got = [t.cpu() for t in s.out]
            _same_tensors(want[s.seed], got, f"handle of seed {s.seed}")
            assert s.env.error_count() == (0, 0)
    finally:
        _close(x, y)
