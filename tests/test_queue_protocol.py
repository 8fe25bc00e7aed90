"""Host model of k_envq's map-ring protocol (pgtg_amd/csrc/pgtg_env.hip: k_envq, k_qfill), checked
without a GPU: the same arithmetic as the kernel, on random reset patterns.

* Rings of two entries: a reset in launch t takes the head slot and requests the map of spawn
  counter k0 + 10 into it; the helpers serve every request of launch t in launch t + 1.  The entry an
  env takes must always carry the tag of its episode (the kernel reports a mismatch as an error).
* One-round launches: a workgroup lists at most 64 requests; the rest go to the overflow list of its
  residue mod 8, and helper j of a residue serves the overflow items [P_j, P_j + spare_j) (P = the
  prefix sum of the spare lanes 64 - count of the residue's workgroups before it), then items
  tot + (k * nj + j) * 64 ... in whole batches.  Every item must be served exactly once.
* The hand-off inside a launch of several ticks (k_envq<BIG, true>, DESIGN 5p *Hand-offs*, *Progress*, *Reuse of
  the lists*): HandoffModel, an explicit-state model of one workgroup explored over every interleaving of its
  waves and every reset pattern.  Bound used: 4 ticks; 1 block per workgroup with two envs (one on each of two
  env waves) or 2 blocks with one env each (on different waves); the third wave carries no env; every env may
  also have reset in the last tick of the launch before (a request pending in the old list).  About 350 000
  states, a few seconds.
"""
import numpy as np
import pytest

LANES = 64


def _overflow_shares(counts, olen):
    """items served by each helper of one residue: counts = the residue's per-workgroup list lengths"""
    nj = len(counts)
    spare = [LANES - min(c, LANES) for c in counts]
    tot = sum(spare)
    served = [[] for _ in range(nj)]
    pre = 0
    for j in range(nj):
        on = min(olen - pre, spare[j]) if olen > pre else 0
        served[j] += list(range(pre, pre + on))
        pre += spare[j]
        st0 = tot + j * LANES
        while st0 < olen:
            served[j] += list(range(st0, min(st0 + LANES, olen)))
            st0 += nj * LANES
    return served


def test_overflow_items_served_exactly_once():
    rng = np.random.default_rng(3)
    for _ in range(300):
        nj = int(rng.integers(1, 140))
        counts = rng.integers(0, LANES + 1, nj)
        # an overflow list of up to (envs per block - 64) per workgroup (128- and 192-env workgroups)
        olen = int(rng.integers(0, nj * 128 + 1))
        served = _overflow_shares(list(counts), olen)
        flat = sorted(x for s in served for x in s)
        assert flat == list(range(olen)), (nj, olen)


def test_two_entry_rings_always_hold_the_episode():
    """reset patterns from every-step resets to none: the head entry's tag is always the episode's"""
    rng = np.random.default_rng(7)
    n = 500
    for p in (1.0, 0.43, 0.1):
        spawn = np.full(n, 5, np.int64)       # the spawn counter of the next episode
        head = np.zeros(n, np.int64)
        tag = np.zeros((n, 2), np.int64)
        tag[:, 0], tag[:, 1] = spawn, spawn + 5  # k_qfill after the reset
        pending = []                              # requests of the previous launch
        for _t in range(200):
            served, pending = pending, []         # the helpers serve the previous launch's requests
            h0 = head.copy()                      # ring heads at the launch's start
            resets = rng.random(n) < p
            for i in np.nonzero(resets)[0]:
                assert tag[i, h0[i]] == spawn[i], "a taken entry was not made for its episode"
                pending.append((i, h0[i], spawn[i] + 10))
                spawn[i] += 5
                head[i] ^= 1
            for i, slot, k in served:             # written during the launch, visible after it:
                assert not (resets[i] and slot == h0[i]), "a refill raced the take of its slot"
                tag[i, slot] = k


def _envb_launch(rng, p, E, spawn, qn, qh, tag, qcap=LANES):
    """One k_envb launch over one block of E envs (pgtg_env.hip k_envb): the helper refills level 0
    (empty rings, all of them, before any take) and then levels 1, 2 in list order (env order within a
    level) up to qcap entries; a reset takes the head; qn/qh follow the kernel's `have` arithmetic."""
    depth = 3
    F = [[i for i in range(E) if qn[i] <= l] for l in range(depth)]
    for i in F[0]:  # heads of empty rings
        tag[i, qh[i]] = spawn[i]
    served = [(i, l) for l in range(1, depth) for i in F[l]][:qcap]
    for i, l in served:  # written by the helper concurrently with the takes of other slots
        tag[i, (qh[i] + l) % depth] = spawn[i] + 5 * l
    resets = rng.random(E) < p
    for i in range(E):
        have = 1 if qn[i] == 0 else qn[i]
        have += sum(1 for (j, l) in served if j == i)
        if resets[i]:
            assert have >= 1 and tag[i, qh[i]] == spawn[i], "k_envb took an entry not made for its episode"
            # a refill written in this launch never lands on the slot taken (levels >= 1 are other slots)
            assert all(l == 0 or (qh[i] + l) % depth != qh[i] for (j, l) in served if j == i)
            spawn[i] += 5
            qh[i] = (qh[i] + 1) % depth
            have -= 1
        qn[i] = have
    return resets.sum()


def test_three_entry_rings_refilled_per_block():
    """k_envb: capped refills (64 per launch) with deferral through three-entry rings -- every take is
    the episode's map, also when a block resets more envs than its helper refills in one launch"""
    rng = np.random.default_rng(11)
    for E, p in ((128, 0.43), (128, 1.0), (192, 0.6), (16, 0.43), (64, 0.9)):
        spawn = np.full(E, 5, np.int64)
        qn = np.full(E, 3, np.int64)
        qh = np.zeros(E, np.int64)
        tag = np.zeros((E, 3), np.int64)
        for l in range(3):  # k_qfill_b after the reset
            tag[:, l] = spawn + 5 * l
        qcap = 2 * LANES if E > 128 else LANES
        for _t in range(300):
            _envb_launch(rng, p, E, spawn, qn, qh, tag, qcap)
            assert (qn >= 0).all() and (qn <= 3).all()


# ---- the hand-off between the waves of a workgroup inside a launch of several ticks ------------------

HANDOFF_TICKS = 4
NP_WAVES = 3  # kBlock / 64 - 1: the env and writer waves (wave 2 here carries no env: a writer wave)
P_STAGE, P_WAIT, P_TAKE, P_END, P_COUNT, P_ARRIVE, P_STEPS = 0, 1, 2, 3, 4, 5, 6


class HandoffModel:
    """One workgroup of k_envq<BIG, true>: its three env and writer waves and its helper, over `ticks` ticks of
    `blocks` blocks.  A state is (the waves' program counters, the helper's (tick, step, entry), fdone, rdone,
    *qn, the two lists' counts, the two lists, the envs' rings, the requests not yet served, the count the
    helper read).  An env is (0, cur slot, the three slots' episodes relative to the live one: head must
    hold 1 when it is taken, -1 is stale); a request is (env, slot, relative episode).  moves() yields
    (violation or None, next state) for every enabled move; a wave's steps, in the kernel's order:

      P_STAGE   the block's first sub_barrier ("plans, line masks"), with the staging of the cur slot before it
      P_WAIT    "the tick's first ring take: the helper has stored the fills it made during the tick before":
                the spin for fdone >= tick, at the tick's first block
      P_TAKE    the take of the ring head and "refill request: the next-but-one episode's map ... into the
                slot freed": the tag check, the atomicAdd on *qn, the req_new store, the roles' rotation.
                Whether the env resets is a choice of the model: both moves are explored.
      P_END     the block's last sub_barrier (before "every request of the block is in")
      P_COUNT   tid 0's store of *qn into S.qctr
      P_ARRIVE  "FUSED, the tick's last block (more ticks follow)": the release and the add to rdone, and
                tid 0's *qn = 0

    and the helper's, per tick: the store of fdone ("this tick's fills are stored"), the spin on rdone ("then the
    next list: every env and writer wave has arrived"), the read of the count, and per list entry its read and
    the fill of the ring slot.  A take and its request are one move, at the earliest point the wave can make
    them, and an entry's read and fill are one move: the helper's progress only ever helps both checks, so
    the earliest take and write are the worst case, and a slow helper is among the interleavings anyway."""

    def __init__(self, blocks, ticks=HANDOFF_TICKS, fdone_wait=True, rdone_need=lambda s: NP_WAVES * s):
        self.nb, self.T, self.fdone_wait, self.rdone_need = blocks, ticks, fdone_wait, rdone_need
        # env -> (block, wave)
        self.envs = [(0, 0), (0, 1)] if blocks == 1 else [(0, 0), (1, 1)]
        self.end_pc = ticks * blocks * P_STEPS

    def pc(self, t, j, pos):
        return (t * self.nb + j) * P_STEPS + pos

    def norm(self, w, p):
        """skip the steps that are no move of wave w"""
        while p < self.end_pc:
            blk, pos = divmod(p, P_STEPS)
            t, j = divmod(blk, self.nb)
            if pos == P_WAIT:
                idle = not (j == 0 and t > 0 and self.fdone_wait)
            elif pos == P_TAKE:
                idle = (j, w) not in self.envs
            elif pos == P_COUNT:
                idle = w != 0
            elif pos == P_ARRIVE:
                idle = not (j == self.nb - 1 and t < self.T - 1)
            else:
                idle = False
            if not idle:
                break
            p += 1
        return p

    def last_write_pc(self, w, t):
        if w == 0:
            return self.pc(t, self.nb - 1, P_COUNT)
        js = [j for (j, ww) in self.envs if ww == w]
        return self.pc(t, max(js), P_TAKE) if js else -1

    def initial_states(self):
        n = len(self.envs)
        for pat in range(1 << n):
            envs, buf, uns = [], [], []
            for i in range(n):
                if pat >> i & 1:
                    envs.append((0, 1, (-1, 0, 1)))
                    buf.append((i, 0, 2))
                    uns.append((i, 0, 2))
                else:
                    envs.append((0, 0, (0, 1, 2)))
            yield ((0,) * NP_WAVES, (0, 2, 0), 0, 0, 0, (0, len(buf)), ((), tuple(buf)), tuple(envs), tuple(sorted(uns)), 0)

    def moves(self, st):
        pcs, (hs, hpos, hj), fdone, rdone, qn, counts, bufs, envs, uns, hcnt = st
        nb, T = self.nb, self.T
        for w in range(NP_WAVES):
            p = pcs[w]
            if p >= self.end_pc:
                continue
            blk, pos = divmod(p, P_STEPS)
            t, j = divmod(blk, nb)
            par = t & 1
            mine = [i for i, (jj, ww) in enumerate(self.envs) if jj == j and ww == w]

            def go(npc, **kw):
                d = dict(fdone=fdone, rdone=rdone, qn=qn, counts=counts, bufs=bufs, envs=envs, uns=uns)
                d.update(kw)
                return (pcs[:w] + (self.norm(w, npc),) + pcs[w + 1:], (hs, hpos, hj), d["fdone"], d["rdone"], d["qn"], d["counts"],
                        d["bufs"], d["envs"], d["uns"], hcnt)
            if pos == P_STAGE:
                if all(q >= p for q in pcs):
                    bad = [i for i in mine if envs[i][2][envs[i][1]] != envs[i][0]]
                    yield ("a wave staged a cur slot that does not hold its episode" if bad else None), go(p + 1)
            elif pos == P_WAIT:
                if j == 0 and t > 0 and self.fdone_wait and fdone < t:
                    continue
                yield None, go(p + 1)
            elif pos == P_TAKE:
                yield None, go(p + 1)
                if mine:
                    i = mine[0]
                    e, cur, cont = envs[i]
                    head = (cur + 1) % 3
                    v = None
                    if cont[head] != e + 1:
                        v = "a take met an entry that does not carry its episode's tag"
                    elif t > 0 and not (hs > t - 1 or (hs == t - 1 and hpos == 3)):
                        v = "a wave wrote a request into a list the helper has not finished reading"
                    # (episodes are kept relative to the env's live one: everything of env i moves down by one)
                    sh = lambda rs: tuple((a, s_, ep - 1) if a == i else (a, s_, ep) for (a, s_, ep) in rs)  # noqa: E731
                    r = (i, cur, 2)
                    b = list(sh(bufs[par]))
                    b[qn:qn + 1] = [r]
                    nbufs = (tuple(b), sh(bufs[1])) if par == 0 else (sh(bufs[0]), tuple(b))
                    nenvs = envs[:i] + ((0, head, tuple(max(c - 1, -1) for c in cont)),) + envs[i + 1:]
                    yield v, go(p + 1, qn=qn + 1, bufs=nbufs, envs=nenvs, uns=tuple(sorted(sh(uns) + (r,))))
            elif pos == P_END:
                if all(q >= p for q in pcs):
                    yield None, go(p + 1)
            elif pos == P_COUNT:
                if w != 0:
                    yield None, go(p + 1)
                else:
                    v = None
                    if t > 0 and not (hs > t - 1 or (hs == t - 1 and hpos == 3)):
                        v = "tid 0 stored a count the helper has not finished with"
                    nc = (qn, counts[1]) if par == 0 else (counts[0], qn)
                    nbufs = bufs
                    if j == nb - 1:  # (entries beyond the count are dead: dropped, to keep the state space small)
                        nbufs = (bufs[0][:qn], bufs[1]) if par == 0 else (bufs[0], bufs[1][:qn])
                    yield v, go(p + 1, counts=nc, bufs=nbufs)
            else:
                if j == nb - 1 and t < T - 1:
                    yield None, go(p + 1, rdone=rdone + 1, qn=0 if w == 0 else qn)
                else:
                    yield None, go(p + 1)
        if hs < T:
            old = (hs & 1) ^ 1

            def hgo(h, **kw):
                d = dict(fdone=fdone, envs=envs, uns=uns, hcnt=hcnt)
                d.update(kw)
                return (pcs, h, d["fdone"], rdone, qn, counts, bufs, d["envs"], d["uns"], d["hcnt"])

            def writable():
                return hs > 0 and any(pcs[w] <= self.last_write_pc(w, hs - 1) for w in range(NP_WAVES))
            if hpos == 0:
                yield None, hgo((hs, 1, 0), fdone=hs)
            elif hpos == 1:
                if rdone >= self.rdone_need(hs):
                    yield None, hgo((hs, 2, 0))
            elif hpos == 2:
                v = "the helper read a count that a wave can still write" if writable() else None
                yield v, hgo((hs, 3, 0), hcnt=counts[old])
            else:
                if hj < hcnt:
                    v = "the helper read a list entry that a wave can still write" if writable() else None
                    if hj >= len(bufs[old]):
                        yield "the helper read past the list", hgo((hs, 3, hj + 1))
                        return
                    r = bufs[old][hj]
                    i, slot, ep = r
                    e, cur, cont = envs[i]
                    if v is None and r not in uns:
                        v = "a request was served twice"
                    if v is None and slot == cur:
                        v = "the helper wrote the cur slot of an env"
                    nuns = tuple(x for x in uns if x != r)
                    ncont = cont[:slot] + (ep,) + cont[slot + 1:]
                    yield v, hgo((hs, 3, hj + 1), envs=envs[:i] + ((e, cur, ncont),) + envs[i + 1:], uns=nuns)
                else:
                    # (the list it has read is dead: dropped, to keep the state space small)
                    nb_ = ((), bufs[1]) if old == 0 else (bufs[0], ())
                    yield None, (pcs, (hs + 1, 0, 0) if hs + 1 < T else (T, 0, 0), fdone, rdone, qn, counts, nb_, envs, uns, 0)

    def final_check(self, st):
        pcs, h, fdone, rdone, qn, counts, bufs, envs, uns, hcnt = st
        par = (self.T - 1) & 1
        left = tuple(sorted(bufs[par][:counts[par]]))
        if left != uns:
            return "a request was lost"
        return None

    def explore(self, first_only=False):
        """(violations, states, final states) over every interleaving and reset pattern; first_only: stop
        at the first violation"""
        seen, stack, viol, finals = set(), [], set(), 0
        for s in self.initial_states():
            seen.add(s)
            stack.append(s)
        while stack:
            st = stack.pop()
            any_move = False
            for v, nx in self.moves(st):
                any_move = True
                if v:
                    viol.add(v)
                    continue
                if nx not in seen:
                    seen.add(nx)
                    stack.append(nx)
            if first_only and viol:
                break
            if not any_move:
                if all(p >= self.end_pc for p in st[0]) and st[1][0] >= self.T:
                    finals += 1
                    v = self.final_check(st)
                    if v:
                        viol.add(v)
                else:
                    viol.add("a state that is not final has no enabled move")
        return viol, len(seen), finals


@pytest.mark.parametrize("blocks", [1, 2])
def test_handoff_model_properties(blocks):
    """Progress: no reachable state but the final ones is without an enabled move.  Reuse of the lists: the
    helper never reads a count or an entry that a wave can still write, and no wave writes a list or its
    count before the helper has finished reading it.  Every entry a take meets carries its episode's tag,
    no fill lands on a cur slot, and every request is served exactly once (those of the last tick are left
    in the list, under its count, for the next launch)."""
    viol, states, finals = HandoffModel(blocks).explore()
    print(blocks, "blocks:", states, "states,", finals, "final")
    assert not viol, viol
    assert states > 10000 and finals > 50  # (the exploration went through the ticks and the reset patterns)


BROKEN = {
    "no_fdone_wait": dict(fdone_wait=False),
    "rdone_threshold_less_one": dict(rdone_need=lambda s: NP_WAVES * s - 1),
    "helper_waits_for_its_own_tick": dict(rdone_need=lambda s: NP_WAVES * (s + 1)),
}


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("name", list(BROKEN))
def test_handoff_model_reports_a_broken_protocol(name, blocks):
    """the model has teeth: without the fdone wait, with the rdone threshold one lower, and with the helper
    waiting for the arrivals of tick t instead of tick t - 1 (which the last tick never makes), it reports
    a violation"""
    viol, _, _ = HandoffModel(blocks, **BROKEN[name]).explore(first_only=True)
    print(name, blocks, viol)
    assert viol
