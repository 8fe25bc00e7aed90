"""k_envq<BIG, true>'s hand-off with the drain as an explicit-state model, every interleaving.

One workgroup: two env-side waves A and B (A holds tid 0) and the helper H, scheduled one atomic step at a time in
every order (a depth-first search over the states reached).  A block has one env per wave.  Per block a wave takes
(at a tick's first block it first waits for `fdone >= tick`): an env that resets checks its ring head's tag against
its spawn counter, rotates the roles (head -> cur, spare -> head) and appends a request for the slot freed to this
tick's list; then the block's last barrier; then A stores the list's count.  At a tick's last block each wave adds
one to `rdone` and A clears `qn`.  H serves the launch before's list at pass 0, then per tick publishes `fdone`,
waits for `rdone >= 2 tick` and serves that tick's list, clearing the count it read; the pass after the last tick is
the drain.  A launch ends when all three have ended.  Two workgroups, which share nothing inside a launch, are
explored one after the other; a second launch follows with their blocks swapped, from every end state of the first.

Held at every step: an entry taken carries the tag of the episode that takes it; H never writes the slot that
holds its env's live plan; no request is served twice.  At a launch's end: every request made was served, both lists'
counts are 0, and a workgroup's list names no env (so any workgroup may own any block next).  Dropping the drain,
lowering the drain's `rdone` threshold by one, or not clearing the counts must each be reported."""
import itertools

import pytest

NW = 2  # env-side waves


class Violation(Exception):
    pass


def _initial_rings(envs):
    # per env: (cur, head, spawn, tags[3]); the head holds episode `spawn`, the spare `spawn + 1`
    return {e: (0, 1, 1, (0, 1, 2)) for e in envs}


def _launch(blocks, ticks, resets, rings, lists, counts, par0, drain=True, thr_off=0, clear=True):
    """Every interleaving of one workgroup's launch.  blocks: tuple of block ids (env of wave w in block b: (b, w));
    resets[(tick, b)]: that block's envs reset in that tick.  Returns the set of end states
    (rings, lists, counts) -- frozen -- or raises Violation."""
    nb = len(blocks)
    # wave state: (pc, tick, k) pc: 4 arrive at the block's first barrier, 5 wait for it, 0 wait/take, 1 at the last
    # barrier, 2 after it (A stores the count), 3 tick end, 9 ended
    # helper state: (pc, pass, idx) pc: 0 read count, 1 serve entry idx, 2 publish, 3 wait, 9 ended
    start = (((4, 0, 0),) * NW, (0, 0, 0), 0, 0, 0, (0,) * (2 * nb),  # waves, helper, qn, rdone, fdone, barrier arrivals
             tuple(sorted(rings.items())), lists, counts, 0, frozenset(), frozenset())  # ..., helper cnt, made, served
    seen, stack, ends = {start}, [start], set()

    def push(st):
        if st not in seen:
            seen.add(st)
            stack.append(st)

    while stack:
        st = stack.pop()
        waves, hel, qn, rdone, fdone, bar, rg, ls, ct, hcnt, made, served = st
        rgd = dict(rg)
        if all(w[0] == 9 for w in waves) and hel[0] == 9:
            if made - served:
                raise Violation(f"requests never served: {sorted(made - served)}")
            if any(ct):
                raise Violation(f"a list's count is {ct} at the launch's end")
            ends.add((rg, ls, ct))
            continue
        moved = False
        for w in range(NW):
            pc, tick, k = waves[w]
            if pc == 9:
                continue
            par = (par0 + tick) & 1
            b = blocks[k] if nb else None
            nqn, nrd, nbar, nrg, nls, nct, nmade = qn, rdone, bar, rg, ls, ct, made
            if nb == 0:
                nw = (9, 0, 0)
            elif pc == 4:
                nw = (5, tick, k)
                nbar = bar[:nb + k] + (bar[nb + k] + 1,) + bar[nb + k + 1:]
            elif pc == 5:
                if bar[nb + k] < NW * (tick + 1):
                    continue  # the block's first barrier (plans staged; A's `qn = 0` of the tick before is behind it)
                nw = (0, tick, k)
            elif pc == 0:
                if k == 0 and tick > 0 and fdone < tick:
                    continue  # the take's wait
                env = (b, w)
                if resets.get((tick, b)):
                    cur, head, spawn, tags = rgd[env]
                    if tags[head] != spawn:
                        raise Violation(f"take of env {env} at tick {tick}: tag {tags[head]} for episode {spawn}")
                    spare = 3 - cur - head
                    req = (env, cur, spawn + 2)
                    lst = list(ls)
                    lst[par] = ls[par][:qn] + (req,)
                    nls, nqn, nmade = tuple(lst), qn + 1, made | {req}
                    rgd2 = dict(rgd)
                    rgd2[env] = (head, spare, spawn + 1, tags)
                    nrg = tuple(sorted(rgd2.items()))
                nw = (1, tick, k)
                nbar = bar[:k] + (bar[k] + 1,) + bar[k + 1:]
            elif pc == 1:
                if bar[k] < NW * (tick + 1):
                    continue  # the block's last barrier
                nw = (2, tick, k)
            elif pc == 2:
                if w == 0:  # tid 0: every request of the block is in
                    c = list(ct)
                    c[par] = qn
                    nct = tuple(c)
                nw = (4, tick, k + 1) if k + 1 < nb else (3, tick, k)
            else:  # pc == 3: the tick's end
                nrd = rdone + 1
                if w == 0:
                    nqn = 0
                nw = (4, tick + 1, 0) if tick + 1 < ticks else (9, 0, 0)
            moved = True
            push((waves[:w] + (nw,) + waves[w + 1:], hel, nqn, nrd, fdone, nbar, nrg, nls, nct, hcnt, nmade, served))
        pc, p, idx = hel
        if pc != 9:
            lpar = (par0 + p + 1) & 1  # the list of the tick before pass p
            nh, nfd, nrg, nct, nhc, nserved = hel, fdone, rg, ct, hcnt, served
            ok = True
            if pc == 0:
                nhc = ct[lpar]
                if clear and nhc:
                    c = list(ct)
                    c[lpar] = 0
                    nct = tuple(c)
                nh = (1, p, 0)
            elif pc == 1:
                if idx < hcnt:
                    env, slot, spawn = req = ls[lpar][idx]
                    cur, head, sp, tags = rgd[env]
                    if slot == cur:
                        raise Violation(f"helper writes slot {slot} of env {env}, its live plan")
                    if req in served:
                        raise Violation(f"request {req} served twice")
                    rgd2 = dict(rgd)
                    rgd2[env] = (cur, head, sp, tags[:slot] + (spawn,) + tags[slot + 1:])
                    nrg, nserved, nh = tuple(sorted(rgd2.items())), served | {req}, (1, p, idx + 1)
                else:
                    last = p == (ticks if drain else ticks - 1)
                    nh = (9, 0, 0) if last or nb == 0 else (2, p, 0)
            elif pc == 2:
                nfd, nh = p + 1, (3, p, 0)
            else:
                thr = NW * (p + 1) - (thr_off if p + 1 == ticks else 0)
                if rdone < thr:
                    ok = False
                else:
                    nh = (0, p + 1, 0)
            if ok:
                moved = True
                push((waves, nh, qn, rdone, nfd, bar, nrg, ls, nct, nhc, made, nserved))
        if not moved:
            raise Violation("deadlock")
    return ends


def _two_launches(nb, pattern, second=True, **kw):
    """Workgroup 0 owns blocks 0..nb-1 and workgroup 1 blocks nb..2nb-1 for 3 ticks; then a launch of 2 ticks with
    the blocks swapped.  pattern: resets per (tick, block position), the same for both workgroups."""
    ticks = 3
    own = [tuple(range(nb)), tuple(range(nb, 2 * nb))]
    res = [{(t, b): pattern[t][k] for t in range(5) for k, b in enumerate(blk)} for blk in own]
    empty = ((), ())
    ends = []
    for g in (0, 1):
        rings = _initial_rings([(b, w) for b in own[g] for w in range(NW)])
        ends.append(_launch(own[g], ticks, res[g], rings, empty, (0, 0), 0, **kw))
    for e0, e1 in itertools.product(*ends) if second else ():
        for g, (mine, theirs) in enumerate(((e0, e1), (e1, e0))):
            rg_other, ls_mine, ct_mine = theirs[0], mine[1], mine[2]
            named = {r[0] for lst, c in zip(ls_mine, ct_mine) for r in lst[:c]}
            if named:
                raise Violation(f"workgroup {g}'s list still names envs {sorted(named)} when its blocks change")
            res2 = {(t, b): res[1 - g][(t + ticks, b)] for t in range(2) for b in own[1 - g]}
            # the lists keep their (dead) entries beyond the counts, as the device's do
            _launch(own[1 - g], 2, res2, dict(rg_other), ls_mine, ct_mine, ticks & 1, **kw)


def _patterns(nb):
    """every reset pattern of the first launch's 3 ticks x nb blocks; the second launch resets every env"""
    for bits in itertools.product((False, True), repeat=3 * nb):
        yield [bits[t * nb:(t + 1) * nb] for t in range(3)] + [(True,) * nb] * 2


@pytest.mark.parametrize("nb", [1, 2])
def test_every_interleaving_and_reset_pattern_holds(nb):
    # (two blocks: the second launch follows the patterns whose first tick resets every env, 16 of the 64)
    for pattern in _patterns(nb):
        _two_launches(nb, pattern, second=nb == 1 or all(pattern[0]))


def test_a_workgroup_without_blocks_ends():
    assert _launch((), 3, {}, {}, ((), ()), (0, 0), 0) == {((), ((), ()), (0, 0))}


@pytest.mark.parametrize("kw,what", [(dict(drain=False), "never served"), (dict(thr_off=1), "never served|count"),
                                     (dict(clear=False), "count|twice")])
def test_broken_variants_are_reported(kw, what):
    import re
    with pytest.raises(Violation) as e:
        for pattern in _patterns(1):
            _two_launches(1, pattern, **kw)
    assert re.search(what, str(e.value)), str(e.value)
