"""Host model of k_envq's three-slot map rings with rotating roles (pgtg_amd/csrc/pgtg_env.hip: k_envq,
k_qfill, queue_spare, queue_req_cap), checked without a GPU: the same arithmetic as the kernel.

Per env three slots: cur (the live episode's plan, never copied elsewhere), head (the entry for the
env's spawn counter k0) and the spare (the entry for k0 + 5, ready or being made).  A reset in launch t
frees the old cur, makes the old head cur and the old spare head, and requests (env, freed slot,
k0 + 10); the helpers serve a launch's requests in the next launch, writing while the env waves read.
Slots carry (tag, plan bytes) here; a plan's bytes are a function of (env, spawn counter) as on the
device, so "unchanged" is checked on content, and a slot under the helper's pen reads as garbage.
"""
import numpy as np
import pytest

LANES = 64      # kQueueLanes
ENVS = 128      # envs per workgroup
GRID = 3        # resident workgroups (the persistent grid)
N = 5 * ENVS + 37
LAUNCHES = 200
GARBAGE = -1


def queue_spare(qc, qh):
    return 3 - qc - qh if qc != qh else (qc + 2) % 3


def queue_req_cap(nblk, grid, envs):
    return max(3 * ((nblk + grid - 1) // grid) * envs, LANES)


def plan_bytes(i, k):
    """stand-in for the generated map of env i, spawn counter k"""
    return (i * 1_000_003 + k * 7919) & 0x7FFFFFFF


def _pattern(name, rng, t, n):
    if name == "bernoulli":
        return rng.random(n) < 0.43
    if name == "every":
        return np.ones(n, bool)
    if name == "bursts":  # alternating: three launches of everything, three of nothing
        return np.full(n, (t // 3) % 2 == 0)
    return np.zeros(n, bool)


@pytest.mark.parametrize("pattern", ["bernoulli", "every", "bursts", "never"])
def test_three_slot_rotation(pattern):
    rng = np.random.default_rng(17)
    n = N
    nblk = (n + ENVS - 1) // ENVS
    cap = queue_req_cap(nblk, GRID, ENVS)
    spawn = np.full(n, 5, np.int64)                 # spawn counter of the next episode (k0)
    cur = np.zeros(n, np.int64)
    head = np.ones(n, np.int64)                     # k_qfill after the reset launch: cur 0, head 1, spare 2
    tag = np.zeros((n, 3), np.int64)
    body = np.zeros((n, 3), np.int64)
    for i in range(n):
        tag[i, 0], body[i, 0] = 0, plan_bytes(i, 0)             # the live episode's plan (k_env wrote it)
        tag[i, 1], body[i, 1] = spawn[i], plan_bytes(i, spawn[i])
        tag[i, 2], body[i, 2] = spawn[i] + 5, plan_bytes(i, spawn[i] + 5)
    live = body[np.arange(n), cur].copy()           # what each env's episode was started with
    pending, takes = [], 0
    for t in range(LAUNCHES):
        served, pending = pending, []
        cur0, head0 = cur.copy(), head.copy()       # roles at the launch's start
        # the helpers write during the launch: their slots hold garbage until it ends
        for i, s, _k in served:
            assert s != cur0[i] and s != head0[i], "the helper writes a slot that is cur or head"
            tag[i, s] = body[i, s] = GARBAGE
        resets = _pattern(pattern, rng, t, n)
        # workgroups take blocks as the kernel does: a workgroup stops taking blocks from the counter
        # before its list could overflow (qn + 2 * envs <= cap); the first block is its own
        qn = np.zeros(GRID, np.int64)
        blocks_of = {g: [g] for g in range(min(GRID, nblk))}
        for b in range(GRID, nblk):  # a random workgroup among those that may still take a block
            made = {g: sum(int(resets[x * ENVS:(x + 1) * ENVS].sum()) for x in bl) for g, bl in blocks_of.items()}
            may = [g for g in blocks_of if made[g] + 2 * ENVS <= cap]
            assert may, "no workgroup may take the next block"
            blocks_of[int(rng.choice(may))].append(b)
        for g, blocks in blocks_of.items():
            for b in blocks:
                for i in range(b * ENVS, min(n, (b + 1) * ENVS)):
                    # staging reads the cur slot: the live plan, unchanged since the take
                    assert body[i, cur0[i]] == live[i], "cur's plan changed while the episode is live"
                    if not resets[i]:
                        continue
                    qc, qh = cur0[i], head0[i]
                    assert tag[i, qh] == spawn[i], "a taken entry was not made for its episode"
                    assert body[i, qh] == plan_bytes(i, spawn[i])
                    takes += 1
                    live[i] = body[i, qh]
                    word = (i << 2 | qc) & 0xFFFFFFFF      # the request word as the kernel packs it
                    assert word >> 2 == i and min(word & 3, 2) == qc
                    pending.append((word >> 2, min(word & 3, 2), spawn[i] + 10))
                    qn[g] += 1
                    cur[i], head[i] = qh, queue_spare(qc, qh)
                    spawn[i] += 5
            assert qn[g] <= cap, "more requests than a workgroup's list holds"
        # the launch ends: the helpers' entries are whole
        for i, s, k in served:
            tag[i, s], body[i, s] = k, plan_bytes(i, k)
        # roles stay a permutation of the three slots
        sp = np.array([queue_spare(int(c), int(h)) for c, h in zip(cur, head)])
        assert ((cur != head) & (sp != cur) & (sp != head) & (sp >= 0) & (sp < 3)).all()
    if pattern == "every":
        assert takes == n * LAUNCHES
    if pattern == "never":
        assert takes == 0 and not pending
    if pattern in ("bernoulli", "bursts"):
        assert takes > n * LAUNCHES // 4


def test_spare_is_always_a_slot():
    """queue_spare on every byte a corrupt state could hold stays inside the ring"""
    for qc in range(3):
        for qh in range(3):
            s = queue_spare(qc, qh)
            assert 0 <= s < 3
            if qc != qh:
                assert s not in (qc, qh)
