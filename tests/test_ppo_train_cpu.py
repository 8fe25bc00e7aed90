"""The host side of PPO.train in full (no GPU): ppo_reference with value clipping against torch float64 autograd of
SB3's expression, permutation_reference (what k_ppo_perm writes), and the ctypes mirrors of PgtgPpoExtra and
PgtgPpoLog against the compiled header."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import helpers
import ppo_cases as ppc
import ppo_train_cases as ptc
from pgtg_amd import _abi
from pgtg_amd import policy as P
from pgtg_amd import rollout as R

D = 29
CLIP_VF = ptc.CLIP_VF
TOTALS = (1, 2, 3, 240, 255, 256, 257, 4099, 65537)


def clipped_batch(c, B):
    return ptc.batch(c.D, B)


@pytest.mark.parametrize("B", (1, 64, 65))
@pytest.mark.parametrize("norm, ent", ppc.CONFIGS)
def test_value_clip_reference_is_torch_float64_autograd(B, norm, ent):
    c = ppc.case(D)
    b, ov = clipped_batch(c, B)
    g, s = P.ppo_reference(c.sd, *b, ppc.CLIP, ent, ppc.VF, norm, clip_range_vf=CLIP_VF, old_values=ov)
    tg, ts = ptc.torch_clipped(c.sd, *b, ov, CLIP_VF, ent, norm, torch.float64)
    for k in ppc.KEYS:
        scale = max(np.abs(tg[k]).max(), 1e-300)
        assert np.abs(g[k] - tg[k]).max() <= 1e-10 * scale, (k, np.abs(g[k] - tg[k]).max(), scale)
    assert np.allclose(s[:6], ts, rtol=1e-10, atol=0), (s, ts)
    plain, _ = P.ppo_reference(c.sd, *b, ppc.CLIP, ent, ppc.VF, norm)
    if B > 1:  # (both sides of the clip are present: the value tower's gradient differs from the unclipped one)
        assert not np.array_equal(g["value_net.weight"], plain["value_net.weight"])
    for k in ("action_net.weight", "mlp_extractor.policy_net.0.weight"):
        assert np.array_equal(g[k], plain[k]), k


def test_value_clip_edges():
    c = ppc.case(D)
    b, ov = clipped_batch(c, 65)
    plain = P.ppo_reference(c.sd, *b, ppc.CLIP, 0.01, ppc.VF, True)
    wide = P.ppo_reference(c.sd, *b, ppc.CLIP, 0.01, ppc.VF, True, clip_range_vf=1e30, old_values=ov)
    assert all(np.array_equal(plain[0][k], wide[0][k]) for k in ppc.KEYS) and np.array_equal(plain[1], wide[1])
    none = P.ppo_reference(c.sd, *b, ppc.CLIP, 0.01, ppc.VF, True, clip_range_vf=None, old_values=ov)
    assert all(np.array_equal(plain[0][k], none[0][k]) for k in ppc.KEYS) and np.array_equal(plain[1], none[1])
    g0, s0 = P.ppo_reference(c.sd, *b, ppc.CLIP, 0.01, ppc.VF, True, clip_range_vf=0.0, old_values=ov)
    for k in ppc.KEYS:
        if "value_net" in k:
            assert not g0[k].any(), k
        else:
            assert np.array_equal(g0[k], plain[0][k]), k
    assert s0[2] == np.mean((b[4].astype(np.float64) - ov.astype(np.float64)) ** 2)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.ppo_reference(c.sd, *b, ppc.CLIP, 0.01, ppc.VF, True, clip_range_vf=bad, old_values=ov)
    with pytest.raises(ValueError):
        P.ppo_reference(c.sd, *b, ppc.CLIP, 0.01, ppc.VF, True, clip_range_vf=0.2)


@pytest.mark.parametrize("total", TOTALS)
def test_permutation_reference_is_a_keyed_bijection(total):
    longest = 0
    first = None
    for counter in range(8):
        perm, walk = R.permutation_reference(total, 7, counter, return_walk=True)
        longest = max(longest, walk)
        assert perm.dtype == np.int64 and perm.shape == (total,)
        assert np.array_equal(np.sort(perm), np.arange(total)), counter
        assert np.array_equal(perm, R.permutation_reference(total, 7, counter))
        first = perm if first is None else first
    print("perm-walk", total, longest)
    assert longest < R.PERM_WALK_CAP
    if total >= 240:  # (a domain of one, two or three elements has too few permutations to tell keys apart)
        others = [R.permutation_reference(total, 7, 1), R.permutation_reference(total, 8, 0),
                  R.permutation_reference(total, 7 + (1 << 32), 0), R.permutation_reference(total, 7, 1 << 40)]
        assert all(not np.array_equal(first, o) for o in others)


def test_permutation_reference_is_uncorrelated_with_the_order():
    s = np.arange(4096)
    corr = [float(np.corrcoef(s, R.permutation_reference(4096, 7, counter))[0, 1]) for counter in range(8)]
    print("perm-corr", [f"{x:+.3f}" for x in corr])
    assert max(abs(x) for x in corr) < 0.05, corr
    with pytest.raises(ValueError):
        R.permutation_reference(0, 7, 0)


def test_new_struct_layouts_match_the_header():
    structs = {"PgtgPpoExtra": _abi.PgtgPpoExtra, "PgtgPpoLog": _abi.PgtgPpoLog}
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "pgtg.h"\nint main(void) {\n'
    want = []
    for name, cls in structs.items():
        probe += f'  printf(" %zu", sizeof({name}));\n'
        want.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            probe += f'  printf(" %zu", offsetof({name}, {f}));\n'
            want.append(getattr(cls, f).offset)
    probe += '  printf(" %u %u %d", PGTG_PPO_CLIP_VF, PGTG_PPO_TARGET_KL, PGTG_ABI_VERSION);\n  return 0;\n}\n'
    want += [_abi.PGTG_PPO_CLIP_VF, _abi.PGTG_PPO_TARGET_KL, _abi.PGTG_ABI_VERSION]
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(helpers.ROOT, "include"), "-o", os.path.join(d, "p"),
                        os.path.join(d, "p.c")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def test_new_entry_points_refuse_without_a_handle():
    L = _abi.lib()
    n = C.c_uint64(0)
    assert L.pgtg_ppo_expl_var_workspace_bytes(None) == _abi.PGTG_E_INVALID
    assert L.pgtg_ppo_expl_var_workspace_bytes(C.byref(n)) == _abi.PGTG_OK and n.value > 0 and n.value % 8 == 0
    assert L.pgtg_ppo_grad_ex(None, None, None) == _abi.PGTG_E_INVALID
    assert L.pgtg_ppo_step_ex(None, None, None) == _abi.PGTG_E_INVALID
    assert L.pgtg_ppo_adv_stats_ex(None, None, None, 2, 1, 1, None, None) == _abi.PGTG_E_INVALID
    assert L.pgtg_ppo_expl_var(None, None, None, 1, None, None) == _abi.PGTG_E_INVALID
    assert L.pgtg_ppo_log(None, None, 1, 1, None, None, None) == _abi.PGTG_E_INVALID
    assert L.pgtg_ppo_perm(None, 1, 0, 0, None) == _abi.PGTG_E_INVALID
