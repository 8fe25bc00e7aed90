"""ppo_reference (pgtg_amd/policy.py) against torch float64 autograd of SB3's loss, the input sets of
ppo_cases.py and their tolerance, and the C ABI of pgtg_ppo_grad (no GPU)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import helpers
import ppo_cases as ppc
from pgtg_amd import _abi
from pgtg_amd import policy as P


@pytest.mark.parametrize("D", ppc.FULL_DS + ppc.EDGE_DS)
def test_the_input_conditions_hold(D):
    c = ppc.case(D)
    assert all(c.conditions.values()), (D, c.seed, c.conditions)

@pytest.mark.parametrize("B, D", [(65, 29), (257, 29), (1, 29), (65, 17), (63, 1239)])
@pytest.mark.parametrize("norm, ent", ppc.CONFIGS)
def test_ppo_reference_is_torch_float64_autograd(B, D, norm, ent):
    c = ppc.case(D)
    g, s, _, _ = c.reference(B, norm, ent)
    tg, ts = ppc.torch_grads(c.sd, *c.batch(c.indices(B)), ppc.CLIP, ent, ppc.VF, norm, dtype=torch.float64)
    for k in ppc.KEYS:
        assert g[k].shape == tg[k].shape == P.weight_shapes(D)[k], k
        scale = max(np.abs(tg[k]).max(), 1e-300)
        assert np.abs(g[k] - tg[k]).max() <= 1e-10 * scale, (k, np.abs(g[k] - tg[k]).max(), scale)
    assert np.allclose(s[:6], ts, rtol=1e-10, atol=0), (s, ts)
    assert s[6] == s[7] == 0


def test_ppo_reference_refuses_other_rows():
    c = ppc.case(29)
    b = c.batch(c.indices(4))
    with pytest.raises(ValueError):
        P.ppo_reference(c.sd, b[0].astype(np.float32), *b[1:], 0.2, 0.0, 0.5, True)


@pytest.mark.parametrize("D", ppc.FULL_DS)
def test_bfloat16_weights_exceed_the_tolerance(D):
    c = ppc.case(D)
    B, norm, ent = 257, True, 0.01
    ref = c.reference(B, norm, ent)
    sd16 = {k: v.to(torch.bfloat16).to(torch.float32) for k, v in c.sd.items()}
    g, s = P.ppo_reference(sd16, *c.batch(c.indices(B)), ppc.CLIP, ent, ppc.VF, norm)
    d = ppc.deviations(g, s, *ref)
    over = {k: d[k] / c.e_torch[k] for k in ppc.KEYS if d[k] > ppc.MARGIN * c.e_torch[k]}
    print("ppo-tolerance bfloat16", D, {k: f"{d[k]:.2e}/{c.e_torch[k]:.2e}" for k in ppc.KEYS})
    assert over, d


def test_struct_layout_matches_header():
    fields = [f for f, _ in _abi.PgtgPpoGrad._fields_]
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "pgtg.h"\nint main(void) {\n' \
            '  printf("%zu %zu", sizeof(PgtgPpoGrad), sizeof(PgtgPpoGrads));\n' \
            + "".join(f'  printf(" %zu", offsetof(PgtgPpoGrad, {f}));\n' for f in fields) \
            + "".join(f'  printf(" %zu", offsetof(PgtgPpoGrads, {f}));\n' for f in _abi.POLICY_WEIGHT_FIELDS) \
            + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.run(["gcc", "-I", os.path.join(helpers.ROOT, "include"), "-o", os.path.join(d, "p"),
                        os.path.join(d, "p.c")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(_abi.PgtgPpoGrad), C.sizeof(_abi.PgtgPpoGrads)] \
        + [getattr(_abi.PgtgPpoGrad, f).offset for f in fields] \
        + [getattr(_abi.PgtgPpoGrads, f).offset for f in _abi.POLICY_WEIGHT_FIELDS]
    assert got == want
    assert [f for f, _ in _abi.PgtgPpoGrads._fields_] == [f for f, _ in _abi.PgtgPolicyWeights._fields_][:12]


def test_workspace_bytes_refuses_a_bad_obs_dim():
    L = _abi.lib()
    n = C.c_uint64(123)
    assert L.pgtg_ppo_workspace_bytes(0, 64, C.byref(n)) == _abi.PGTG_E_INVALID
    assert L.pgtg_ppo_workspace_bytes(_abi.PGTG_POLICY_MAX_OBS_DIM + 1, 64, C.byref(n)) == _abi.PGTG_E_INVALID
    assert L.pgtg_ppo_workspace_bytes(29, 64, None) == _abi.PGTG_E_INVALID
    assert L.pgtg_ppo_workspace_bytes(29, 1 << 60, C.byref(n)) == _abi.PGTG_E_INVALID and n.value == 123
    assert L.pgtg_ppo_workspace_bytes(29, 64, C.byref(n)) == _abi.PGTG_OK and n.value > 0 and n.value % 16 == 0
    one = n.value
    assert L.pgtg_ppo_workspace_bytes(29, 65, C.byref(n)) == _abi.PGTG_OK and n.value > one
    assert L.pgtg_ppo_workspace_bytes(_abi.PGTG_POLICY_MAX_OBS_DIM, 1, C.byref(n)) == _abi.PGTG_OK
