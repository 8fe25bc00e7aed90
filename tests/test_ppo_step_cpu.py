"""policy_adam_reference (pgtg_amd/policy.py) against torch's clip_grad_norm_ + torch.optim.Adam at float64, and
the C ABI of pgtg_ppo_step, pgtg_ppo_step_workspace_bytes and pgtg_ppo_adv_stats (no GPU)."""
import ctypes as C
import math
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

BETAS = (0.9, 0.999)


def made_up_grads(sd, seed, norm):
    """Normal gradients of the state dict's shapes, scaled to a total norm of `norm`."""
    g = torch.Generator().manual_seed(seed)
    out = {k: torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in sd.items()}
    total = math.sqrt(sum(float((x * x).sum()) for x in out.values()))
    return {k: (x * (norm / total)).to(torch.float32) for k, x in out.items()}


def torch_steps(sd, grad_list, lr, eps, max_norm, dtype):
    """clip_grad_norm_ + Adam over the gradients in turn on CPU tensors of dtype; per step (p, m, v, total)."""
    params = {k: torch.nn.Parameter(v.detach().clone().to(dtype)) for k, v in sd.items()}
    opt = torch.optim.Adam(params.values(), lr=lr, betas=BETAS, eps=eps)
    out = []
    for grads in grad_list:
        for k, p in params.items():
            p.grad = grads[k].detach().clone().to(dtype)
        total = torch.nn.utils.clip_grad_norm_(params.values(), max_norm)
        opt.step()
        st = opt.state_dict()["state"]
        out.append(({k: p.detach().clone().numpy() for k, p in params.items()},
                    {k: st[i]["exp_avg"].clone().numpy() for i, k in enumerate(params)},
                    {k: st[i]["exp_avg_sq"].clone().numpy() for i, k in enumerate(params)}, float(total)))
    return out


@pytest.mark.parametrize("eps", [1e-5, 1e-8])
@pytest.mark.parametrize("max_norm, norms", [(0.5, (3.0, 0.1, 0.7)), (0.5, (0.2, 0.3, 0.4)), (math.inf, (3.0, 0.1, 40.0))])
@pytest.mark.parametrize("D", [17, 29])
def test_policy_adam_reference_is_torch_float64(D, max_norm, norms, eps):
    sd = ppc.case(D).sd
    grad_list = [made_up_grads(sd, 100 * D + i, n) for i, n in enumerate(norms)]
    want = torch_steps(sd, grad_list, 3e-4, eps, max_norm, torch.float64)
    p = {k: v.double().numpy() for k, v in sd.items()}
    m = {k: np.zeros_like(x) for k, x in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    for step, (grads, (wp, wm, wv, wt)) in enumerate(zip(grad_list, want), start=1):
        p, m, v, total = P.policy_adam_reference(p, grads, m, v, step, 3e-4, BETAS, eps, max_norm)
        assert abs(total - wt) <= 1e-12 * wt
        assert (total > max_norm) == (norms[step - 1] > max_norm)  # (the case clips where it was made to)
        for got, ref, name in ((p, wp, "p"), (m, wm, "m"), (v, wv, "v")):
            for k in ref:
                assert got[k].dtype == np.float64 and got[k].shape == ref[k].shape
                scale = np.abs(ref[k]).max()
                assert np.abs(got[k] - ref[k]).max() <= 1e-12 * scale, (step, name, k)


def test_zero_gradient_at_step_one_changes_nothing():
    sd = ppc.case(17).sd
    for dtype in (np.float64, np.float32):
        p0 = {k: v.numpy().astype(dtype) for k, v in sd.items()}
        z = {k: np.zeros_like(x) for k, x in p0.items()}
        p, m, v, total = P.policy_adam_reference(p0, z, z, z, 1, 3e-4, BETAS, 1e-5, 0.5, dtype=dtype)
        assert total == 0
        for k in p0:
            assert np.array_equal(p[k], p0[k]) and p[k].dtype == dtype
            assert not m[k].any() and not v[k].any()
            assert np.isfinite(p[k]).all()
    with pytest.raises(ValueError):
        P.policy_adam_reference(p0, z, z, z, 0, 3e-4, BETAS, 1e-5, 0.5)


def test_struct_layout_matches_header():
    fields = [f for f, _ in _abi.PgtgPpoStep._fields_]
    probe = '#include <stdio.h>\n#include <stddef.h>\n#include "pgtg.h"\nint main(void) {\n' \
            '  printf("%zu %zu", sizeof(PgtgPpoStep), sizeof(PgtgPpoConstGrads));\n' \
            + "".join(f'  printf(" %zu", offsetof(PgtgPpoStep, {f}));\n' for f in fields) \
            + "".join(f'  printf(" %zu", offsetof(PgtgPpoConstGrads, {f}));\n' for f in _abi.POLICY_WEIGHT_FIELDS) \
            + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(probe)
        subprocess.run(["gcc", "-I", os.path.join(helpers.ROOT, "include"), "-o", os.path.join(d, "p"),
                        os.path.join(d, "p.c")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(_abi.PgtgPpoStep), C.sizeof(_abi.PgtgPpoGrads)] \
        + [getattr(_abi.PgtgPpoStep, f).offset for f in fields] \
        + [getattr(_abi.PgtgPpoGrads, f).offset for f in _abi.POLICY_WEIGHT_FIELDS]
    assert got == want


def test_step_workspace_bytes():
    L = _abi.lib()
    n = C.c_uint64(123)
    assert L.pgtg_ppo_step_workspace_bytes(0, C.byref(n)) == _abi.PGTG_E_INVALID
    assert L.pgtg_ppo_step_workspace_bytes(_abi.PGTG_POLICY_MAX_OBS_DIM + 1, C.byref(n)) == _abi.PGTG_E_INVALID
    assert L.pgtg_ppo_step_workspace_bytes(29, None) == _abi.PGTG_E_INVALID and n.value == 123
    assert L.pgtg_ppo_step_workspace_bytes(29, C.byref(n)) == _abi.PGTG_OK and n.value > 0 and n.value % 16 == 0
    small = n.value
    assert L.pgtg_ppo_step_workspace_bytes(1239, C.byref(n)) == _abi.PGTG_OK and n.value >= small
    big = n.value
    # the grid is capped: the largest obs_dim asks for no more than D = 1239 does
    assert L.pgtg_ppo_step_workspace_bytes(_abi.PGTG_POLICY_MAX_OBS_DIM, C.byref(n)) == _abi.PGTG_OK and n.value == big


def test_refusals_without_a_device():
    """Without a handle every call is refused before anything is dereferenced or launched, whatever else is
    wrong with it (the refusals' messages need a handle: test_gpu_ppo_step.py)."""
    L = _abi.lib()
    buf = (C.c_float * 64)()
    ptr = C.addressof(buf)
    tensors = _abi.PgtgPpoGrads(*([ptr] * 12))
    good = dict(obs_dim=29, params=tensors, grads=tensors, exp_avg=tensors, exp_avg_sq=tensors, packed=ptr, workspace=ptr,
                step=1, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5, grad_norm=ptr)
    bad = [{}, dict(obs_dim=0), dict(obs_dim=_abi.PGTG_POLICY_MAX_OBS_DIM + 1), dict(packed=None), dict(workspace=None),
           dict(packed=ptr + 4), dict(workspace=ptr + 4), dict(step=0), dict(lr=math.nan), dict(eps=math.inf), dict(beta1=1.0), dict(beta2=-0.1),
           dict(max_grad_norm=0.0), dict(max_grad_norm=math.nan), dict(params=_abi.PgtgPpoGrads())]
    for over in bad:
        a = _abi.PgtgPpoStep(**{**good, **over})
        assert L.pgtg_ppo_step(None, C.byref(a)) == _abi.PGTG_E_INVALID, over
    assert L.pgtg_ppo_step(None, None) == _abi.PGTG_E_INVALID
    for args in ((ptr, ptr, 64, 3, 96, ptr), (None, ptr, 64, 3, 96, ptr), (ptr, None, 64, 3, 96, ptr), (ptr, ptr, 64, 3, 96, None),
                 (ptr, ptr, 1, 3, 96, ptr), (ptr, ptr, 0, 3, 96, ptr), (ptr, ptr, 64, 0, 96, ptr), (ptr, ptr, 64, 3, 0, ptr),
                 (ptr, ptr, 64, 1 << 62, 1 << 62, ptr)):
        assert L.pgtg_ppo_adv_stats(None, *args) == _abi.PGTG_E_INVALID, args
    assert not any(buf)
