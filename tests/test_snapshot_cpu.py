"""The host side of the device-resident snapshots, no GPU: the library exports the pgtg_snapshot_*
entry points of ABI 9, and fork_indices (pgtg_amd/vector.py) against a numpy restatement."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers
from pgtg_amd import _abi, build

SNAPSHOT_ABI = ["pgtg_snapshot_bytes", "pgtg_snapshot_create", "pgtg_snapshot_destroy", "pgtg_snapshot_load",
                "pgtg_snapshot_save"]


def test_library_exports_the_snapshot_entry_points():
    syms = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pgtg_\w+)", syms))
    assert [f for f in SNAPSHOT_ABI if f not in exported] == []
    assert [f for f in SNAPSHOT_ABI if f not in _abi.EXPORTED] == []
    L = _abi.lib()
    for f in SNAPSHOT_ABI:
        assert getattr(L, f).argtypes is not None, f


def test_abi_version_is_9_in_header_and_mirror():
    src = open(os.path.join(helpers.ROOT, "include", "pgtg.h")).read()
    assert re.search(r"^#define PGTG_ABI_VERSION 9$", src, re.M)
    assert _abi.PGTG_ABI_VERSION == 9


def _fork_indices_np(roots, copies):
    roots = np.asarray(roots, dtype=np.int64).reshape(-1)
    slot = np.repeat(roots, copies)
    env = np.concatenate([np.arange(r * copies, r * copies + copies) for r in roots]) if roots.size else np.zeros(0, np.int64)
    return slot, env.astype(np.int64)


@pytest.mark.parametrize("roots, copies", [(list(range(5)), 3), ([4, 0, 2], 16), (list(range(7)), 1), ([], 4), ([3], 1),
                                           (np.arange(4096), 16)])
def test_fork_indices_matches_numpy(roots, copies):
    from pgtg_amd import fork_indices
    from pgtg_amd.vector import fork_indices as same
    assert fork_indices is same
    slot, env = fork_indices(roots, copies)
    want_slot, want_env = _fork_indices_np(roots, copies)
    assert slot.dtype == env.dtype == torch.int64 and slot.device.type == env.device.type == "cpu"
    assert np.array_equal(slot.numpy(), want_slot) and np.array_equal(env.numpy(), want_env)
    # consecutive roots fill a batch of len(roots) * copies envs, every env once
    if len(roots) and list(roots) == list(range(len(roots))):
        assert np.array_equal(env.numpy(), np.arange(len(roots) * copies))
    # a tensor of roots gives the same indices
    s2, e2 = fork_indices(torch.as_tensor(np.asarray(roots, dtype=np.int64)), copies)
    assert torch.equal(s2, slot) and torch.equal(e2, env)


def test_fork_indices_refuses_no_copies():
    from pgtg_amd.vector import fork_indices
    with pytest.raises(ValueError):
        fork_indices([0, 1], 0)
