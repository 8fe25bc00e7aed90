"""Build and load the stand-alone device-RNG probe (tests/csrc/rng_probe.hip) with the product
library's compiler flags, into pgtg_amd/librng_probe.so (git-ignored, beside the other libraries).
Test infrastructure: the product never loads it."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from pgtg_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "rng_probe.hip")
DEPS = [SRC, os.path.join(B.PKG, "csrc", "pgtg_device.h"), os.path.join(B.PKG, "csrc", "pgtg_records.h"),
        os.path.join(os.path.dirname(B.PKG), "include", "pgtg.h")]
OUT = os.path.join(B.PKG, "librng_probe.so")


def build(force: bool = False, verbose: bool = False) -> str:
    import fcntl
    with open(OUT + ".lock", "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            stale = not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS)
            if force or stale:
                tmp = OUT + f".tmp{os.getpid()}"
                cmd = [B.HIPCC, *B.FLAGS, "-o", tmp, SRC]
                if verbose:
                    print(" ".join(cmd), flush=True)
                subprocess.run(cmd, check=True)
                os.replace(tmp, OUT)
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)
    return OUT


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.rng_probe_run.restype = C.c_int
        L.rng_probe_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        L.rng_probe_tables_bytes.restype = C.c_int
        L.rng_probe_tables_bytes.argtypes = []
        _lib = L
    return _lib
