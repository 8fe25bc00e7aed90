"""Build the in-tree HIP library for gfx950 (and nothing else): `python -m pgtg_amd.build`.

The library is two translation units, compiled to objects under pgtg_amd/obj/ and linked: `env`, once per
variant of the library (the -DPGTG_* builds of the environment's kernels), and `train`, once in all and linked
into every one of them ("Two translation units")."""
from __future__ import annotations

import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(PKG, "libpgtg_hip.so")
OBJ = os.path.join(PKG, "obj")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-Wall", "-Wno-unused-function"]


def _csrc(*names: str) -> list[str]:
    return [os.path.join(PKG, "csrc", n) for n in names]


# A unit's source, then the headers it includes.  An edit of a training header recompiles `train` alone.
_BOTH = _csrc("pgtg_host.h") + [os.path.join(os.path.dirname(PKG), "include", "pgtg.h")]
UNITS = {
    "env": _csrc("pgtg_env.hip", "pgtg_device.h", "pgtg_records.h", "pgtg_tables.h", "pgtg_episode.h",
                 "pgtg_snapshot.h", "pgtg_shares.h") + _BOTH,
    "train": _csrc("pgtg_train.hip", "pgtg_rollout.h", "pgtg_cost.h", "pgtg_norm.h", "pgtg_eval.h", "pgtg_policy.h",
                   "pgtg_ppo.h", "pgtg_ppo_step.h", "pgtg_ppo_log.h") + _BOTH,
}

# test variant: occupancy counters saturating at 2 cars so that the exact-recount path runs often
# (tests/test_gpu_occupancy.py replays the traffic trajectories through it)
VARIANTS = {"occsat": ["-DPGTG_OCC_MAX=2"]}
# A/B and diagnostic build (tools/*.sh): reads the PGTG_SPREAD/COMPACT/QUEUE/LINEMASK/DIAG knobs from
# the environment; the product library reads none.  Not built by default (PGTG_LIB selects it).
TOOL_VARIANTS = {"tuning": ["-DPGTG_TUNING"], "stamps": ["-DPGTG_STAMPS"], "ntobs": ["-DPGTG_NT_OBS"],
                 "stampsobs": ["-DPGTG_STAMPS", "-DPGTG_STAMPS_OBS"]}


def variant_path(name: str) -> str:
    return os.path.join(PKG, f"libpgtg_hip_{name}.so")


def _objects(out: str) -> dict[str, str]:
    """The objects library `out` links, by unit: an env object of its own and the one train object."""
    return {"env": os.path.join(OBJ, os.path.basename(out)[:-len(".so")] + ".env.o"),
            "train": os.path.join(OBJ, "train.o")}


def _stale(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def needs_build(out: str = OUT) -> bool:
    """Whether a source of either unit, or an object left by an earlier build, is newer than the library.  (The
    objects are intermediates: a library newer than every source is up to date without them.)"""
    return _stale(out, UNITS["env"] + UNITS["train"] + [o for o in _objects(out).values() if os.path.exists(o)])


def _hipcc(args: list[str], target: str, verbose: bool) -> None:
    root, ext = os.path.splitext(target)
    tmp = f"{root}.tmp{os.getpid()}{ext}"  # (keeps the extension: .gitignore covers it if the build is interrupted)
    cmd = [HIPCC, *args, "-o", tmp]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(tmp, target)  # atomic: a concurrent loader or linker never sees a partial file


def _make(variants, force: bool, verbose: bool) -> list[str]:
    """(Re)build the libraries of `variants` (None: the product) whose sources are newer: the stale objects
    among theirs compiled concurrently, then a link each.  Serialised by a file lock so that the ranks of a
    multi-process run can all call it: one compiles, the others wait and find everything up to date."""
    import fcntl
    from concurrent.futures import ThreadPoolExecutor
    defines = {None: [], **VARIANTS, **TOOL_VARIANTS}
    outs = {v: OUT if v is None else variant_path(v) for v in variants}
    os.makedirs(OBJ, exist_ok=True)
    with open(os.path.join(PKG, "build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            todo = [v for v in variants if force or needs_build(outs[v])]
            compiles = {}  # object -> hipcc arguments; the train object once, whichever libraries want it
            for v in todo:
                for unit, obj in _objects(outs[v]).items():
                    if force or _stale(obj, UNITS[unit]):
                        extra = defines[v] if unit == "env" else []
                        compiles[obj] = [*(f for f in FLAGS if f != "-shared"), *extra, "-c", UNITS[unit][0]]
            with ThreadPoolExecutor(max_workers=max(1, len(compiles))) as ex:  # (at most an env object each + train)
                for f in [ex.submit(_hipcc, args, obj, verbose) for obj, args in compiles.items()]:
                    f.result()
            for v in todo:
                _hipcc([FLAGS[0], "-shared", "-fPIC", *_objects(outs[v]).values()], outs[v], verbose)
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)
    return [outs[v] for v in variants]


def build(force: bool = False, verbose: bool = False, variant: str | None = None) -> str:
    """(Re)build the product library, or a variant of it, if a source is newer."""
    return _make((variant,), force, verbose)[0]


def build_all(force: bool = False, verbose: bool = False, variants=tuple(VARIANTS)) -> list[str]:
    """The product library and the given variants: one hipcc per stale object at a time, then the links."""
    return _make((None, *variants), force, verbose)


if __name__ == "__main__":
    tools = [a.split("=", 1)[1].split(",") for a in sys.argv if a.startswith("--tools=")]
    print("\n".join(build_all(force="--force" in sys.argv, verbose=True,
                               variants=tuple(VARIANTS) + tuple(tools[0] if tools else ()))))
