"""Cost of the device-resident snapshots (include/pgtg.h pgtg_snapshot_*, the kernel k_state_copy).

Per workload, on one handle after a short warm rollout:
  * save all + load all, timed with HIP events on the handle's stream (the map-ring fill that both calls
    begin with included), warm, the median of `--runs` runs, beside the byte model: each call reads and
    writes bytes_per_env x N, so the pair moves 4 x bytes_per_env x N over the measured stream-copy rate
    (pgtg_measure_hbm counts read + write bytes);
  * a fork of `--roots` saved envs into `--copies` envs each (pgtg_amd.vector.fork_indices);
  * the host round trip it replaces: dump_state + load_state, wall clock;
  * the bytes of every state section per env (from the blob's table), largest first.
`--blob-only` measures the round trip alone (for a library of an earlier ABI, PGTG_LIB + PGTG_ABI_COMPAT).

    python tools/snapshot_cost.py [--workloads cfg5,train] [--runs 9] [--out FILE] [--blob-only]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def section_bytes(blob, n):
    """{section id: bytes per env} from a pgtg_dump_state blob's table (the batch-wide counters left out)."""
    import numpy as np
    hdr = 56
    n_sec = int(np.frombuffer(blob[16:20].tobytes(), np.uint32)[0])
    ent = np.frombuffer(blob[hdr:hdr + 16 * n_sec].tobytes(), dtype=[("id", "<u4"), ("pad", "<u4"), ("bytes", "<u8")])
    return {int(e["id"]): int(e["bytes"]) / n for e in ent if int(e["id"]) != 5}


def main():
    import torch

    import bench
    from pgtg_amd import _abi
    from pgtg_amd.config import make_spec
    from pgtg_amd.vector import PGTGVecEnv, fork_indices
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg5,train")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--roots", type=int, default=4096)
    ap.add_argument("--copies", type=int, default=16)
    ap.add_argument("--envs", type=int, default=0)
    ap.add_argument("--blob-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        """Median milliseconds of fn() between two events on the current stream, after two warm calls."""
        for _ in range(2):
            fn()
        ms = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    gbs = C.c_double()
    rc = _abi.lib().pgtg_measure_hbm(0, 1 << 30, 20, C.byref(gbs))
    assert rc == 0, rc
    for name in args.workloads.split(","):
        _, _, n, kw = bench.WORKLOADS[name]
        kw = dict(kw)
        n = args.envs or n
        limit = kw.pop("max_episode_steps", None)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec = make_spec(**kw)
        env = PGTGVecEnv(n, spec=spec, device=0, autoreset=True, max_episode_steps=limit)
        env.reset(seed=0)
        env.step_many(env.random_actions(10, seed=1))
        torch.cuda.synchronize()
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            blob = env.dump_state()
            env.load_state(blob, observe=False)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        out = {"workload": name, "envs": n, "kernel": env.step_kernel(), "abi": int(os.environ.get("PGTG_ABI_COMPAT") or
                                                                                   _abi.PGTG_ABI_VERSION),
               "dump_load_state_wall_ms_median": round(statistics.median(wall), 2), "dump_load_state_wall_ms": [round(w, 2) for w in wall],
               "blob_bytes": int(blob.size), "copy_gbs": round(gbs.value, 1)}
        if not args.blob_only:
            sec = section_bytes(blob, n)
            snap = env.snapshot()
            bpe = snap.bytes_per_env
            assert abs(sum(sec.values()) - bpe) < 1e-6, (sum(sec.values()), bpe)

            def save_load():
                snap.save(env)
                snap.load(env, observe=False, check=False)

            both = timed(save_load)
            save = timed(lambda: snap.save(env))
            model_ms = 4 * bpe * n / (gbs.value * 1e9) * 1e3
            out.update({"bytes_per_env": bpe, "snapshot_device_bytes": snap.nbytes,
                        "save_load_ms_median": round(both[0], 4), "save_load_ms_min_max": [round(both[1], 4), round(both[2], 4)],
                        "save_ms_median": round(save[0], 4),
                        "byte_model_ms": round(model_ms, 4), "byte_model": "4 x bytes_per_env x N / copy_gbs (read + write bytes)",
                        "fraction_of_copy_rate": round(model_ms / both[0], 3),
                        "sections_bytes_per_env": {str(k): v for k, v in sorted(sec.items(), key=lambda kv: -kv[1])}})
            snap.close()
            # a fork: `roots` saved envs into `copies` envs each
            roots, copies = min(args.roots, n // args.copies), args.copies
            fs = env.snapshot(roots)
            slot_idx, env_idx = fork_indices(torch.arange(roots, device=env.device), copies)
            slot_idx, env_idx = slot_idx.to(torch.int32), env_idx.to(torch.int32)
            fs.save(env, env_idx=torch.arange(roots, device=env.device))
            fork = timed(lambda: fs.load(env, slot_idx, env_idx, observe=False, check=False))
            fork_model = (roots + roots * copies) * bpe / (gbs.value * 1e9) * 1e3  # read each root once, write every copy
            out.update({"fork_roots": roots, "fork_copies": copies, "fork_load_ms_median": round(fork[0], 4),
                        "fork_load_ms_min_max": [round(fork[1], 4), round(fork[2], 4)],
                        "fork_byte_model_ms": round(fork_model, 4),
                        "fork_fraction_of_copy_rate": round(fork_model / fork[0], 3)})
            fs.close()
        emit(out)
        env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
