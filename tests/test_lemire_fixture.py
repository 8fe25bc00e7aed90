"""tests/golden/lemire_rejections.json (tools/find_rejection_seeds.py): every recorded seed still meets
the recorded draws in the oracle's rejection trace and gives the recorded car list, and the fixture
discriminates: an oracle built with -DORC_NO_REJECT (the rejection loop skipped, so every later draw
sits one half early) produces a different car list for the Floyd and shuffle entries."""
import ctypes as C
import json
import os
import subprocess
import warnings
import zlib

import numpy as np
import pytest

import helpers
from oracle import oracle as O

FIXTURE = os.path.join(helpers.GOLDEN, "lemire_rejections.json")


def load_fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


def spec_of(doc: dict, name: str):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return helpers.make_spec(**doc["configs"][name]["kwargs"])


def entries(doc: dict, name: str | None = None, tag: str | None = None) -> list[dict]:
    out = []
    for cname, cfg in doc["configs"].items():
        if name in (None, cname):
            out += [e for e in cfg["entries"] if tag is None or tag in e["tags"]]
    return out


def run_entry(L, cfg, e: dict, trace: bool):
    """the entry's reset (and idle steps) on library L: (crc32 of the car list, trace records of the
    last call in the fixture's form)"""
    h = L.orc_create(C.byref(cfg))
    try:
        win = L.orc_window(h)
        obs = (C.c_uint8 * (cfg.n_channels * win * win + 8))()
        out = O.OrcOut()
        recs = []
        with O.Trace(cap=256, L=L) as tr:
            assert L.orc_reset(h, e["seed"], obs, C.byref(out)) == 0
            for _ in range(e["step"]):
                tr.clear()
                assert L.orc_step(h, 4, obs, C.byref(out)) == 0 and not out.terminated
            if trace:
                recs = [{"site": r["site"], "d": r["ord"], "n": r["n"], "buffered": r["buffered"], "car": r["car"],
                         "rejects": r["rejects"]} for r in tr.records()]
        cars = (O.OrcCar * 4096)()
        n = L.orc_get_cars(h, cars, 4096)
        arr = np.array([[c.id, c.x, c.y, c.route, c.profile, c.patience, c.delay] for c in cars[:n]], np.int32)
        return zlib.crc32(arr.tobytes()), recs
    finally:
        L.orc_destroy(h)


def test_fixture_reports_its_scan():
    doc = load_fixture()
    assert set(doc["configs"]) == {"cfg3", "dense5x5", "tall_map", "wide_map"}
    for name, cfg in doc["configs"].items():
        assert cfg["resets_refused"] == 0, name
        for q, s in cfg["sites"].items():
            assert s["seeds_scanned"] > 0 and s["kept"] <= s["found"], (name, q)
            assert (q in cfg["not_reached"]) == (s["kept"] < s["wanted"]), (name, q)
        # the rejection proper was reached by directed seeds in every configuration
        assert "floyd" not in cfg["not_reached"] and "shuffle" not in cfg["not_reached"], name


def test_entries_reproduce_in_the_oracle():
    doc = load_fixture()
    L = O.lib()
    for name in doc["configs"]:
        cfg = O.config_from_spec(spec_of(doc, name))
        for e in entries(doc, name):
            crc, recs = run_entry(L, cfg, e, trace=True)
            if e["step"] > 0:
                recs = [r for r in recs if r["site"] == "car_pass"]
            assert recs == e["draws"], (name, e["seed"], e["step"])
            assert crc == e["crc32"], (name, e["seed"], e["step"])


@pytest.fixture(scope="module")
def no_reject_lib(tmp_path_factory):
    """the oracle with Lemire's rejection loop compiled out (-DORC_NO_REJECT; no other build has it)"""
    d = tmp_path_factory.mktemp("orc_no_reject")
    so = str(d / "liboracle_no_reject.so")
    src = os.path.join(O.HERE, "pgtg_oracle.c")
    subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-fPIC", "-std=gnu11", "-ffp-contract=off", "-DORC_NO_REJECT",
                    "-shared", "-o", so, src, "-lm"], check=True)
    return O.load(so)


def test_fixture_discriminates(no_reject_lib):
    """Without the rejection loop the Floyd and shuffle entries give another car list.  A shifted
    stream can select the same cars by chance, so up to one entry in ten may coincide; the seeds of
    the bench shape (cfg3) are expected not to.  Coinciding entries found when the fixture was
    made: 0 of the 38 Floyd and shuffle entries of the four configurations."""
    doc = load_fixture()
    total, same = 0, []
    for name in doc["configs"]:
        cfg = O.config_from_spec(spec_of(doc, name))
        for e in entries(doc, name):
            if e["step"] == 0 and any(r["site"] in ("floyd", "shuffle") and r["rejects"] > 0 for r in e["draws"]):
                total += 1
                crc, _ = run_entry(no_reject_lib, cfg, e, trace=False)
                if crc == e["crc32"]:
                    same.append((name, e["seed"]))
    print(f"discrimination: {len(same)} of {total} entries coincide: {same}")
    assert total >= 4 * 9
    assert len(same) * 10 <= total, same
    assert not [s for s in same if s[0] == "cfg3"], same
