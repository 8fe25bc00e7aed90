"""pgtg_amd/build.py builds two units, `env` per library and `train` once, and rebuilds only what an edit
reaches.  No compiler and no GPU: build.py runs in a temporary copy of the package layout (empty sources under the
real names), its subprocess.run replaced by a recorder that touches the -o file, on a clock of the test's own."""
import importlib.util
import itertools
import os
import re
import shutil
import types

import pytest

import helpers

PKG = os.path.join(helpers.ROOT, "pgtg_amd")
TRAIN_HEADERS = ["pgtg_rollout.h", "pgtg_cost.h", "pgtg_norm.h", "pgtg_eval.h", "pgtg_policy.h", "pgtg_ppo.h",
                 "pgtg_ppo_step.h", "pgtg_ppo_log.h"]
ENV_HEADERS = ["pgtg_device.h", "pgtg_records.h", "pgtg_tables.h", "pgtg_snapshot.h", "pgtg_episode.h", "pgtg_shares.h"]
VARIANTS = ("occsat", "stamps", "stampsobs")  # the default variant and two tool variants, one with two defines


class Tree:
    def __init__(self, root):
        self.root = str(root)
        self.clock = itertools.count(1_000_000_000)
        self.cmds = []
        os.makedirs(os.path.join(self.root, "pgtg_amd", "csrc"))
        os.makedirs(os.path.join(self.root, "include"))
        shutil.copy(os.path.join(PKG, "build.py"), os.path.join(self.root, "pgtg_amd", "build.py"))
        for name in os.listdir(os.path.join(PKG, "csrc")):
            self.touch("pgtg_amd", "csrc", name)
        self.touch("include", "pgtg.h")
        spec = importlib.util.spec_from_file_location("build_units_copy", os.path.join(self.root, "pgtg_amd", "build.py"))
        self.B = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(self.B)
        self.B.subprocess = types.SimpleNamespace(run=self.run)
        self.libs = [self.B.OUT, *(self.B.variant_path(v) for v in VARIANTS)]

    def touch(self, *parts):
        path = os.path.join(self.root, *parts)
        open(path, "a").close()
        t = next(self.clock)
        os.utime(path, (t, t))

    def run(self, cmd, check):
        assert check
        self.cmds.append(list(cmd))
        self.touch(cmd[cmd.index("-o") + 1])

    def build_all(self):
        self.cmds.clear()
        assert self.B.build_all(variants=VARIANTS) == self.libs
        return self.cmds

    def compiles(self, source):
        return [c for c in self.cmds if "-c" in c and any(a.endswith(os.sep + source) for a in c)]

    def links(self):
        return [c for c in self.cmds if "-shared" in c]


@pytest.fixture
def tree(tmp_path):
    return Tree(tmp_path)


def test_nothing_exists(tree):
    cmds = tree.build_all()
    env, train, links = tree.compiles("pgtg_env.hip"), tree.compiles("pgtg_train.hip"), tree.links()
    assert len(env) == len(tree.libs) and len(train) == 1 and len(links) == len(tree.libs)
    assert len(cmds) == len(env) + len(train) + len(links)
    assert all(os.path.exists(lib) for lib in tree.libs)
    # each variant's defines on that variant's env compile and on no other command
    defines = {None: [], **tree.B.VARIANTS, **tree.B.TOOL_VARIANTS}
    want = sorted(sorted(defines[v]) for v in (None, *VARIANTS))
    assert sorted(sorted(a for a in c if a.startswith("-D")) for c in env) == want
    assert not [a for c in train + links for a in c if a.startswith("-D")]
    # every library links an env object of its own and the same train object
    objs = [[a for a in c if a.endswith(".o") and ".tmp" not in a] for c in links]
    assert all(len(o) == 2 for o in objs)
    assert len({o[0] for o in objs}) == len(tree.libs) and len({o[1] for o in objs}) == 1
    # no leftovers of the temp-file step
    left = [f for d, _, fs in os.walk(tree.root) for f in fs if ".tmp" in f]
    assert not left, left


def test_up_to_date(tree):
    tree.build_all()
    assert tree.build_all() == []
    assert not any(tree.B.needs_build(lib) for lib in tree.libs)
    assert tree.B.build() == tree.B.OUT and tree.cmds == []


@pytest.mark.parametrize("header", TRAIN_HEADERS)
def test_training_header_touched(tree, header):
    tree.build_all()
    tree.touch("pgtg_amd", "csrc", header)
    assert all(tree.B.needs_build(lib) for lib in tree.libs)
    tree.build_all()
    assert not tree.compiles("pgtg_env.hip")
    assert len(tree.compiles("pgtg_train.hip")) == 1
    assert len(tree.links()) == len(tree.libs) and len(tree.cmds) == 1 + len(tree.libs)
    assert tree.build_all() == []


@pytest.mark.parametrize("header", ["pgtg_device.h", "pgtg_shares.h"])
def test_env_header_touched(tree, header):
    tree.build_all()
    tree.touch("pgtg_amd", "csrc", header)
    tree.build_all()
    assert not tree.compiles("pgtg_train.hip")
    assert len(tree.compiles("pgtg_env.hip")) == len(tree.libs)
    assert len(tree.links()) == len(tree.libs)
    assert tree.build_all() == []


@pytest.mark.parametrize("parts", [("include", "pgtg.h"), ("pgtg_amd", "csrc", "pgtg_host.h")])
def test_shared_header_touched(tree, parts):
    tree.build_all()
    tree.touch(*parts)
    tree.build_all()
    assert len(tree.compiles("pgtg_train.hip")) == 1
    assert len(tree.compiles("pgtg_env.hip")) == len(tree.libs)
    assert len(tree.links()) == len(tree.libs)


def test_needs_build_is_what_build_would_do(tree):
    """One library at a time: build(variant) runs hipcc exactly where needs_build says so, and a variant built
    after the product reuses the product's train object."""
    assert tree.B.needs_build(tree.B.OUT)
    tree.B.build()
    assert len(tree.cmds) == 3 and not tree.B.needs_build(tree.B.OUT)
    out = tree.B.variant_path("occsat")
    assert tree.B.needs_build(out)
    tree.cmds.clear()
    assert tree.B.build(variant="occsat") == out
    assert len(tree.compiles("pgtg_env.hip")) == 1 and not tree.compiles("pgtg_train.hip") and len(tree.links()) == 1
    assert "-DPGTG_OCC_MAX=2" in tree.compiles("pgtg_env.hip")[0]
    assert not tree.B.needs_build(out)
    tree.cmds.clear()
    tree.B.build(force=True)
    assert len(tree.cmds) == 3


def test_dependency_lists_cover_the_sources():
    from pgtg_amd import build as B
    named = set(B.UNITS["env"]) | set(B.UNITS["train"])
    real = {os.path.join(PKG, "csrc", f) for f in os.listdir(os.path.join(PKG, "csrc"))}
    real.add(os.path.join(helpers.ROOT, "include", "pgtg.h"))
    assert named == real, sorted(named ^ real)
    assert B.UNITS["env"][0].endswith("pgtg_env.hip") and B.UNITS["train"][0].endswith("pgtg_train.hip")
    shared = {os.path.join(PKG, "csrc", "pgtg_host.h"), os.path.join(helpers.ROOT, "include", "pgtg.h")}
    assert set(B.UNITS["env"]) & set(B.UNITS["train"]) == shared
    assert {os.path.basename(p) for p in B.UNITS["train"]} >= set(TRAIN_HEADERS)


def _includes(name):
    src = open(os.path.join(PKG, "csrc", name)).read()
    return {os.path.basename(i) for i in re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', src, re.M)}


def test_the_seam_in_the_sources():
    assert not _includes("pgtg_env.hip") & set(TRAIN_HEADERS)
    assert not _includes("pgtg_train.hip") & set(ENV_HEADERS)
    assert "pgtg_host.h" in _includes("pgtg_env.hip") and "pgtg_host.h" in _includes("pgtg_train.hip")
    # nor do the training headers reach the env's through one another
    for h in TRAIN_HEADERS:
        assert not _includes(h) & set(ENV_HEADERS), h
