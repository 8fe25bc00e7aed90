"""The coverage claims of the k_flatten sweep (tests/test_gpu_flatten_kernel.py), checked without a GPU:
the layout table of tests/flat_layouts.py builds the specs it says it does, its hand-derived row lengths
and variants are what the classifier computes, and every class of row the kernel treats differently is
reached by at least one layout for each dtype and variant it applies to."""
import pytest

import helpers  # noqa: F401
from flat_layouts import DTYPES, LAYOUTS, ONE_PASS, classify, layout_spec, variants
from pgtg_amd.flat import flat_dim, flat_order


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layout_builds_the_spec_the_table_says(name):
    lay = LAYOUTS[name]
    spec = layout_spec(lay)
    assert len(spec.channels) == lay.n and spec.window == lay.w and bool(spec.next_subgoal) == bool(lay.nsd)
    assert flat_dim(spec) == lay.D
    keys = [k for k, _ in spec.channels]
    if lay.n >= 2:  # the channel permutation is not the identity
        assert keys != sorted(keys) and flat_order(spec) != list(range(lay.n))
    for dtype in DTYPES:
        c = classify(lay.n, lay.w, lay.nsd, dtype)
        assert c.D == lay.D and c.cw2 == lay.n * lay.w * lay.w
        want = lay.f32 if dtype == "float32" else ("multi" if lay.f32 == "multi" else "one")
        assert c.variant == want


def _hit(pred):
    """{(dtype, variant)} of the table's rows for which pred(row class) holds."""
    out = set()
    for lay in LAYOUTS.values():
        for dtype in DTYPES:
            c = classify(lay.n, lay.w, lay.nsd, dtype)
            if pred(c):
                out.add((dtype, c.variant))
    return out


ALL_ONE_PASS = {(d, v) for d in DTYPES for v in variants(d)}
SINGLE = {(d, "one") for d in DTYPES}
PAIR = {("float32", "pair")}
MULTI = {(d, "multi") for d in DTYPES}

# class: (predicate on the row class, the (dtype, variant) combinations that must reach it)
CLASSES = {
    **{f"OB % 4 == {m}": ((lambda c, m=m: c.ob_mod4 == m), ALL_ONE_PASS) for m in range(4)},
    "OB just below 1 024": (lambda c: 1024 - 16 < c.cw2 <= 1024, ALL_ONE_PASS),
    "OB just past 1 024": (lambda c: 1024 < c.cw2 <= 1024 + 16, ALL_ONE_PASS),
    # (pairs: cw2 = n w^2 a multiple of 128 needs n = 128, which no one-pass row has)
    "tail starts on a chunk boundary": (lambda c: c.tail_start == 0, SINGLE),
    # (float single stores have an odd D)
    "row ends on a chunk boundary": (lambda c: c.d_mod_ch == 0, {("int8", "one")} | PAIR),
    "tail wholly inside chunk pb": (lambda c: not c.straddles, ALL_ONE_PASS),
    "tail across chunks pb and pb + 1": (lambda c: c.straddles, ALL_ONE_PASS),
    "pair across the observation/tail boundary (odd cw2), tail inside": (lambda c: c.cw2 % 2 == 1 and not c.straddles, PAIR),
    "pair across the observation/tail boundary (odd cw2), tail across": (lambda c: c.cw2 % 2 == 1 and c.straddles, PAIR),
    "no pair across the boundary (even cw2), tail inside": (lambda c: c.cw2 % 2 == 0 and not c.straddles, PAIR),
    "no pair across the boundary (even cw2), tail across": (lambda c: c.cw2 % 2 == 0 and c.straddles, PAIR),
    "smallest row": (lambda c: c.D == 29, SINGLE),
    "tail in the last chunk, pb + 1 skipped": (lambda c: c.pb == ONE_PASS // c.CH - 1 and c.skips_pb1, ALL_ONE_PASS),
    "chunk pb + 1 stored": (lambda c: not c.skips_pb1, ALL_ONE_PASS),
    "D == 1 145 with the one-hot": (lambda c: c.D == 1145 and c.cw2 == 1116, SINGLE),
    "first multi-pass row": (lambda c: ONE_PASS < c.D <= ONE_PASS + 2, MULTI),
    "two passes": (lambda c: c.passes == 2 and c.D > ONE_PASS + 64, MULTI),
    "many passes": (lambda c: c.passes >= 5, MULTI),
}


@pytest.mark.parametrize("cls", list(CLASSES))
def test_every_class_is_reached(cls):
    pred, need = CLASSES[cls]
    assert need <= _hit(pred), (cls, sorted(need - _hit(pred)))


def test_named_layouts_are_in_the_table():
    """The fixed 9 x 9 window with the default features, and the caller's layout (pgtg/train.py:21-40)."""
    from pgtg_amd.config import DEFAULT_FEATURES
    for name, w, nsd in (("fixed9_default", 9, 0), ("caller", 11, 1)):
        lay = LAYOUTS[name]
        spec = layout_spec(lay)
        assert lay.default and spec.features == DEFAULT_FEATURES and (spec.window, int(spec.next_subgoal)) == (w, nsd)
    assert layout_spec(LAYOUTS["caller"]).sliding_size == 5


def test_one_pass_threshold_is_the_kernels():
    """The classifier's one-pass bound is launch_flatten's: kFlatU x 64 values, read from the source."""
    import os
    import re
    src = open(os.path.join(helpers.ROOT, "pgtg_amd", "csrc", "pgtg_env.hip")).read()
    assert int(re.search(r"constexpr int kFlatU = (\d+);", src).group(1)) * 64 == ONE_PASS
    assert "const bool one = a.D <= kFlatU * 64 && a.OB <= 2048;" in src
    assert "const bool pair = one && !h->flat_dtype && a.D % 2 == 0;" in src
