"""Row layouts of the k_flatten sweep (tests/test_gpu_flatten_kernel.py) and a pure-Python statement of
which kernel variant and which chunk positions each of them reaches (tests/test_flat_layout_classes.py
checks the table against make_spec / flat_dim and that every class below is hit, without a GPU).

A layout is (n_channels, window, next_subgoal): cw2 = n * w^2 observation values, D = cw2 + 9 * nsd + 20
values per row, OB = cw2 observation bytes per env.  `classify` restates the selection in launch_flatten
(pgtg_amd/csrc/pgtg_env.hip: one pass <=> D <= 18 * 64; float pairs <=> one pass, float32 and D even)
and the chunk arithmetic of k_flatten's one-pass path: chunks of CH = 64 V values (V = 2 for pairs),
the tail (next-subgoal one-hot, position one-hots, velocity) starting in chunk pb = cw2 // CH and ending
in pb or pb + 1, chunk pb + 1 skipped when it starts at or past D.
"""
from __future__ import annotations

import random
import warnings
from typing import NamedTuple

FLAT_U = 18              # values per lane in one pass (kFlatU)
ONE_PASS = FLAT_U * 64   # the longest row written in one pass
DTYPES = ("float32", "int8")
ONE_PASS_VARIANTS = ("one", "pair")


class Layout(NamedTuple):
    n: int          # channels
    w: int          # window side: 9 the fixed tile window, else a sliding window of size (w - 1) / 2
    nsd: int        # 1 with the next-subgoal one-hot
    D: int          # hand-derived row length, checked against flat_dim(make_spec(...))
    f32: str        # hand-derived variant for float32 rows: "one", "pair" or "multi" (int8: "one" or "multi")
    default: bool = False  # the default feature list (9 real channels) instead of n generated names


# name: layout.  The comments give what each row is in the table for (cw2; chunk facts with CH = 64 and,
# for pairs, CH = 128).
LAYOUTS: dict[str, Layout] = {
    # OB % 4 of 0..3 without the one-hot (float: 0 and 2 are pairs, 1 and 3 single stores) ...
    "ob0": Layout(12, 3, 0, 128, "pair"),      # cw2 108; D % 64 == D % 128 == 0: the row ends on a chunk boundary
    "ob1": Layout(9, 3, 0, 101, "one"),        # cw2 81; tail 17..36 of chunk 1: wholly inside
    "ob2": Layout(10, 3, 0, 110, "pair"),      # cw2 90, even: no pair straddles the observation/tail boundary
    "ob3": Layout(11, 3, 0, 119, "one"),       # cw2 99
    # ... and with it, which flips the parity of D: float single stores at OB % 4 of 0 and 2, pairs at 1 and 3
    "ob0_nsd": Layout(12, 3, 1, 137, "one"),   # cw2 108; tail 44..72 of chunk 1: straddles into chunk 2
    "ob1_nsd": Layout(9, 3, 1, 110, "pair"),   # cw2 81, odd: a pair holds the last byte and the one-hot's first value
    "ob2_nsd": Layout(10, 3, 1, 119, "one"),   # cw2 90
    "ob3_nsd": Layout(11, 3, 1, 128, "pair"),  # cw2 99; D % 128 == 0
    # OB on both sides of 1 024, where the second 16-byte load (q1) starts
    "below_1024": Layout(113, 3, 0, 1037, "one"),       # cw2 1 017
    "past_1024": Layout(41, 5, 0, 1045, "one"),         # cw2 1 025: byte 1 024 comes with the byte load
    "below_1024_nsd": Layout(113, 3, 1, 1046, "pair"),
    "past_1024_nsd": Layout(41, 5, 1, 1054, "pair"),
    # cw2 576 = 9 * 64: the tail starts on a chunk boundary (single stores; for pairs cw2 = n * w^2 would have
    # to be a multiple of 128 with an odd w >= 3, so n = 128 and D > 1 152: no such one-pass row exists)
    "tail_on_chunk": Layout(64, 3, 1, 605, "one"),
    # the tail across chunks pb and pb + 1
    "straddle_single": Layout(7, 3, 0, 83, "one"),      # cw2 63: the tail starts in chunk 0's last lane
    "straddle_pair_odd": Layout(13, 3, 1, 146, "pair"),   # cw2 117; 117 + 29 > 128
    "straddle_pair_even": Layout(14, 3, 0, 146, "pair"),  # cw2 126; 126 + 20 > 128 (int8: 62 + 20 > 64)
    "smallest": Layout(1, 3, 0, 29, "one"),
    # the largest one-pass rows: the tail in the last chunk (17 of 18; pairs 8 of 9), chunk pb + 1 skipped
    "largest": Layout(125, 3, 0, 1145, "one"),          # cw2 1 125
    "largest_pair": Layout(124, 3, 0, 1136, "pair"),    # cw2 1 116
    "largest_nsd": Layout(124, 3, 1, 1145, "one"),
    # rows in passes of 1 152 values
    "first_multi": Layout(126, 3, 0, 1154, "multi"),    # cw2 1 134: the second pass holds the tail's last 2 values
    "multi_2": Layout(9, 15, 1, 2054, "multi", default=True),  # the existing several-pass layout: 2 passes
    "multi_10": Layout(128, 9, 0, 10388, "multi"),      # every channel the ABI allows, fixed window: 10 passes
    "fixed9_default": Layout(9, 9, 0, 749, "one", default=True),
    # pgtg/train.py:21-40: the default features, a sliding window of size 5, the next-subgoal one-hot
    "caller": Layout(9, 11, 1, 1118, "pair", default=True),
}


def feature_names(n: int) -> list[str]:
    """n distinct names the vocabulary does not know (legal all-zero channels: config.feature_channels),
    in an order that is not their name order (n >= 2), so that k_flatten's channel permutation is not the
    identity."""
    names = [f"ch{k:03d}" for k in range(n)]
    random.Random(n).shuffle(names)
    if n >= 2 and names == sorted(names):
        names.reverse()
    return names


def layout_kwargs(lay: Layout) -> dict:
    """make_spec / PGTGVecEnv keyword arguments of a layout: a 3 x 3 map without traffic."""
    kw: dict = dict(random_map_width=3, random_map_height=3)
    if lay.w != 9:
        assert lay.w % 2 == 1 and 3 <= lay.w < 19  # (a sliding window of size >= 9 cannot be flattened)
        kw.update(use_sliding_observation_window=True, sliding_observation_window_size=(lay.w - 1) // 2)
    if lay.nsd:
        kw["use_next_subgoal_direction"] = True
    if not lay.default:
        kw["features_to_include_in_observation"] = feature_names(lay.n)
    return kw


def layout_spec(lay: Layout):
    from pgtg_amd.config import make_spec
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return make_spec(**layout_kwargs(lay))


class RowClass(NamedTuple):
    variant: str      # "one" (one pass, single stores), "pair" (one pass, float pairs) or "multi"
    D: int
    cw2: int
    ob_mod4: int      # OB % 4: the bytes of the row's last, partial dword (the byte load)
    CH: int           # values per chunk: 64 V
    pb: int           # the chunk where the tail starts
    tail_start: int   # the tail's first value within chunk pb
    d_mod_ch: int     # D % CH: 0 = the row ends on a chunk boundary
    straddles: bool   # the tail runs on into chunk pb + 1
    skips_pb1: bool   # chunk pb + 1 starts at or past D: its store is skipped
    passes: int       # passes of 1 152 values over a row (1 for the one-pass variants)


def classify(n: int, w: int, nsd: int, dtype: str) -> RowClass:
    assert dtype in DTYPES
    cw2 = n * w * w
    tail = 9 * nsd + 20
    D = cw2 + tail
    one = D <= ONE_PASS and cw2 <= 2048
    pair = one and dtype == "float32" and D % 2 == 0
    CH = 128 if pair else 64
    pb, tail_start = divmod(cw2, CH)
    return RowClass(variant="pair" if pair else "one" if one else "multi", D=D, cw2=cw2, ob_mod4=cw2 % 4, CH=CH,
                    pb=pb, tail_start=tail_start, d_mod_ch=D % CH, straddles=tail_start + tail > CH,
                    skips_pb1=(pb + 1) * CH >= D, passes=-(-D // ONE_PASS))


def variants(dtype: str) -> tuple[str, ...]:
    """The one-pass variants a dtype has."""
    return ONE_PASS_VARIANTS if dtype == "float32" else ("one",)
