"""Cases for the baseline window [start, min(end, L)) on every route that computes it.

The layouts, their records (dips anywhere, the edge samples included) and the route names are those of
tests/test_hip_layout_routes.py; what varies here is the window: inside a 16-byte chunk, across the 32-sample round of
the span16 kernel's per-record sum, around the record end, empty by the clamp, and -- on the ragged run -- empty for some
records only.  The reference is the integer rule itself: int(sum of the samples) / count, Python's correctly rounded
division of two integers below 2**53, which is np.mean over float64 of integer samples and the kernels'
(double)sum / (double)n.  tests/test_baseline_window_cpu.py proves the cases without a GPU,
tests/test_hip_baseline_window.py runs them."""

import functools
import re

import numpy as np

from oracle import wfa_oracle as O
from tests import test_hip_layout_routes as LR
from waveformanalysis_amd import synth

LAYOUTS = ("L64", "L80", "L88", "L72", "L40", "L68", "L24", "ragged", "L64off4", "L64mixed")
SG_SLOW = (21, 4)                      # a plan outside the fast set: the pass takes k_hits<sg_fused,baseline> by itself
SELECTORS = LR.OPTIONS + ("sg21_4",)   # "", no_runs32, no_pad, no_span, no_fast, and the plan above without any option
FAST = ("", "no_runs32", "no_pad", "no_span")          # selectors whose rows are byte-identical among each other
CONTROL = (0, synth.BASELINE_SAMPLES)
I32_MAX = 2**31 - 1
THRESHOLD = 10.0


def max_len(name):
    m = re.match(r"L(\d+)", name)
    return int(m.group(1)) if m else 64


def window_groups(name):
    """{group: [windows]} of one layout.  A chunk-edge or round-edge window fits when it ends inside the longest
    record; the other groups are functions of L and always fit."""
    L = max_len(name)
    fits = lambda ws: [w for w in ws if w[1] <= L]
    groups = {
        "chunk edges": fits([(0, 1), (0, 8), (0, 9), (7, 8), (7, 9), (8, 16), (5, 29)]),
        "round edges": fits([(0, 32), (0, 33), (31, 33), (32, 40), (33, 34), (24, 72)]),
        "control": [CONTROL],
        "record end": [(0, L - 1), (0, L), (0, L + 1), (1, L), (L - 1, L), (L - 1, I32_MAX)],
        "empty by clamp": [(L, L + 8), (L + 5, L + 70)],
    }
    if name == "ragged":
        # (39, 41) starts inside the shortest record (lengths 40..64), so it mixes one- and two-sample means but gives
        # no NaN; (40, 42) is the same edge one sample on, where the records of 40 samples are NaN
        groups["ragged only"] = [(44, 52), (39, 41), (40, 42), (63, 64)]
    return {g: ws for g, ws in groups.items() if ws}


def windows(name):
    seen = []
    for ws in window_groups(name).values():
        seen += [w for w in ws if w not in seen]
    return seen


def plan_of(selector):
    return SG_SLOW if selector == "sg21_4" else (11, 2)


def reference(rec, pool, window):
    """Baseline of every record by the stated rule."""
    s, e = window
    out = np.full(len(rec), np.nan, dtype=np.float64)
    for i in range(len(rec)):
        o, L = int(rec["wave_offset"][i]), int(rec["event_length"][i])
        e1 = min(e, L)
        if e1 > s:
            out[i] = int(pool[o + s : o + e1].sum(dtype=np.int64)) / (e1 - s)
    return out


@functools.lru_cache(maxsize=None)
def filtered(name, plan=(11, 2)):
    rec, pool, _want, filt = LR._case(name)
    if plan == (11, 2):
        return filt
    out = O.filter_wave_pool(rec, pool, sg_window_size=plan[0], sg_poly_order=plan[1])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(name, window, plan=(11, 2)):
    """(records carrying the reference baselines, pool, oracle rows) of one layout and window; computed once and shared
    by every route selector."""
    rec, pool, _want, _filt = LR._case(name)
    rec_ref = rec.copy()
    rec_ref["baseline"] = reference(rec, pool, window)
    want = O.threshold_hits(rec_ref, filtered(name, plan), threshold=THRESHOLD)
    for a in (rec_ref, want):
        a.setflags(write=False)
    return rec_ref, pool, want


def expected_stage(name, selector, window):
    """Stage kernels of the fused pass.  The streaming kernel takes the window (0, 40) only: on the layouts that reach
    it, every other window falls to the span16 kernel (in place, or on the padded shadow with k_pad_rows in front), or
    to k_sg_mask where the option forbids the span kernels."""
    if selector in ("no_fast", "sg21_4"):
        return LR.LITERAL
    route = LR.ROUTES[name][0][selector]
    if window == CONTROL or route not in (LR.RUNS, LR.RUNS_PAD):
        return route
    if selector == "no_span":
        return LR.MASK
    return LR.SPAN16 if route == LR.RUNS else LR.SPAN16_PAD


# ---- the 32-bit case: a window whose sum does not fit an int ---------------------------------------------------------
BIG_R = 66                             # two spans of the span16 kernel, the second with 2 records
BIG_LAYOUTS = {"L32784": 32_784,       # L % 16 == 0, L % 32 != 0: span16 in place
               "L32790": 32_790}       # L % 16 == 6 >= H of SG(11,2): span16 on the padded shadow
FULL = 0xFFFF
BIG_EDGE = 32_769                      # 32 769 * 0xFFFF = 2 147 516 415 > 2**31 - 1


def big_windows(name):
    return [(0, BIG_EDGE - 1), (0, BIG_EDGE), (0, BIG_LAYOUTS[name])]


@functools.lru_cache(maxsize=None)
def big_case(name, window):
    """Records of 0xFFFF with three 10-sample dips of depth 2000 each.  For (0, 32 769) the dips start behind sample
    32 769 (the L - 32 769 samples left there make them overlap), so the window's sum is exactly 32 769 * 0xFFFF; for
    the other windows they lie anywhere."""
    L = BIG_LAYOUTS[name]
    rec, _pool = synth.make_run(BIG_R, "vx2730", cfg=900 + L % 100, L=L)
    w = np.full((BIG_R, L), FULL, dtype=np.int32)
    rng = np.random.default_rng(L + window[1])
    for i in range(BIG_R):
        if window[1] == BIG_EDGE:
            starts = (BIG_EDGE, (BIG_EDGE + L - 10) // 2, L - 10)
        else:
            starts = rng.integers(0, L - 10, 3)
        for a in starts:
            w[i, int(a) : int(a) + 10] -= 2000
    pool = w.astype(np.uint16).reshape(-1)
    rec_ref = rec.copy()
    rec_ref["baseline"] = reference(rec, pool, window)
    want = O.threshold_hits(rec_ref, O.filter_wave_pool(rec_ref, pool), threshold=THRESHOLD)
    for a in (rec_ref, pool, want):
        a.setflags(write=False)
    return rec_ref, pool, want
