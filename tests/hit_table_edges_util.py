"""Hit tables that put the hit-table stages of wfa_hits.hip (lexsort, k_hit_prep / k_float_keys, k_event_flags,
k_merge_chain, k_merge_emit, wfa_records_sort) on their key, window and summation edges, and a second, independent
restatement of the reference rules in plain Python.

The oracle (oracle/wfa_oracle.py) restates the reference with numpy (np.lexsort, np.argsort, np.sum); the models here use
python ints and floats, `sorted` with tuple keys and an explicit pairwise tree, so that the expected values the GPU is
compared with are cross-checked on the CPU by something that shares no sorting or summation code with them.  The models
also count how often a comparison is met exactly at, and one quantum either side of, its boundary, and carry switches
for the ways a kernel could be subtly wrong (`MUTANTS`): `test_hit_table_edges_cpu.py` proves with them that the tables
do reach their edges and do tell right from wrong; `test_hip_hit_table_edges.py` runs the tables through the kernels.

Builders (every one deterministic, no GPU, no torch):
  A key_route          the `crafted` layout of test_hip_hits.py based at timestamps on both sides of the 4.0e18 key switch
  B window_boundaries  event chains with starts exactly at / one quantum around running_max_end + window
  C merge_boundaries   gap == merge_gap, total == cap, dt changes, shadowed chains, one long segment, many segments
  D key_extremes       type extremes, constant keys, block and grid edges of k_key_ranges; record_sort_columns likewise
  E fixed_windows      abs_start_fix / abs_end_fix: fractional, negative, far away, +0.0 / -0.0
  F integral_ties      clusters whose float32 integral depends on the order of the float64 additions
  G anchor_ties        anchor ties, clusters over two records, clamped widths
"""

from __future__ import annotations

import math

import numpy as np

from waveformanalysis_amd.dtypes import THRESHOLD_HIT_DTYPE

KEY_SWITCH = 4.0e18          # k_hit_prep: |abs_start| >= this raises *inexact (float keys for the whole table)
COMPARABLE_END = 2**63 - 2048  # beyond this int(np.max(abs_end)) no longer fits int64 in the reference itself
I16 = (-32768, -1, 0, 32767)
I32 = (-2**31, -1, 0, 2**31 - 1)
I64 = (-2**63, -1, 0, 2**63 - 1)
DT_EXTREMES = (1, 2, 4, 2**31 - 1)


# ---- the reference rules once more, in plain Python -----------------------------------------------------------------------
def abs_windows(hits, fix0=None, fix1=None):
    """([abs_start], [abs_end]) as python floats: float(ts) + (float(edge) - float(pos)) * (float(dt) * 1e3); a non-NaN
    fix replaces the value (k_hit_prep, wfa_hits.hip:179-182)."""
    a0, a1 = [], []
    for i in range(len(hits)):
        t, p, dps = float(int(hits["timestamp"][i])), float(int(hits["position"][i])), float(int(hits["dt"][i])) * 1e3
        s = t + (float(int(hits["edge_start"][i])) - p) * dps
        e = t + (float(int(hits["edge_end"][i])) - p) * dps
        if fix0 is not None and not math.isnan(fix0[i]):
            s = float(fix0[i])
        if fix1 is not None and not math.isnan(fix1[i]):
            e = float(fix1[i])
        a0.append(s)
        a1.append(e)
    return a0, a1


def _zero_rank(v):
    """-0.0 before +0.0 (what a sort on the float64 bit pattern does); every other value ties with itself."""
    return 0 if (v == 0.0 and math.copysign(1.0, v) < 0) else 1


def group_model(hits, time_window_ns, fix0=None, fix1=None, *, quantum=1.0, ge_new_event=False, prev_end=False,
                neg_zero_first=False, int_ts_key=False):
    """Events of group_hit_windows as [(t_min, t_max, [hit indices])] plus a dict of counts.

    Rules: global order by (abs_start, dt, timestamp, record_id); a hit opens a new event iff
    abs_start > running max of every earlier abs_end + window; members ordered by (board, channel, dt, abs_start,
    timestamp, record_id); t_min / t_max = int() (truncation) of the event's extreme window values.
    counts: eq / above / below = hits whose start is exactly at the threshold, within one `quantum` above, within one below;
    held_earlier = of those, the ones where the running max is NOT the previous hit's end.
    Switches (each a way the kernels could be wrong): ge_new_event `>` -> `>=` (k_event_flags); prev_end: previous end
    instead of the running max; neg_zero_first: -0.0 sorts before +0.0 (ord_f64 unguarded); int_ts_key: keys
    (int(abs_start), dt, timestamp - int(abs_start)) whatever the table holds (k_hit_prep without its switch)."""
    n = len(hits)
    counts = {"eq": 0, "above": 0, "below": 0, "held_earlier": 0}
    if n == 0:
        return [], counts
    a0, a1 = abs_windows(hits, fix0, fix1)
    ts = [int(v) for v in hits["timestamp"]]
    dt = [int(v) for v in hits["dt"]]
    rid = [int(v) for v in hits["record_id"]]
    board = [int(v) for v in hits["board"]]
    chan = [int(v) for v in hits["channel"]]
    if int_ts_key:
        key = lambda i: (int(a0[i]), dt[i], ts[i] - int(a0[i]), rid[i])  # noqa: E731
    elif neg_zero_first:
        key = lambda i: (a0[i], _zero_rank(a0[i]), dt[i], ts[i], rid[i])  # noqa: E731
    else:
        key = lambda i: (a0[i], dt[i], ts[i], rid[i])  # noqa: E731
    order = sorted(range(n), key=key)
    gap = time_window_ns * 1e3
    groups = [[order[0]]]
    run = a1[order[0]]
    prev = a1[order[0]]
    for i in order[1:]:
        thr = (prev if prev_end else run) + gap
        if a0[i] == thr:
            counts["eq"] += 1
        elif 0 < a0[i] - thr <= quantum:
            counts["above"] += 1
        elif 0 < thr - a0[i] <= quantum:
            counts["below"] += 1
        if abs(a0[i] - thr) <= quantum and run != prev:
            counts["held_earlier"] += 1
        new = a0[i] >= thr if ge_new_event else a0[i] > thr
        if new:
            groups.append([i])
            run = a1[i]
        else:
            groups[-1].append(i)
            run = a1[i] if a1[i] > run else run
        prev = a1[i]
    events = []
    for g in groups:
        if int_ts_key:
            inner = lambda i: (board[i], chan[i], dt[i], int(a0[i]), ts[i] - int(a0[i]), rid[i])  # noqa: E731
        elif neg_zero_first:
            inner = lambda i: (board[i], chan[i], dt[i], a0[i], _zero_rank(a0[i]), ts[i], rid[i])  # noqa: E731
        else:
            inner = lambda i: (board[i], chan[i], dt[i], a0[i], ts[i], rid[i])  # noqa: E731
        members = sorted(g, key=inner)
        events.append((int(min(a0[i] for i in g)), int(max(a1[i] for i in g)), members))
    return events, counts


def merge_model(hits, merge_gap_ns, max_total_width_ns, *, quantum=1.0, walk_running_max=False, gap_strict=False,
                cap_strict=False):
    """Clusters of hit_merge as lists of hit indices (chain order) plus counts.

    Rules: per (board, channel) ascending, hits stable by abs_start; a hit joins the current cluster iff merging is on
    (gap > 0), its dt equals the previous hit's, abs_start - cluster_end <= gap and max(cluster_end, abs_end) -
    cluster_start <= cap.  counts: gap_eq / gap_above / gap_below and cap_eq / cap_above / cap_below = comparisons met
    exactly at, one quantum above, one below their bound; shadowed = breaks taken although abs_start - (running max of
    every earlier end of the channel) <= gap, i.e. where k_merge_chain's head test does not fire and only its in-walk
    test can break.  Switches: walk_running_max: the walk measures the gap from that running max instead of the cluster
    end; gap_strict / cap_strict: `<=` -> `<`."""
    counts = {k: 0 for k in ("gap_eq", "gap_above", "gap_below", "cap_eq", "cap_above", "cap_below", "shadowed")}
    n = len(hits)
    if n == 0:
        return [], counts
    a0, a1 = abs_windows(hits)
    dt = [int(v) for v in hits["dt"]]
    board = [int(v) for v in hits["board"]]
    chan = [int(v) for v in hits["channel"]]
    gap, cap = merge_gap_ns * 1e3, max_total_width_ns * 1e3
    order = sorted(range(n), key=lambda i: (board[i], chan[i], a0[i]))  # python's sort is stable: input order on ties
    clusters = []
    cur = None
    for k, i in enumerate(order):
        p = order[k - 1] if k else None
        if p is None or (board[p], chan[p]) != (board[i], chan[i]):
            cur = [i]
            clusters.append(cur)
            c_start, c_end, run = a0[i], a1[i], a1[i]
            continue
        ok = merge_gap_ns > 0 and dt[i] == dt[p]
        if ok:
            d = a0[i] - (run if walk_running_max else c_end)
            if d == gap:
                counts["gap_eq"] += 1
            elif 0 < d - gap <= quantum:
                counts["gap_above"] += 1
            elif 0 < gap - d <= quantum:
                counts["gap_below"] += 1
            ok = d < gap if gap_strict else d <= gap
        if ok:
            nxt = a1[i] if a1[i] > c_end else c_end
            w = nxt - c_start
            if w == cap:
                counts["cap_eq"] += 1
            elif 0 < w - cap <= quantum:
                counts["cap_above"] += 1
            elif 0 < cap - w <= quantum:
                counts["cap_below"] += 1
            ok = w < cap if cap_strict else w <= cap
        if ok:
            cur.append(i)
            c_end = nxt
        else:
            if merge_gap_ns > 0 and dt[i] == dt[p] and a0[i] - run <= gap:
                counts["shadowed"] += 1
            cur = [i]
            clusters.append(cur)
            c_start, c_end = a0[i], a1[i]
        run = a1[i] if a1[i] > run else run
    return clusters, counts


def pairwise_sum(x, *, leaf=128, lanes=8, loop_below=8, align=8):
    """numpy's pairwise float64 sum of the python floats x (numpy/_core/src/umath/loops_utils.h.src): fewer than
    `loop_below` terms: a running sum from 0.0; up to `leaf` terms: `lanes` accumulators over the whole multiples of
    `lanes`, combined as a balanced tree, then the tail one by one; otherwise split at n // 2 rounded down to a multiple
    of `align`.  numpy: leaf=128, lanes=8, loop_below=8, align=8."""
    n = len(x)
    if n < loop_below or lanes == 1:
        r = 0.0
        for v in x:
            r += v
        return r
    if n <= leaf:
        acc = [float(v) for v in x[:lanes]]
        full = n - n % lanes
        for i in range(lanes, full, lanes):
            for j in range(lanes):
                acc[j] += x[i + j]
        while len(acc) > 1:
            acc = [acc[k] + acc[k + 1] for k in range(0, len(acc), 2)]
        r = acc[0]
        for v in x[full:]:
            r += v
        return r
    h = n // 2
    h -= h % align
    kw = dict(leaf=leaf, lanes=lanes, loop_below=loop_below, align=align)
    return pairwise_sum(x[:h], **kw) + pairwise_sum(x[h:], **kw)


NUMPY_TREE = dict(leaf=128, lanes=8, loop_below=8, align=8)
WRONG_TREES = {
    "left_to_right": dict(leaf=1 << 30, lanes=1, loop_below=8, align=8),
    "four_accumulators": dict(leaf=128, lanes=4, loop_below=8, align=8),
    "leaf_64": dict(leaf=64, lanes=8, loop_below=8, align=8),
    "leaf_256": dict(leaf=256, lanes=8, loop_below=8, align=8),
    "split_unaligned": dict(leaf=128, lanes=8, loop_below=8, align=1),
}


def merged_model(hits, clusters, tree=None):
    """Per cluster of several hits (anchor hit index, height f32, integral f32, sample_start, sample_end, width f32) by the
    rules of _emit_cluster (hit_merge.py:256-322): the anchor is the member of maximal height, ties to the smallest
    timestamp, then to the first such member; the integral is numpy's pairwise float64 sum rounded to float32; the window
    is (min edge_start, max edge_end) if all members share a record, else (-1, -1); width = max(end - start, 0), or -1
    without a window.  A cluster of one hit is the hit itself."""
    tree = NUMPY_TREE if tree is None else tree
    out = []
    for members in clusters:
        if len(members) == 1:
            h = hits[members[0]]
            out.append((int(members[0]), np.float32(h["height"]), np.float32(h["integral"]), int(h["edge_start"]),
                        int(h["edge_end"]), np.float32(h["width"])))
            continue
        best = None
        for i in members:
            hv, tv = float(hits["height"][i]), int(hits["timestamp"][i])
            if best is None or hv > best[0] or (hv == best[0] and tv < best[1]):
                best = (hv, tv, int(i))
        if len({int(hits["record_id"][i]) for i in members}) == 1:
            s0 = min(int(hits["edge_start"][i]) for i in members)
            s1 = max(int(hits["edge_end"][i]) for i in members)
        else:
            s0 = s1 = -1
        width = -1.0 if (s0 < 0 or s1 < 0) else float(max(s1 - s0, 0))
        total = pairwise_sum([float(hits["integral"][i]) for i in members], **tree)
        out.append((best[2], np.float32(best[0]), np.float32(total), s0, s1, np.float32(width)))
    return out


def sort_model(timestamp, pid, board, channel):
    """Stable order by (timestamp, pid, board, channel) with python ints (records_builder.py:115-120)."""
    keys = list(zip((int(v) for v in timestamp), (int(v) for v in pid), (int(v) for v in board), (int(v) for v in channel)))
    return sorted(range(len(keys)), key=keys.__getitem__)


MUTANTS = {
    # name: (model, switch, the kernel line it stands for)
    "new_event_ge": ("group", "ge_new_event", "k_event_flags: abs0[perm[j]] > run_max[j - 1] + gap_ps"),
    "previous_end": ("group", "prev_end", "the MaxF64 inclusive scan feeding k_event_flags"),
    "neg_zero_first": ("group", "neg_zero_first", "k_float_keys: ord_f64(abs0[i]) on a -0.0 start"),
    "int_keys_always": ("group", "int_ts_key", "k_hit_prep: the inexact flag and the 4.0e18 switch"),
    "walk_running_max": ("merge", "walk_running_max", "k_merge_chain: gap = a - c_end inside the walk"),
    "gap_lt": ("merge", "gap_strict", "k_merge_chain: gap <= gap_ps"),
    "cap_lt": ("merge", "cap_strict", "k_merge_chain: total <= max_width_ps"),
}


# ---- helpers of the builders ------------------------------------------------------------------------------------------------
def quantum_at(base) -> float:
    """Spacing of the representable window values around `base`: 1 ps while integers are exact, np.spacing above."""
    return 1.0 if abs(base) < 2**53 else float(np.spacing(np.float64(abs(base))))


def _table(rows) -> np.ndarray:
    """rows: dicts with timestamp, position, edge_start, edge_end, dt, board, channel, record_id[, height, integral]."""
    hits = np.zeros(len(rows), dtype=THRESHOLD_HIT_DTYPE)
    for name in ("timestamp", "position", "edge_start", "edge_end", "dt", "board", "channel", "record_id"):
        hits[name] = [r[name] for r in rows]
    hits["width"] = hits["edge_end"] - hits["edge_start"]
    hits["height"] = [r.get("height", 20.0 + (k % 7)) for k, r in enumerate(rows)]
    hits["integral"] = [r.get("integral", 100.0 + (k % 13)) for k, r in enumerate(rows)]
    return hits


def _row(start_ps: int, n_samples: int, dt: int, board: int, channel: int, rid: int, lead: int = 0, s: int = 10, **kw):
    """A hit whose window starts at the integer `start_ps` and spans n_samples of dt ns; `lead` samples lie between the
    window start and the hit position (timestamp = start + lead * dt * 1000: exact below 2^53, use lead = 0 above)."""
    return dict(timestamp=int(start_ps) + lead * dt * 1000, position=s + lead, edge_start=s, edge_end=s + n_samples, dt=dt,
                board=board, channel=channel, record_id=rid, **kw)


def _actual(row):
    """(abs_start, abs_end) of a row as the kernels and the reference compute them."""
    t, p, dps = float(row["timestamp"]), float(row["position"]), float(row["dt"]) * 1e3
    return t + (float(row["edge_start"]) - p) * dps, t + (float(row["edge_end"]) - p) * dps


# ---- A ---------------------------------------------------------------------------------------------------------------------
KEY_ROUTE_BASES = {
    "negative": -10**15, "zero": 0, "below_2p53": 2**53 - 10**6, "2p58": 2**58, "below_switch": int(3.9e18),
    "straddle": None, "2p62": 2**62, "below_2p63": 2**63 - 2**40,
}
INTEGER_ROUTE_BASES = ("negative", "zero", "below_2p53", "2p58", "below_switch")


def key_route(base_name: str, n: int = 30000, seed: int = 31, n_records: int = 100, n_channels: int = 3) -> np.ndarray:
    """The `crafted` table of test_hip_hits.py with its timestamps moved to start at a base on either side of
    k_hit_prep's switch (wfa_hits.hip:185 `fabs(a0) < 4.0e18`): below it the integer keys of :186-190, above it (and for
    the straddling table: for ALL rows) k_float_keys.  Above 2^53 neighbouring starts round to the same float64, so the
    later keys dt / timestamp / record_id of lexsort (:883) decide."""
    from tests.test_hip_hits import crafted

    hits = crafted(seed, n, n_records, n_channels)
    rel = hits["timestamp"] - 2**58
    if base_name == "straddle":
        base = int(KEY_SWITCH) - int(np.median(rel))
    else:
        base = KEY_ROUTE_BASES[base_name]
    hits["timestamp"] = rel + base
    a1 = np.array(abs_windows(hits)[1])
    assert a1.max() < COMPARABLE_END
    return hits


def with_far_row(hits: np.ndarray) -> np.ndarray:
    """hits + one row in a channel and at a time of its own whose start is >= 4.0e18: it switches every row to the
    float keys (hit_prep, wfa_hits.hip:221) and forms an event / a cluster of its own."""
    out = np.concatenate([hits, _table([_row(2**62, 3, 4, 7, 30000, 123456789)])])
    return out


# ---- B ---------------------------------------------------------------------------------------------------------------------
WINDOWS_NS = (0.0, 0.0005, 100.0, 3000.0)


def window_boundaries(window_ns: float, base: int, cycles: int = 120, seed: int = 5):
    """(hits, fix0, fix1, quantum).  Cycles of three hits in sorted order: L (long, far after everything before: a new
    event, holds the running max), S (short, inside L: the PREVIOUS end is smaller than the running max) and X, whose start
    is exactly running_max_end + window, or that plus / minus one quantum (k_event_flags, wfa_hits.hip:294: `>`; the
    running max comes from the MaxF64 scan of :893).  Where the threshold is not an integer (0.0005 ns below 2^53) X
    carries its window in abs_start_fix / abs_end_fix, which also takes the float keys."""
    rng = np.random.default_rng(seed)
    q = quantum_at(base)
    gap = window_ns * 1e3
    rows, fixes = [], []
    t = int(base)
    rid = 0
    for c in range(cycles * 3):
        delta = (0.0, q, -q)[c % 3]
        dt = int(rng.choice([2, 4]))
        lead = int(rng.integers(0, 3)) if base < 2**52 else 0
        long_row = _row(t, int(rng.integers(200, 300)), dt, int(rng.integers(0, 3)), int(rng.integers(-2, 6)), rid, lead)
        l0, l1 = _actual(long_row)
        short = _row(int(l0) + 8 * int(q) * int(rng.integers(1, 5)), int(rng.integers(1, 20)), dt, int(rng.integers(0, 3)),
                     int(rng.integers(-2, 6)), rid + 1)
        s0, s1 = _actual(short)
        assert l0 <= s0 and s1 < l1
        want = (l1 + gap) + delta
        x = _row(int(want), int(rng.integers(1, 20)), int(rng.choice([2, 4])), int(rng.integers(0, 3)),
                 int(rng.integers(-2, 6)), rid + 2)
        x0, x1 = _actual(x)
        fx = (math.nan, math.nan)
        if x0 != want:  # a fractional threshold: the window goes in through the fix arrays
            assert base < 2**52
            fx = (want, want + 4000.5)
            x0, x1 = fx
        assert x0 == want and x0 >= s0
        rows += [long_row, short, x]
        fixes += [(math.nan, math.nan), (math.nan, math.nan), fx]
        t = int(max(l1, x1)) + int(gap) + 50_000_000 + 1024 * int(q) * int(rng.integers(1, 9))
        rid += 3
    perm = rng.permutation(len(rows))
    hits = _table([rows[k] for k in perm])
    fix0 = np.array([fixes[k][0] for k in perm])
    fix1 = np.array([fixes[k][1] for k in perm])
    if np.all(np.isnan(fix0)):
        fix0 = fix1 = None
    return hits, fix0, fix1, q


# ---- C ---------------------------------------------------------------------------------------------------------------------
MERGE_GAP_NS, MERGE_CAP_NS = 20.0, 900.0


def merge_boundaries(base: int = 10**12, reps: int = 110, seed: int = 9):
    """(hits, quantum) for merge_gap_ns = 20, max_total_width_ns = 900 (k_merge_chain, wfa_hits.hip:421-451).
    Channel by channel:
      gap   pairs with start - cluster_end == gap, one quantum more, one less                     (:441 gap <= gap_ps)
      cap   pairs within the gap whose joint width == cap, one quantum more, one less            (:441 total <= max_width_ps)
      dt    a dt change inside an otherwise mergeable chain                                        (:427 / :435 sdt)
      shadowed  a long hit (1200 ns > cap) that contains 2 .. 50 short hits, some more than the gap apart: the cluster of
            the long hit closes on the cap, and every later break lies below the channel's running max end, where the head
            test of :427-428 cannot fire (the issue's A=[0,1000] B=[10,20] C=[500,510]); also two overlapping long hits."""
    rng = np.random.default_rng(seed)
    q = quantum_at(base)
    gap, cap = int(MERGE_GAP_NS * 1e3), int(MERGE_CAP_NS * 1e3)
    step = int(max(q, 1))
    rows = []
    rid = 0

    def far(t):
        return t + 40 * cap + 4096 * step * int(rng.integers(1, 5))

    # gap boundaries, board 0 channel -32768
    t = int(base)
    for r in range(reps * 3):
        d = (0, step, -step)[r % 3]
        a = _row(t, int(rng.integers(2, 30)), 4, 0, -32768, rid)
        a1 = _actual(a)[1]
        b = _row(int(a1) + gap + d, int(rng.integers(2, 30)), 4, 0, -32768, rid + 1)
        assert _actual(b)[0] - a1 == gap + d
        rows += [a, b]
        t, rid = far(int(_actual(b)[1])), rid + 2
    # cap boundaries, board 0 channel 32767
    t = int(base)
    for r in range(reps * 3):
        d = (0, step, -step)[r % 3]
        a = _row(t, 201, 4, 0, 32767, rid)
        a0, a1 = _actual(a)
        n_b = 20
        b_start = int(a0) + cap + d - n_b * 4000
        b = _row(b_start, n_b, 4, 0, 32767, rid + 1)
        b0, b1 = _actual(b)
        assert b1 - a0 == cap + d and 0 <= b0 - a1 <= gap
        rows += [a, b]
        t, rid = far(int(b1)), rid + 2
    # dt change inside a mergeable chain, board 32767 channel 0
    t = int(base)
    for r in range(reps):
        for k, dt in enumerate((4, 4, 2, 2, 4)):
            rows.append(_row(t, 2, dt, 32767, 0, rid))
            t, rid = int(_actual(rows[-1])[1]) + 4000, rid + 1
        t = far(t)
    # shadowed chains, board -32768 channel -1
    t = int(base)
    for depth in list(range(2, 51)) + [7, 19, 33]:
        rows.append(_row(t, 300, 4, -32768, -1, rid))  # 1200 ns
        u = t + 4000 * int(rng.integers(1, 4))
        for k in range(depth):
            rows.append(_row(u, 1, 4, -32768, -1, rid + 1 + k % 2))
            u += 4000 + int(rng.choice([8000, 24000]))  # gap of 8 ns (joins) or 24 ns (breaks)
        if depth % 5 == 0:  # a second long hit overlapping the first, with shorts inside both
            rows.append(_row(t + 600_000, 300, 4, -32768, -1, rid))
            rows.append(_row(t + 700_000, 1, 4, -32768, -1, rid))
            rows.append(_row(t + 800_000, 1, 4, -32768, -1, rid))
        t, rid = far(t + 2_000_000), rid + 3
    perm = rng.permutation(len(rows))
    return _table([rows[k] for k in perm]), q


def long_segment(n: int = 20500, seed: int = 13) -> np.ndarray:
    """One channel holding a single segment of n hits no gap ever cuts (every gap <= 20 ns), so that one lane of
    k_merge_chain walks all of it and only the 900 ns cap closes clusters (wfa_hits.hip:434-450); a second, short channel
    on each side of it in (board, channel) order."""
    rng = np.random.default_rng(seed)
    rows = [_row(10**9 + 50_000 * k, 2, 4, 0, 0, k) for k in range(5)]
    t = 10**9
    for k in range(n):
        rows.append(_row(t, 1, 4, 1, 3, k // 50, lead=int(rng.integers(0, 2))))
        t += 4000 + 4000 * int(rng.integers(1, 6))
    rows += [_row(10**9 + 50_000 * k, 2, 4, 2, -2, k) for k in range(5)]
    perm = rng.permutation(len(rows))
    return _table([rows[k] for k in perm])


def many_segments(n: int = 52000, seed: int = 17) -> np.ndarray:
    """n hits on 4 channels, every one more than any tested merge gap after the channel's previous end: n segments of one
    hit each, one walking lane per hit (k_merge_chain's head test, wfa_hits.hip:427-429)."""
    rng = np.random.default_rng(seed)
    ch = rng.integers(0, 4, n)
    hits = np.zeros(n, dtype=THRESHOLD_HIT_DTYPE)
    hits["channel"], hits["board"], hits["dt"] = ch - 2, 1, 4
    hits["edge_start"], hits["edge_end"], hits["position"] = 10, 13, 11
    hits["width"] = 3
    hits["record_id"] = np.arange(n) // 8
    hits["timestamp"] = 7 * 10**11 + np.arange(n, dtype=np.int64) * 200_000 + rng.integers(0, 50, n) * 1000
    hits["height"] = 25.0
    hits["integral"] = 80.0
    return hits[rng.permutation(n)]


# ---- D ---------------------------------------------------------------------------------------------------------------------
KEY_NAMES = ("abs_start", "dt", "timestamp", "record_id", "board", "channel")
KEY_SIZES = (1, 2, 255, 256, 257, 65537)


def key_extremes(n: int, constant=(), seed: int = 23) -> np.ndarray:
    """n hits whose sort keys take their types' extremes, with heavy ties on every key so that the later ones decide:
    board / channel in I16, record_id in I64 + random, dt in DT_EXTREMES, few distinct starts.  `constant`: names out of
    KEY_NAMES held at one value (lexsort skips such a key, wfa_hits.hip:138; all six: every pass is skipped and the order
    must be the identity).  Sizes 255 / 256 / 257 / 65 537 are block edges of k_key_ranges and of
    the one-row-per-lane kernels (kTB = 256: a last block of 255, 0 or 1 rows; 65 537 rows: 257 blocks, one row in the last)."""
    rng = np.random.default_rng(seed + n)
    pick = lambda vals, name, fixed: np.full(n, fixed) if name in constant else rng.choice(np.array(vals), n)  # noqa: E731
    dt = pick(DT_EXTREMES, "dt", 4).astype(np.int64)
    big = dt == 2**31 - 1
    lead = np.where(big, 0, rng.integers(0, 3, n))  # samples between window start and position
    start = 10**13 + rng.integers(0, 12, n) * 4000 if "abs_start" not in constant else np.full(n, 10**13)
    ts = start + lead * dt * 1000
    if "timestamp" in constant:  # the starts then vary through (lead, dt) alone
        ts = np.full(n, 10**13 + 8000)
        if "abs_start" in constant:
            lead = np.zeros(n, dtype=np.int64)
    rid = np.where(rng.random(n) < 0.7, rng.choice(np.array(I64, dtype=np.int64), n), rng.integers(-5, 5, n))
    if "record_id" in constant:
        rid = np.full(n, 2**63 - 1)
    hits = np.zeros(n, dtype=THRESHOLD_HIT_DTYPE)
    hits["timestamp"], hits["dt"], hits["record_id"] = ts, dt, rid
    hits["edge_start"] = 5
    hits["position"] = 5 + lead
    hits["edge_end"] = 5 + np.where(big, 1, rng.integers(1, 4, n))
    hits["width"] = hits["edge_end"] - hits["edge_start"]
    hits["board"] = pick(I16, "board", -32768)
    hits["channel"] = pick(I16, "channel", 32767)
    hits["height"] = rng.choice([12.0, 30.5, 77.25], n)
    hits["integral"] = rng.integers(1, 900, n)
    return hits


SORT_DTYPE = np.dtype([("timestamp", "i8"), ("pid", "i4"), ("board", "i2"), ("channel", "i2")])
SORT_KEYS = ("timestamp", "pid", "board", "channel")


def record_sort_columns(n: int, constant=(), seed: int = 29) -> np.ndarray:
    """Rows for wfa_records_sort (wfa_hits.hip:1150): timestamps in I64 + a few random ones (a span of 2^64 - 1: lexsort's
    `bits == 64`), pid in I32, board / channel in I16; few distinct values per key, so most rows tie on all four and the
    stable input order is what is tested.  `constant`: keys held at one value."""
    rng = np.random.default_rng(seed + n)
    rec = np.zeros(n, dtype=SORT_DTYPE)
    extra = rng.integers(-2**62, 2**62, 3)
    rec["timestamp"] = rng.choice(np.concatenate([np.array(I64, dtype=np.int64), extra]), n)
    rec["pid"] = rng.choice(np.array(I32, dtype=np.int32), n)
    rec["board"] = rng.choice(np.array(I16, dtype=np.int16), n)
    rec["channel"] = rng.choice(np.array(I16, dtype=np.int16), n)
    for name, v in zip(SORT_KEYS, (-2**63, 2**31 - 1, -32768, 32767)):
        if name in constant:
            rec[name] = v
    return rec


# ---- E ---------------------------------------------------------------------------------------------------------------------
def fixed_windows(fractional: bool = True, seed: int = 37):
    """(hits, fix0, fix1): rows whose window comes from abs_start_fix / abs_end_fix (k_hit_prep, wfa_hits.hip:181-182).
    Groups, far apart in time: `zeros`: eight rows starting at +0.0 / -0.0 in turn whose (dt, timestamp, record_id) order
    is the reverse of their input order (np.lexsort ties -0.0 with +0.0; k_float_keys' ord_f64 must not order them);
    `negative`: starts at -x.5 (t_min = int(-2.5) = -2: truncation toward zero, k_event_minmax :325); `half`: starts and
    ends at x.5 ps between integer rows one ps either side; `collapse`: pairs of one channel whose starts differ by half a ps and
    truncate to the same integer, the later start carrying the smaller timestamp (integer keys would swap them); `far`: fixes
    10^9 ps away from the row's own timestamp.
    fractional=False keeps every fix an integer (then only the zeros are special, and the integer keys are used)."""
    rng = np.random.default_rng(seed)
    h = 0.5 if fractional else 0.0
    rows, fixes = [], []

    def add(row, f0=math.nan, f1=math.nan):
        rows.append(row)
        fixes.append((f0, f1))

    for k in range(8):  # input order k = 0..7, key order reversed: later rows have the smaller (dt, ts, rid)
        add(_row(900 - 100 * k, 2, 4 if k < 4 else 2, 0, 1, 50 - k), 0.0 if k % 2 == 0 else -0.0, 3000.0 + h)
    for k in range(6):
        add(_row(-10**9 + 1000 * k, 2, 2, 1, k % 2, k), -10**9 - 2.0 - h - k, -10**9 + 4000.0 + h)
    add(_row(-5000, 1, 1, 1, 0, 7), -2.0 - h, -1.0 - h)  # an event of its own at window 0: t_min = int(-2.5)
    for k in range(40):
        t = 10**7 + 100_000 * (k // 4)
        if k % 4 == 0:
            add(_row(t, 3, 4, 2, k % 5 - 2, k))
        else:
            add(_row(t + 50, 3, 4, 2, k % 5 - 2, k), t + 12_000.0 + (k % 4 - 2) + h, t + 13_000.0 + h)
    for k in range(6):  # `collapse`: starts u and u + 0.5 (-u - 0.5 and -u) of one channel, the later start has the smaller timestamp
        u = 3 * 10**8 + 10_000 * k
        low, high = (float(u), u + h) if k % 2 == 0 else (-u - h, float(-u))
        add(_row(int(low) + 5000, 2, 4, 1, 2, 200 + k), low, low + 8000.0)
        add(_row(int(low) + 100, 2, 4, 1, 2, 300 + k), high, high + 8000.0)
    for k in range(10):
        add(_row(5 * 10**9 + k, 2, 4, 0, 1, 100 + k), 2.0 * 10**8 + 1000 * (k % 3) + h, 2.0 * 10**8 + 9000.0)
    perm = np.concatenate([np.arange(8), 8 + rng.permutation(len(rows) - 8)])  # the zeros keep their input order
    hits = _table([rows[k] for k in perm])
    return hits, np.array([fixes[k][0] for k in perm]), np.array([fixes[k][1] for k in perm])


# ---- F ---------------------------------------------------------------------------------------------------------------------
TIE_SIZES = (2, 7, 8, 9, 16, 127, 128, 129, 140, 255, 256, 257, 300, 1000, 5000)
BIG, MID, TINY = 2.0**30, 64.0, 2.0**-24


def integral_ties(sizes=TIE_SIZES):
    """[(size, label, float32 integrals)]: one 2^30, one 64 eight places after it (wrapping), some 2^-24, the rest 0.
    2^30 + 64 is exactly half-way between two float32 values and a 2^-24 added to 2^30 in float64 is lost, so the rounded
    sum (2^30 or 2^30 + 128) tells whether a small term met another small term or the 64 before it met 2^30: one bit of
    the addition tree of np_pairwise_sum (wfa_numpy.hpp) as used by k_merge_emit (wfa_hits.hip:496)."""
    out = []
    seen = set()
    for n in sizes:
        half = n // 2
        n2 = half - half % 8
        for big in sorted({0, min(3, n - 1), n // 2, n - 1}):
            mid = (big + 8) % n
            if mid == big:
                mid = (big + 1) % n
            idx = np.arange(n)
            other_half = (idx >= n2) if big < n2 else (idx < n2)
            masks = {
                "class": idx % 8 == big % 8,
                "class+4": idx % 8 == (big + 4) % 8,
                "other_half": other_half,
                "n2_to_half": (idx >= n2) & (idx < half),
                "second_quarter": (idx >= n // 4) & (idx < n // 2),
                "third_quarter": (idx >= n // 2) & (idx < 3 * n // 4),
                "none": np.zeros(n, dtype=bool),
            }
            for label, m in masks.items():
                x = np.zeros(n, dtype=np.float32)
                x[m] = TINY
                x[mid] = MID
                x[big] = BIG
                key = (n, x.tobytes())
                if key in seen:
                    continue
                seen.add(key)
                out.append((n, f"big{big}_{label}", x))
    return out


def clusters_table(integral_sets, seed: int = 41):
    """(hits, clusters): one cluster of consecutive hits per integral set (all of one record and channel), heights and
    timestamps random, for wfa_hit_merge_emit with a hand-made membership table."""
    rng = np.random.default_rng(seed)
    n = sum(len(x) for x in integral_sets)
    hits = np.zeros(n, dtype=THRESHOLD_HIT_DTYPE)
    hits["integral"] = np.concatenate(integral_sets)
    hits["height"] = rng.choice([12.0, 30.5, 77.25, 140.0], n)
    hits["timestamp"] = 10**12 + rng.integers(0, 1000, n) * 1000
    hits["edge_start"] = rng.integers(0, 300, n)
    hits["edge_end"] = hits["edge_start"] + rng.integers(1, 20, n)
    hits["position"] = hits["edge_start"]
    hits["width"] = hits["edge_end"] - hits["edge_start"]
    hits["dt"], hits["channel"] = 4, 3
    clusters, at = [], 0
    for k, x in enumerate(integral_sets):
        clusters.append(list(range(at, at + len(x))))
        hits["record_id"][at:at + len(x)] = k
        at += len(x)
    return hits, clusters


# ---- G ---------------------------------------------------------------------------------------------------------------------
def anchor_ties():
    """(hits, clusters) for k_merge_emit's anchor and window rules (wfa_hits.hip:470-495): the maximal height held by
    several members with equal and with different timestamps, the first such member late in the cluster; a cluster over
    two records (-1 / -1 / -1.0); windows whose max edge_end <= min edge_start (width clamps to 0.0); a cluster of one."""
    rows, clusters = [], []

    def cluster(members):
        at = len(rows)
        rows.extend(members)
        clusters.append(list(range(at, at + len(members))))

    def hit(ts, height, rid=1, s=10, e=14, integral=3.0):
        return dict(timestamp=ts, position=s, edge_start=s, edge_end=e, dt=4, board=0, channel=1, record_id=rid,
                    height=height, integral=integral)

    # equal heights, different timestamps: the smallest timestamp wins although it comes last
    cluster([hit(5000, 9.0), hit(4000, 77.25), hit(3000, 12.0), hit(3500, 77.25), hit(3200, 77.25)])
    # equal heights and equal timestamps: the first of them, which stands late in the cluster
    cluster([hit(100, 1.0), hit(90, 2.0), hit(80, 3.0), hit(70, 140.0, s=20, e=30), hit(70, 140.0, s=40, e=50),
             hit(71, 140.0)])
    # a tie among hundreds of members (past one pairwise leaf), first maximal member at index 200
    many = [hit(10**6 + k, 30.5 if k < 200 else 99.0, s=k, e=k + 2) for k in range(300)]
    many[250]["timestamp"] = 10**6 - 1
    cluster(many)
    # two records: no sample window
    cluster([hit(10, 5.0, rid=1), hit(20, 6.0, rid=2), hit(30, 6.0, rid=1)])
    # max(edge_end) <= min(edge_start): width 0.0, equal and reversed
    cluster([hit(10, 5.0, s=50, e=50), hit(20, 4.0, s=50, e=50)])
    cluster([hit(10, 5.0, s=50, e=40), hit(20, 7.0, s=60, e=45)])
    # record ids at the int64 extremes, negative timestamps
    cluster([hit(-2**62, 8.0, rid=-2**63), hit(-2**62 - 1, 8.0, rid=-2**63)])
    cluster([hit(0, 8.0, rid=-2**63), hit(-1, 8.0, rid=2**63 - 1)])
    cluster([hit(77, 1.5)])
    return _table(rows), clusters


# ---- the case lists both test files walk ------------------------------------------------------------------------------------
B_BASES = {"0": 0, "2p58": 2**58, "2p62": 2**62}
ONE_EVENT_WINDOW_NS = 1e12  # larger than the span of every B table
CONSTANT_SETS = ((),) + tuple((k,) for k in KEY_NAMES) + (("board", "channel", "dt"), KEY_NAMES)


def group_case_names():
    names = [f"A-{b}" for b in KEY_ROUTE_BASES]
    names += [f"B-{w}-{b}" for w in WINDOWS_NS for b in B_BASES]
    names += ["C-boundaries", "C-many_segments"]
    names += [f"D-{n}-{'+'.join(c) or 'vary'}" for n in (255, 256, 257) for c in CONSTANT_SETS]
    names += [f"D-{n}-{'+'.join(c) or 'vary'}" for n in (1, 2, 65537) for c in ((), KEY_NAMES)]
    names += ["E-fractional", "E-integer"]
    return names


_CACHE: dict = {}


def group_case(name: str) -> dict:
    """{hits, fix0, fix1, windows (ns), quantum, design_window} of a name out of group_case_names()."""
    if name in _CACHE:
        return _CACHE[name]
    kind, _, rest = name.partition("-")
    case = dict(fix0=None, fix1=None, quantum=1.0, design_window=None)
    if kind == "A":
        case.update(hits=key_route(rest), windows=(0.0, 100.0, 3000.0), quantum=quantum_at(KEY_ROUTE_BASES[rest] or KEY_SWITCH))
    elif kind == "B":
        w, _, b = rest.partition("-")
        hits, f0, f1, q = window_boundaries(float(w), B_BASES[b])
        case.update(hits=hits, fix0=f0, fix1=f1, quantum=q, design_window=float(w),
                    windows=tuple(dict.fromkeys((float(w),) + WINDOWS_NS + (ONE_EVENT_WINDOW_NS,))))
    elif kind == "C":
        hits = merge_boundaries()[0] if rest == "boundaries" else many_segments()
        case.update(hits=hits, windows=(0.0005, MERGE_GAP_NS))
    elif kind == "D":
        n, _, c = rest.partition("-")
        case.update(hits=key_extremes(int(n), () if c == "vary" else tuple(c.split("+"))), windows=(0.0, 100.0))
    else:
        hits, f0, f1 = fixed_windows(rest == "fractional")
        case.update(hits=hits, fix0=f0, fix1=f1, windows=(0.0, 0.0005, 100.0))
    _CACHE[name] = case
    return case


MERGE_CONFIGS = ((MERGE_GAP_NS, MERGE_CAP_NS), (0.0, MERGE_CAP_NS), (0.001, MERGE_CAP_NS), (400.0, 10000.0))


def merge_case_names():
    return ["C-boundaries", "C-boundaries-above_2p53", "C-long_segment", "C-many_segments", "A-2p58", "A-straddle", "A-below_2p63",
            "D-257-vary", "D-257-board+channel+dt", "D-65537-vary"]


def merge_case(name: str) -> dict:
    """{hits, configs ((merge_gap_ns, max_total_width_ns), ...), quantum} of a name out of merge_case_names()."""
    key = "merge:" + name
    if key in _CACHE:
        return _CACHE[key]
    case = dict(configs=MERGE_CONFIGS, quantum=1.0)
    if name == "C-boundaries":
        case["hits"], case["quantum"] = merge_boundaries()
    elif name == "C-boundaries-above_2p53":
        case["hits"], case["quantum"] = merge_boundaries(base=2**53 + 2**40)  # quantum 2 ps: 20 ns and 900 ns stay exact
    elif name == "C-long_segment":
        case["hits"] = long_segment()
    elif name == "C-many_segments":
        case["hits"] = many_segments()
    else:
        case["hits"] = group_case(name)["hits"]
        case["configs"] = MERGE_CONFIGS[:2] + MERGE_CONFIGS[3:]
    _CACHE[key] = case
    return case


def sort_case_names():
    names = [f"{n}-{'+'.join(c) or 'vary'}" for n in (255, 256, 257)
             for c in ((),) + tuple((k,) for k in SORT_KEYS) + (("pid", "board", "channel"), SORT_KEYS)]
    return names + [f"{n}-{'+'.join(c) or 'vary'}" for n in (1, 2, 65537) for c in ((), SORT_KEYS)]


def sort_case(name: str) -> np.ndarray:
    n, _, c = name.partition("-")
    return record_sort_columns(int(n), () if c == "vary" else tuple(c.split("+")))
