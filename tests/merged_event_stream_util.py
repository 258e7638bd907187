"""The merged-event stream's rule restated in numpy, and a device double that answers its three session calls with it.

`NumpyMergedEventStream` is the rule of DESIGN.md section 10 written against the rule, not against the library: the merge
step is `NumpyMergeStream` (the oracle's literal chain under a horizon); the group step appends the merged rows of the
clusters just closed behind its carry, with the windows the static route gives them (anchor formula, or the extent of the
member hits where the row has no sample window), groups carry ++ new rows and closes the events that end more than the
window before the grouping horizon G.  `static_merged_events` is the static grouping of a whole hit_merged table.
"""

from __future__ import annotations

import math

import numpy as np

from tests.event_stream_util import make_hits, row_horizons
from tests.merge_stream_util import CPU_CHUNK_SIZES, FIXTURES, NumpyMergeStream, chunk_size_of, fixture
from tests.stream_hits_util import OracleSession
from waveformanalysis_amd.event_grouping import EVENT_COLUMNS
from waveformanalysis_amd.dtypes import EVENT_MERGED_HIT_DTYPE, HIT_MERGED_DTYPE, THRESHOLD_HIT_DTYPE

EXACT_LIMIT_PS = 2**53
PER_HIT = (("dt", "dt"), ("boards", "board"), ("channels", "channel"), ("heights", "height"), ("integrals", "integral"),
           ("timestamps", "timestamp"), ("record_ids", "record_id"), ("sample_starts", "sample_start"),
           ("sample_ends", "sample_end"))


def hit_windows(hits: np.ndarray):
    t = hits["timestamp"].astype(np.float64)
    p = hits["position"].astype(np.float64)
    dps = hits["dt"].astype(np.float64) * 1e3
    return t + (hits["edge_start"].astype(np.float64) - p) * dps, t + (hits["edge_end"].astype(np.float64) - p) * dps


def member_windows(merged: np.ndarray, members: list, hits: np.ndarray):
    """(fix0, fix1) per merged row: NaN where the row has a sample window, else min abs_start / max abs_end of its member
    hits (`members[i]` = indices into `hits`)."""
    a0, a1 = hit_windows(hits)
    fix0, fix1 = np.full(len(merged), np.nan), np.full(len(merged), np.nan)
    for i in np.flatnonzero((merged["sample_start"] < 0) | (merged["sample_end"] < 0)):
        fix0[i], fix1[i] = a0[members[i]].min(), a1[members[i]].max()
    return fix0, fix1


def merged_windows(merged: np.ndarray, fix0: np.ndarray, fix1: np.ndarray):
    """abs_start / abs_end of merged rows: the anchor formula, replaced by the fix windows where they are not NaN."""
    t = merged["timestamp"].astype(np.float64)
    p = merged["position"].astype(np.float64)
    dps = merged["dt"].astype(np.float64) * 1e3
    a0 = t + (merged["sample_start"].astype(np.float64) - p) * dps
    a1 = t + (merged["sample_end"].astype(np.float64) - p) * dps
    return np.where(np.isnan(fix0), a0, fix0), np.where(np.isnan(fix1), a1, fix1)


def static_merged_events(merged: np.ndarray, fix0: np.ndarray, fix1: np.ndarray, window_ns: float) -> dict:
    """order (row indices, event-major), event_start, t_min, t_max (truncated) and hi (float max abs_end) per event."""
    n = len(merged)
    if n == 0:
        z = np.zeros(0, dtype=np.int64)
        return {"order": z, "event_start": np.zeros(1, dtype=np.int64), "t_min": z, "t_max": z, "hi": np.zeros(0)}
    a0, a1 = merged_windows(merged, fix0, fix1)
    gap = float(window_ns) * 1e3
    first = np.lexsort((merged["record_id"], merged["timestamp"], merged["dt"], a0))
    run_max = np.maximum.accumulate(a1[first])
    opens = np.ones(n, dtype=bool)
    opens[1:] = a0[first][1:] > run_max[:-1] + gap
    event = np.empty(n, dtype=np.int64)
    event[first] = np.cumsum(opens) - 1
    order = np.lexsort((merged["record_id"], merged["timestamp"], a0, merged["dt"], merged["channel"], merged["board"], event))
    n_events = int(event.max()) + 1
    event_start = np.searchsorted(event[order], np.arange(n_events + 1))
    lo = np.minimum.reduceat(a0[order], event_start[:-1])
    hi = np.maximum.reduceat(a1[order], event_start[:-1])
    return {"order": order, "event_start": event_start.astype(np.int64), "t_min": lo.astype(np.int64),
            "t_max": hi.astype(np.int64), "hi": hi}


def rows_of(merged: np.ndarray, ev: dict, first_event: int = 0, n_events: int | None = None) -> np.ndarray:
    """EVENT_MERGED_HIT_DTYPE rows of the first n_events events of a static_merged_events result."""
    k = len(ev["t_min"]) if n_events is None else int(n_events)
    stop = int(ev["event_start"][k])
    counts = np.diff(ev["event_start"][: k + 1])
    out = np.zeros(stop, dtype=EVENT_MERGED_HIT_DTYPE)
    out["event_id"] = np.repeat(first_event + np.arange(k, dtype=np.int64), counts)
    out["t_min"] = np.repeat(ev["t_min"][:k], counts)
    out["t_max"] = np.repeat(ev["t_max"][:k], counts)
    picked = merged[ev["order"][:stop]]
    for name in HIT_MERGED_DTYPE.names:
        out[name] = picked[name]
    return out


def static_rows(merged: np.ndarray, components: np.ndarray, hits: np.ndarray, window_ns: float) -> np.ndarray:
    """The static hit_grouped of a static hit_merged table (with hit_merged_components and hit_threshold), as rows."""
    index = np.asarray(components["hit_index"], dtype=np.int64)
    members = [index[int(o) : int(o) + int(c)] for o, c in zip(merged["component_offset"], merged["component_count"])]
    fix0, fix1 = member_windows(merged, members, hits)
    return rows_of(merged, static_merged_events(merged, fix0, fix1, window_ns))


def lowered(value: float, margin: float) -> float:
    """A computed window start lowered by three ulps of the run's magnitude (`margin` is two of them) and one step: no
    window computed another way from the same exact start lies below it.  Unchanged for margin 0 and for +inf."""
    value = float(value)
    if not margin > 0 or value == math.inf:
        return value
    return float(np.nextafter(np.float64(value) - 1.5 * margin, -np.inf))


class NumpyMergedEventStream:
    """push(rows, horizon) -> (event rows, hit_index of the clusters the merge step closed, hits carried, merged rows
    carried, G)."""

    def __init__(self, merge_gap_ns: float = 0.0, max_total_width_ns: float = 10000.0, time_window_ns: float = 100.0,
                 horizon_margin_ps: float = 0.0):
        self.merge = NumpyMergeStream(merge_gap_ns, max_total_width_ns)
        self.window_ns, self.margin = float(time_window_ns), float(horizon_margin_ps)
        self.carry = np.zeros(0, dtype=HIT_MERGED_DTYPE)
        self.fix0, self.fix1 = np.zeros(0), np.zeros(0)
        self.hits = np.zeros(0, dtype=THRESHOLD_HIT_DTYPE)     # every row pushed so far: what hit_index points into
        self.next_event = self.max_carry = 0
        self.group_horizon = -math.inf

    def push(self, rows, horizon: float):
        new = np.zeros(0, dtype=THRESHOLD_HIT_DTYPE) if rows is None else np.asarray(rows)
        self.hits = np.concatenate([self.hits, new])
        # 1. the merge step
        merged, hit_index, n_merge_carry, open_start = self.merge.push(rows, horizon)
        ends = np.cumsum(merged["component_count"].astype(np.int64))
        members = [hit_index[int(e - c) : int(e)] for e, c in zip(ends, merged["component_count"])]
        fix0, fix1 = member_windows(merged, members, self.hits)
        # 2. the grouping horizon
        previous = self.group_horizon
        g = self.group_horizon = max(previous, min(float(horizon), lowered(open_start, self.margin)))
        # 3. the group step over carry ++ the new merged rows, in the merge step's delivery order
        table = np.concatenate([self.carry, merged])
        fix0, fix1 = np.concatenate([self.fix0, fix0]), np.concatenate([self.fix1, fix1])
        if len(merged):
            assert merged_windows(merged, fix0[len(self.carry):], fix1[len(self.carry):])[0].min() >= previous, \
                "a merged row starts below the previous grouping horizon"
        ev = static_merged_events(table, fix0, fix1, self.window_ns)
        closed = ev["hi"] + self.window_ns * 1e3 < g
        k = len(closed) if closed.all() else int(np.argmin(closed))      # the closed prefix
        out = rows_of(table, ev, self.next_event, k)
        keep = np.ones(len(table), dtype=bool)
        keep[ev["order"][: int(ev["event_start"][k])]] = False
        self.carry, self.fix0, self.fix1 = table[keep], fix0[keep], fix1[keep]      # original row order
        self.next_event += k
        self.max_carry = max(self.max_carry, n_merge_carry + len(self.carry))
        return out, hit_index, n_merge_carry, len(self.carry), g


def stream_all(push, hits: np.ndarray, chunk_size: int, horizons: list | None = None):
    """Everything `push(rows, horizon)` delivers for `hits` in chunks of chunk_size, plus the flush: (event rows,
    hit_index), concatenated in delivery order."""
    horizons = row_horizons(hits, chunk_size) if horizons is None else horizons
    rows, members = [np.zeros(0, dtype=EVENT_MERGED_HIT_DTYPE)], [np.zeros(0, dtype=np.int64)]
    previous = -math.inf
    for k, lo in enumerate(range(0, len(hits), chunk_size)):
        out = push(hits[lo : lo + chunk_size], horizons[k])
        assert out[4] >= previous                                          # G never falls
        previous = out[4]
        rows.append(out[0])
        members.append(out[1])
    out = push(None, math.inf)
    assert out[2:] == (0, 0, math.inf)
    rows.append(out[0])
    members.append(out[1])
    return np.concatenate(rows), np.concatenate(members)


def assert_recorded(rows: np.ndarray, case: dict, tag: str) -> None:
    """The rows of all events against the g{k}_w{tw}_* columns the reference recorded."""
    ids = rows["event_id"]
    starts = np.concatenate([[0], np.flatnonzero(np.diff(ids)) + 1]) if len(rows) else np.zeros(0, dtype=np.int64)
    np.testing.assert_array_equal(ids[starts], np.arange(len(starts)))
    np.testing.assert_array_equal(rows["t_min"][starts], case[f"{tag}_t_min"])
    np.testing.assert_array_equal(rows["t_max"][starts], case[f"{tag}_t_max"])
    np.testing.assert_array_equal(np.diff(np.concatenate([starts, [len(rows)]])), case[f"{tag}_n_hits"])
    for column, field in PER_HIT:
        np.testing.assert_array_equal(rows[field], case[f"{tag}_{column}"], err_msg=f"{tag} {column}")


def fixture_margin(hits: np.ndarray) -> float:
    """Two ulps of the largest magnitude a window of the table reaches (0 below 2^53 ps): the run's margin when only the
    hit table is known."""
    a0, a1 = hit_windows(hits)
    m = float(max(np.abs(a0).max(), np.abs(a1).max(), np.abs(hits["timestamp"]).max()))
    return 0.0 if m < EXACT_LIMIT_PS else 2.0 * float(np.spacing(m))


def fixture_horizons(hits: np.ndarray, chunk_size: int, margin: float) -> list:
    """row_horizons -- the smallest COMPUTED abs_start among the rows of later chunks -- lowered like open_start: the rule
    asks for a horizon below every window computed from a later hit's exact start, the anchor formula of a cluster
    included."""
    return [lowered(h, margin) for h in row_horizons(hits, chunk_size)]


def assert_frames_equal(got, want):
    assert list(got.columns) == list(want.columns) == EVENT_COLUMNS and len(got) == len(want)
    for column in EVENT_COLUMNS:
        for a, b in zip(got[column], want[column]):
            assert np.array_equal(np.asarray(a), np.asarray(b)) and np.asarray(a).dtype == np.asarray(b).dtype, column


def assert_components(outs, rows, want_merged, want_components):
    """Every row's component_offset / component_count address the concatenation of all chunks' hit_index, and the members
    found there are the static components of the same merged row."""
    first = 0
    for o in outs:
        assert o.metadata["first_component"] == first and o.metadata["hit_index"].dtype == np.int64
        first += len(o.metadata["hit_index"])
    hit_index_all = np.concatenate([o.metadata["hit_index"] for o in outs])
    assert len(hit_index_all) == len(want_components) == int(rows["component_count"].sum())
    static_members = {}
    for row in want_merged:
        lo = int(row["component_offset"])
        key = (int(row["board"]), int(row["channel"]), int(row["timestamp"]), int(row["position"]), int(row["record_id"]),
               int(row["component_count"]))
        static_members.setdefault(key, []).append(want_components["hit_index"][lo : lo + int(row["component_count"])].tolist())
    for row in rows:
        lo = int(row["component_offset"])
        key = (int(row["board"]), int(row["channel"]), int(row["timestamp"]), int(row["position"]), int(row["record_id"]),
               int(row["component_count"]))
        assert hit_index_all[lo : lo + int(row["component_count"])].tolist() in static_members[key], key
    return hit_index_all


def late_pushes(same_channel: bool = False):
    """The construction of the merge stream's test at 2^60 ps: one ulp is 256 ps; dt = 3 ns and odd record timestamps make
    float(ts), the product and the sum all round.  16 records of two hits each, four records per push; the hits of a
    record share timestamp - position * dt.  `same_channel`: the two hits of a record lie in one channel, so that
    clusters form inside a record and take the anchor formula (as given, every cluster of several hits spans records).
    -> (pushes of (rows, horizon) without the flush, the run's margin)."""
    from waveformanalysis_amd.event_stream import horizon_margin, horizon_of

    rng = np.random.default_rng(11)
    n_rec = 16
    rec_ts = 2**60 + np.arange(n_rec, dtype=np.int64) * 1_000_003 + rng.integers(0, 255, n_rec)
    hits = np.zeros(2 * n_rec, dtype=THRESHOLD_HIT_DTYPE)
    for i in range(2 * n_rec):
        r = i // 2
        pos = int(rng.integers(3, 60))
        start = 0 if i % 2 == 0 else int(rng.integers(0, pos + 1))
        hits[i] = (pos, float(i), 1.0, start, pos + int(rng.integers(1, 9)), 0.0, 3, 0.0, 0.0, int(rec_ts[r]) + pos * 3000,
                   0, (r if same_channel else i) % 3, r)
    margin = horizon_margin(int(rec_ts.max()) + 3 * 1000 * 80)
    pushes = []
    for lo in range(0, n_rec, 4):                                          # four records (eight hits) per push
        later = int(rec_ts[lo + 4:].min()) if lo + 4 < n_rec else None
        pushes.append((hits[2 * lo : 2 * lo + 8], horizon_of(later, margin)))
    return pushes, margin


# ---- device doubles -----------------------------------------------------------------------------------------------------
class MergedEventOracleSession(OracleSession):
    """OracleSession that also answers the merged-event stream calls with NumpyMergedEventStream and records them."""

    def __init__(self, device_id: int = 0, log=None, uploads=None, calls=None):
        super().__init__(device_id, log, uploads)
        self.calls = [] if calls is None else calls
        self._stream = None

    def merged_event_stream_begin(self, merge_gap_ns, max_total_width_ns, time_window_ns, horizon_margin_ps=0.0):
        self.calls.append(("begin", float(merge_gap_ns), float(max_total_width_ns), float(time_window_ns),
                           float(horizon_margin_ps), self))
        self._stream = NumpyMergedEventStream(merge_gap_ns, max_total_width_ns, time_window_ns, horizon_margin_ps)

    def merged_event_stream_push(self, rows, horizon):
        assert self._stream is not None, "push without begin"
        self.calls.append(("push", 0 if rows is None else len(rows), float(horizon), self))
        return self._stream.push(rows, horizon)

    def merged_event_stream_end(self):
        self.calls.append(("end", self))
        self._stream = None


def merged_event_pool(device_ids=(0,), **kw):
    from waveformanalysis_amd.device import DevicePool

    log, uploads, calls = [], [], []
    pool = DevicePool(device_ids=list(device_ids),
                      session_factory=lambda dev: MergedEventOracleSession(dev, log, uploads, calls), **kw)
    pool.log, pool.uploads, pool.calls = log, uploads, calls
    return pool


__all__ = ["NumpyMergedEventStream", "MergedEventOracleSession", "merged_event_pool", "stream_all", "static_rows",
           "static_merged_events", "rows_of", "member_windows", "merged_windows", "hit_windows", "lowered", "assert_recorded",
           "fixture_margin", "fixture_horizons", "assert_frames_equal", "assert_components", "late_pushes", "fixture", "FIXTURES", "CPU_CHUNK_SIZES", "chunk_size_of", "make_hits",
           "row_horizons", "THRESHOLD_HIT_DTYPE"]
