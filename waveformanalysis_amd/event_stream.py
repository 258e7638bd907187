"""HipHitGroupedStream -- `hit_grouped` chunk by chunk: the coincidence events of the records stream, with the hits of the
events still open kept on the device between chunks.

The reference groups the run's whole hit table at once (processing/event_grouping.py:286-471) and has no streaming form
of it (profiles.py names streaming_default() as not available yet).  The static rule: after a global sort by abs_start a
hit opens a new event iff abs_start > running max(abs_end) + gap.  An event can therefore be emitted as soon as no later
hit can reach it.  A horizon H is a float64 such that every hit not yet seen has computed abs_start >= H; an event of the
table at hand is closed iff max(abs_end) + gap < H, strictly.  The closed events are a prefix of the table's events, no
later hit can join or precede them, so they are final; the hits of all other events (the carry) are grouped again together
with the next chunk's hits.  After the last chunk H = +inf closes everything.  Holding back more than necessary only
delays rows, it never changes them: all chunks together give the static table, whatever the chunk size.

The device part is wfa_event_stream_* (DeviceSession.event_stream_begin / _push / _end): the carry stays in HBM, a push
runs the grouping pass of the static entry over carry ++ new rows and returns EVENT_HIT_DTYPE rows, one per hit of the
events it closed.
"""

from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Any

import numpy as np

from .device import DevicePool
from .dtypes import EVENT_HIT_DTYPE, THRESHOLD_HIT_DTYPE
from .event_grouping import EVENT_COLUMNS
from .plugins import _common as K
from .plugins.hit_grouped import HipHitGroupedPlugin
from .push_stream import PushStream, later_minima
from .streaming import HipThresholdHitStream

HIT_OPTION_NAMES = tuple(HipThresholdHitStream.options)
EXACT_LIMIT_PS = 2**53   # below it every int64 ps value, and so every abs window, is exact in float64


def abs_windows(rows: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(abs_start, abs_end) in float64 ps, rounded as the device and the reference round them:
    float(ts) + (float(edge) - float(position)) * (float(dt) * 1e3)."""
    t = rows["timestamp"].astype(np.float64)
    p = rows["position"].astype(np.float64)
    dps = rows["dt"].astype(np.float64) * 1e3
    return t + (rows["edge_start"].astype(np.float64) - p) * dps, t + (rows["edge_end"].astype(np.float64) - p) * dps


def horizon_margin(magnitude_ps: float) -> float:
    """What to subtract from float(minimum later record timestamp) so that it is a horizon, given the largest magnitude
    (ps) any timestamp, record end or record span of the run reaches.  Below 2^53 ps everything is exact: 0.  Beyond it
    four roundings stand between the integer bound and a later hit's computed abs_start -- float(minimum) itself,
    float(hit timestamp), the product (edge - position) * (dt * 1e3) and the final sum -- each at most half an ulp of a
    value whose magnitude the argument bounds: two ulps of it."""
    m = abs(float(magnitude_ps))
    if m < EXACT_LIMIT_PS:
        return 0.0
    return 2.0 * float(np.spacing(m))


def run_magnitude(records: np.ndarray) -> int:
    """Largest |value| in ps among the records' timestamps, their ends and their spans (Python ints: no overflow)."""
    if len(records) == 0:
        return 0
    ts = records["timestamp"].astype(np.int64)
    # (a hit's position may lie in the padding up to the run's longest record: the widest span at the largest dt)
    lo, hi = int(ts.min()), int(ts.max())
    width = int(records["dt"].max()) * 1000 * int(records["event_length"].max())
    return max(abs(lo), abs(hi), abs(lo) + width, abs(hi) + width)


def horizon_of(min_later_timestamp: int | None, margin: float) -> float:
    """The horizon of a push after which only records with timestamp >= min_later_timestamp follow (None: nothing
    follows)."""
    if min_later_timestamp is None:
        return math.inf
    h = float(min_later_timestamp)
    if margin > 0.0:
        h = float(np.nextafter(h - margin, -np.inf))   # (the subtraction rounds to nearest: one more step down)
    return h


def run_margin(chunks: list) -> float:
    """horizon_margin of the run the records chunks make up."""
    return horizon_margin(max((run_magnitude(c.data) for c in chunks if len(c.data)), default=0))


def chunk_horizons(chunks: list, margin: float | None = None) -> list[float]:
    """One horizon per records chunk: the minimum record timestamp over all records of LATER chunks (a suffix minimum,
    taken once per run; correct for unsorted runs as well), as float64 less the run's margin (`run_margin`, taken here
    unless given); +inf for the last chunk.
    A threshold hit has edge_start >= 0 and timestamp = record timestamp + position * dt * 1e3, so its abs_start is at
    least its record's timestamp."""
    if margin is None:
        margin = run_margin(chunks)
    return [horizon_of(later, margin) for later in later_minima(chunks)]


def event_rows(hits: np.ndarray, flat: dict, first_event: int = 0) -> np.ndarray:
    """EVENT_HIT_DTYPE rows from the flat form of the static pass (event_grouping.group_hit_windows_flat)."""
    order, es = np.asarray(flat["order"], dtype=np.int64), np.asarray(flat["event_start"], dtype=np.int64)
    counts = np.diff(es)
    out = np.zeros(len(order), dtype=EVENT_HIT_DTYPE)
    out["event_id"] = np.repeat(first_event + np.arange(len(counts), dtype=np.int64), counts)
    out["t_min"] = np.repeat(np.asarray(flat["t_min"], dtype=np.int64), counts)
    out["t_max"] = np.repeat(np.asarray(flat["t_max"], dtype=np.int64), counts)
    picked = hits[order]
    for name in THRESHOLD_HIT_DTYPE.names:
        out[name] = picked[name]
    return out


def events_frame(rows: np.ndarray, window_fields: tuple[str, str] = ("edge_start", "edge_end")):
    """The reference's hit_grouped DataFrame (EVENT_COLUMNS) from EVENT_HIT_DTYPE rows: one frame row per run of equal
    event_id, n_hits = the run's length, the per-hit columns as arrays in row order.  `window_fields` names the rows'
    sample window (merged rows call it sample_start / sample_end: merged_event_stream.merged_events_frame)."""
    import pandas as pd

    if len(rows) == 0:
        return pd.DataFrame(columns=EVENT_COLUMNS)
    ids = rows["event_id"]
    starts = np.concatenate([[0], np.flatnonzero(ids[1:] != ids[:-1]) + 1, [len(rows)]])
    cols = {"dt": ("dt", np.int32), "boards": ("board", np.int16), "channels": ("channel", np.int16),
            "heights": ("height", np.float32), "integrals": ("integral", np.float32), "timestamps": ("timestamp", np.int64),
            "record_ids": ("record_id", np.int64), "sample_starts": (window_fields[0], np.int32),
            "sample_ends": (window_fields[1], np.int32)}
    flat = {k: np.ascontiguousarray(rows[f], dtype=t) for k, (f, t) in cols.items()}
    out = []
    for a, b in zip(starts[:-1].tolist(), starts[1:].tolist()):
        t_min, t_max = int(rows["t_min"][a]), int(rows["t_max"][a])
        row = {"event_id": int(ids[a]), "t_min": t_min, "t_max": t_max, "dt/ns": (t_max - t_min) / 1e3, "n_hits": b - a}
        for k, v in flat.items():
            row[k] = v[a:b].copy()
        out.append(row)
    return pd.DataFrame(out, columns=EVENT_COLUMNS)


class HitPushStream(PushStream):
    """The push streams over the hit stream's rows (hit_grouped_stream here, hit_merged_stream in merge_stream.py,
    hit_merged_grouped_stream in merged_event_stream.py): PushStream with the inner hit stream and float horizons.

    The records are chunked like hit_threshold_stream; an inner HipThresholdHitStream (same options, same ring of two
    sessions per device, same overlap of upload and kernels) finds every chunk's hits.  Each chunk's rows, empty ones
    included, go in order to ONE more session borrowed for the whole run, with the chunk's horizon (`chunk_horizons`);
    after the last chunk one push with +inf.

    The rows travel device -> host -> device once more than necessary: the ring's sessions download a chunk's 60-byte
    rows (the hit stream's product), and the push uploads them to the borrowed session."""

    def __init__(self, device_pool: DevicePool | None = None, max_len: int = 0, **given):
        self.max_len = int(max_len)
        super().__init__(device_pool, **given)

    def _inner(self, cfg: dict, pool: DevicePool) -> HipThresholdHitStream:
        """The hit stream with this stream's resolved options as its constructor values (so they win in its own
        _configure) and this stream's chunking knobs."""
        given = {name: cfg[name] for name in HIT_OPTION_NAMES}
        if str(given["filter_source"]) == "wave_pool_filtered":  # (that plugin's filter settings: none of our own)
            given.pop("sg_window_size"), given.pop("sg_poly_order")
        inner = HipThresholdHitStream(max_len=self.max_len, device_pool=pool, **given)
        inner.chunk_size, inner.break_threshold_ps = self.chunk_size, self.break_threshold_ps
        return inner

    def _run_margin(self, margin: float) -> None:
        """Told the run's horizon margin (ps; `run_margin`) before `_begin`, for a device stream that takes it."""

    def _sessions(self) -> str:
        return f"two sessions for the hit ring, one for the {self.role}"

    def run_chunks(self, chunks: list, context: Any, run_id: str, max_workers: int | None = None,
                   first_event_time: list | None = None):
        """Generator over the result chunks of ready-made records chunks (what compute() cuts).  `first_event_time`
        (optional list) receives time.perf_counter() when the first rows are delivered."""
        cfg = self._configure(context)
        self._check_scope(context)
        pool = self._pool(context)
        self._check_pool(pool)
        inner = self._inner(cfg, pool)
        margin = run_margin(chunks)
        horizons = chunk_horizons(chunks, margin)
        self._run_margin(margin)
        stats = self.stats = self._new_stats()
        if not self.parallel or (max_workers is not None and int(max_workers) <= 1):
            inner._configure(context)
            width, plan = inner._run_width(context, run_id, chunks), inner._run_plan(context, run_id, chunks)
            hits = ((c, inner._compute_one(c, context, run_id, width, plan)) for c in chunks)
        else:
            # the push session is borrowed first and for the whole run: the ring may take what is left, no more
            ring = int(pool.max_sessions) - 1
            hits = inner._pipeline(chunks, context, run_id, max_workers=min(ring, int(max_workers)) if max_workers else ring)
        yield from self._push_loop(pool, cfg, hits, len(chunks), lambda k, _chunk, raw: (raw.data, horizons[k]),
                                   (None, math.inf), run_id, stats, first_event_time)


class HipHitGroupedStream(HitPushStream):
    """compute() = the events of the records stream, delivered as they close (HitPushStream with wfa_event_stream_*).

    A result chunk holds the EVENT_HIT_DTYPE rows of the events one push closed, with bounds
    [min t_min, max t_max + 1); a push that closes nothing yields nothing.  `events_frame(all rows)` is the DataFrame of
    HipHitGroupedPlugin on HipThresholdHitPlugin's rows under the same configuration.

    Options: those of hit_threshold_stream, and `time_window_ns` / `dt` with hit_grouped's names and defaults.  The
    stream's rows always carry dt (the records'), so `dt` is read for parity only, as the static plugin ignores it when
    its hits have the column.

    Refused on the host, before any upload: a Context whose configuration sets merge_gap_ns > 0 for hit_merged (the
    static plugin would then group merged hits, which the stream does not build), and a device pool with fewer than three
    sessions (two for the ring, one for the grouping).  The stream that does group merged hits is hit_merged_grouped_stream
    (merged_event_stream.py); this one keeps its refusal, so that a configuration with merging never silently gets events
    of unmerged hits."""

    provides = "hit_grouped_stream"
    description = "Coincidence events of the records stream, delivered as they close (HIP, gfx950)."
    output_dtype = EVENT_HIT_DTYPE
    output_data_kind = "events"
    output_time_field = "t_min"
    output_endtime_field = "t_max"
    role = "grouping"

    options = {**HipThresholdHitStream.options, **HipHitGroupedPlugin.options}

    def _check_cfg(self, cfg: dict) -> None:
        cfg["time_window_ns"] = float(cfg["time_window_ns"])
        if cfg["time_window_ns"] < 0:
            raise ValueError("time_window_ns must be >= 0")

    def _check_scope(self, context: Any) -> None:
        if not isinstance(getattr(context, "config", None), dict):
            return
        gap = K.raw_config(context, SimpleNamespace(provides="hit_merged"), "merge_gap_ns")
        if gap is not None and float(gap) > 0:
            raise ValueError(f"hit_grouped_stream: the configuration sets merge_gap_ns = {gap!r} for hit_merged; the static "
                             "hit_grouped would group merged hits, the stream groups threshold hits only")

    counters = ("events",)

    def _begin(self, sess, cfg: dict) -> None:
        sess.event_stream_begin(cfg["time_window_ns"])

    def _end(self, sess) -> None:
        sess.event_stream_end()

    def _push(self, sess, rows, horizon: float, run_id: str, stats: dict):
        out, n_carry = sess.event_stream_push(rows, horizon)
        self._count_push(stats, rows, len(out), n_carry)
        return self._events_chunk(out, run_id, stats, n_carry=int(n_carry))


__all__ = ["HipHitGroupedStream", "HitPushStream", "events_frame", "event_rows", "chunk_horizons", "horizon_of", "horizon_margin",
           "run_magnitude", "run_margin", "abs_windows", "EVENT_HIT_DTYPE"]
