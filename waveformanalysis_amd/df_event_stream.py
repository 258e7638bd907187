"""HipGroupedEventsStream -- `df_events` chunk by chunk: the features and fixed-window coincidence events of the records
stream, with the rows of the event still open kept on the device between chunks.

The default chain records + wave_pool -> basic_features -> df -> df_events -> df_paired works on a whole run.  Its
grouping rule (event_grouping.py: find_cluster_boundaries, _group_multi_channel_order_host): after a stable sort by
timestamp an event takes every row whose timestamp is <= (double)first + window in float64, and inside an event the rows
stand by channel (stable).  Events are anchored at their first row and compare raw integer timestamps, so the horizon of
a push is an int64 H with every row not yet pushed at timestamp >= H, and an event with anchor a is closed iff
(double)H > (double)a + window, strictly: the conversion is monotone, so a later row has
(double)ts >= (double)H > (double)a + window >= (double) of every member and can neither join nor precede it.  No float
margin is needed.  The rows of all other events (the carry, in row order) are chained again with the next chunk's rows;
the last chunk is pushed final.  Holding back more than necessary only delays rows: all chunks together give the static
table, whatever the chunk size.

The device part is wfa_df_event_stream_* (DeviceSession.df_event_stream_begin / _push / _end).  The 40-byte rows take one
host hop: a features session downloads a chunk's basic_features rows, `df_rows` joins them with the chunk's records, and
the push uploads them to the grouping session.
"""

from __future__ import annotations

import copy
from typing import Any

import numpy as np

from .device import DevicePool
from .dtypes import DF_EVENT_ROW_DTYPE, DF_ROW_DTYPE
from .features_stream import HipBasicFeaturesStream
from .plugin_api import Option
from .plugins.event_analysis import _remember, build_events_frame, pair_events
from .push_stream import PushStream, later_minima

FEATURE_OPTION_NAMES = tuple(HipBasicFeaturesStream.options)
HORIZON_END = int(np.iinfo(np.int64).max)   # the horizon of the last push: nothing follows


def df_rows(records: np.ndarray, features: np.ndarray) -> np.ndarray:
    """DF_ROW_DTYPE rows of one chunk: timestamp, board and channel from the records, record_id from the records' column
    (the row's index in the run, the features' event_index, when there is none), the four features from basic_features:
    the columns of HipDataFramePlugin's records branch, before its sort."""
    n = len(records)
    if len(features) != n:
        raise ValueError(f"basic_features length ({len(features)}) != records length ({n})")
    names = records.dtype.names or ()
    out = np.zeros(n, dtype=DF_ROW_DTYPE)
    out["timestamp"] = records["timestamp"]
    out["record_id"] = records["record_id"] if "record_id" in names else features["event_index"]
    for name in ("area", "height", "amp", "max_abs_diff"):
        out[name] = features[name]
    if "board" in names:
        out["board"] = records["board"]
    if "channel" in names:
        out["channel"] = records["channel"]
    return out


def chunk_horizons_ts(chunks: list) -> list[int]:
    """One int64 horizon per records chunk: the minimum record timestamp over all records of LATER chunks (a suffix
    minimum, taken once per run; correct for unsorted runs as well); HORIZON_END for the last chunk."""
    return [HORIZON_END if later is None else later for later in later_minima(chunks)]


def grouped_events_frame(rows: np.ndarray):
    """The MULTI_CHANNEL_COLUMNS frame of HipGroupedEventsPlugin from DF_EVENT_ROW_DTYPE rows: one frame row per run of
    equal event_id, the per-row columns as arrays in row order."""
    import pandas as pd

    from .event_grouping import MULTI_CHANNEL_COLUMNS

    if len(rows) == 0:
        return pd.DataFrame(columns=MULTI_CHANNEL_COLUMNS)
    ids = rows["event_id"]
    bounds = np.concatenate([[0], np.flatnonzero(ids[1:] != ids[:-1]) + 1, [len(rows)]]).astype(np.int64)
    cols = [np.ascontiguousarray(rows[name]) for name in ("timestamp", "channel", "area", "height")]
    frame, flat = build_events_frame(np.arange(len(rows), dtype=np.int64), bounds, *cols)
    frame["event_id"] = ids[bounds[:-1]].astype(np.int64)
    _remember(frame, flat)
    return frame


def paired_events_frame(rows: np.ndarray, time_window_ns: float = 100.0, n_channels: int = 2, start_channel_slice: int = 6):
    """pair_events (HipPairedEventsPlugin) on grouped_events_frame(rows).  Pairing is per event, so it commutes with
    chunking: the frames of the result chunks, concatenated, are the frame of all rows."""
    return pair_events(grouped_events_frame(rows), time_window_ns, n_channels=n_channels,
                       start_channel_slice=start_channel_slice)


class HipGroupedEventsStream(PushStream):
    """compute() = the df_events rows of the records stream, delivered as their events close (PushStream with
    wfa_df_event_stream_*).

    The records are chunked like hit_threshold_stream; an inner HipBasicFeaturesStream (same options, same chunking
    knobs; serial, or its thread-per-session `_compute_parallel`) computes every chunk's features.  `df_rows` of every
    chunk, empty ones included, go in chunk order to ONE more session borrowed for the whole run, with the chunk's
    horizon (`chunk_horizons_ts`); the last chunk is pushed final.

    A result chunk holds the DF_EVENT_ROW_DTYPE rows of the events one push closed, with bounds
    [min t_min, max t_max + 1) and metadata first_event / n_carry; a push that closes nothing yields nothing.
    `grouped_events_frame(all rows)` is the frame of HipGroupedEventsPlugin, `paired_events_frame` that of
    HipPairedEventsPlugin, of hip_full() under the same configuration with wave_source="records" for basic_features and
    df.  area_pe / height_pe are not in the rows: gains are a host lookup on (board, channel), left to the caller.

    Options: those of basic_features_stream, and `time_window_ns` (default 100.0, from df_events).  Refused on the host,
    before any upload: what basic_features_stream refuses, time_window_ns < 0, and a device pool with fewer than three
    sessions (two for the features, one for the grouping)."""

    provides = "df_events_stream"
    description = "Fixed-window coincidence events of the records stream, delivered as they close (HIP, gfx950)."
    output_dtype = DF_EVENT_ROW_DTYPE
    output_data_kind = "events"
    output_time_field = "t_min"
    output_endtime_field = "t_max"
    role = "grouping"

    options = {**HipBasicFeaturesStream.options, "time_window_ns": Option(default=100.0, type=float)}

    counters = ("events",)

    def _sessions(self) -> str:
        return f"one session for the {self.role}, held for the whole run, and two for the features of the chunks"

    def _check_cfg(self, cfg: dict) -> None:
        cfg["time_window_ns"] = float(cfg["time_window_ns"])
        if not cfg["time_window_ns"] >= 0:
            raise ValueError("time_window_ns must be >= 0")
        self._inner(cfg, None)   # (its constructor resolves and refuses the feature options)

    def _inner(self, cfg: dict, pool: DevicePool | None) -> HipBasicFeaturesStream:
        """The features stream with this stream's resolved options as its constructor values and this stream's chunking
        knobs."""
        inner = HipBasicFeaturesStream(device_pool=pool, **{name: cfg[name] for name in FEATURE_OPTION_NAMES})
        inner.chunk_size, inner.break_threshold_ps = self.chunk_size, self.break_threshold_ps
        return inner

    def run_chunks(self, chunks: list, context: Any, run_id: str, max_workers: int | None = None,
                   first_event_time: list | None = None):
        """Generator over the result chunks of ready-made records chunks (what compute() cuts).  `first_event_time`
        (optional list) receives time.perf_counter() when the first rows are delivered."""
        cfg = self._configure(context)
        pool = self._pool(context)
        self._check_pool(pool)
        inner = self._inner(cfg, pool)
        # event_index counts through THIS list: the inner stream gets shallow copies that carry their own record_base (a
        # value left in the caller's metadata by another cut neither wins nor is touched)
        numbered, base = [], 0
        for c in chunks:
            own = copy.copy(c)
            own.metadata = {**c.metadata, "record_base": base}
            numbered.append(own)
            base += len(c.data)
        chunks = numbered
        horizons = chunk_horizons_ts(chunks)
        stats = self.stats = self._new_stats()
        if not self.parallel or (max_workers is not None and int(max_workers) <= 1):
            features = ((c, inner._compute_one(c, context, run_id, inner.cfg)) for c in chunks)
        else:
            # the grouping session is borrowed first and for the whole run: the workers may take what is left, no more
            workers = int(pool.max_sessions) - 1
            if max_workers:
                workers = min(workers, int(max_workers))
            features = self._parallel_features(inner, chunks, context, run_id, workers)
        last = len(chunks) - 1
        yield from self._push_loop(pool, cfg, features, len(chunks),
                                   lambda k, chunk, raw: (df_rows(chunk.data, raw.data), horizons[k], k == last),
                                   None, run_id, stats, first_event_time)

    @staticmethod
    def _parallel_features(inner, chunks: list, context: Any, run_id: str, workers: int):
        """(chunk, features chunk) pairs in order from the inner stream's worker threads; closing this generator closes
        theirs (what has not started is cancelled, the sessions come back)."""
        results = inner._compute_parallel(iter(chunks), context, run_id, executor_config={"max_workers": workers})
        try:
            yield from zip(chunks, results)
        finally:
            results.close()

    def _begin(self, sess, cfg: dict) -> None:
        sess.df_event_stream_begin(cfg["time_window_ns"])

    def _end(self, sess) -> None:
        sess.df_event_stream_end()

    def _push(self, sess, rows, horizon: int, final: bool, run_id: str, stats: dict):
        out, n_carry = sess.df_event_stream_push(rows, horizon, final)
        self._count_push(stats, rows, len(out), n_carry)
        return self._events_chunk(out, run_id, stats, n_carry=int(n_carry))


__all__ = ["HipGroupedEventsStream", "df_rows", "chunk_horizons_ts", "grouped_events_frame", "paired_events_frame",
           "DF_ROW_DTYPE", "DF_EVENT_ROW_DTYPE", "HORIZON_END"]
