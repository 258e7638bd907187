"""The df_events stream's rule restated in numpy, the static rows it must add up to, and the recorded frames.

`static_rows` is the static grouping (`_group_multi_channel_order_host`) written out as DF_EVENT_ROW_DTYPE rows;
`NumpyDfStream` is the stream on top of the same host pass: carry ++ new rows, the closed prefix under an int64 horizon,
the carry in original row order.  Both are written against the rule, not against the library's device code: the CPU tests
compare them with each other and with the frames the reference recorded (tests/golden/legacy_events_df.npz), the GPU
tests compare the library with them and with its own static device pass.
"""

from __future__ import annotations

import json

import numpy as np

from tests import events_util as E
from tests.stream_hits_util import OracleSession
from waveformanalysis_amd.dtypes import BASIC_FEATURES_DTYPE, DF_EVENT_ROW_DTYPE, DF_ROW_DTYPE
from waveformanalysis_amd.event_grouping import _group_multi_channel_order_host

FIXTURE_CASES = ("records_plain", "pair_drop_all", "window_0", "window_5000", "pair_drop_some")
HORIZON_END = int(np.iinfo(np.int64).max)
COPIED = ("timestamp", "record_id", "area", "height", "amp", "max_abs_diff", "board", "channel")


def make_rows(ts, ch, board=None) -> np.ndarray:
    """DF_ROW_DTYPE rows from timestamps and channels: record_id = row index, the features functions of it."""
    n = len(ts)
    out = np.zeros(n, dtype=DF_ROW_DTYPE)
    out["timestamp"], out["channel"] = ts, ch
    out["board"] = 0 if board is None else board
    out["record_id"] = np.arange(n)
    out["area"], out["height"] = 100.0 + np.arange(n), 0.5 * np.arange(n)
    out["amp"], out["max_abs_diff"] = 7.0 - np.arange(n), 3.0 * np.arange(n) + 0.25
    return out


def events_of(rows: np.ndarray, window_ns: float):
    """(order, bounds) of the static host pass over the rows' timestamps and channels."""
    if len(rows) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64)
    return _group_multi_channel_order_host(rows["timestamp"], rows["channel"], float(window_ns) * 1e3)


def rows_of(rows: np.ndarray, order: np.ndarray, bounds: np.ndarray, first_event: int = 0, n_events: int | None = None):
    """DF_EVENT_ROW_DTYPE rows of the first n_events events of a grouping."""
    k = len(bounds) - 1 if n_events is None else int(n_events)
    stop = int(bounds[k])
    counts = np.diff(bounds[: k + 1])
    picked = rows[order[:stop]]
    out = np.zeros(stop, dtype=DF_EVENT_ROW_DTYPE)
    for name in COPIED:
        out[name] = picked[name]
    if stop:
        out["event_id"] = np.repeat(first_event + np.arange(k, dtype=np.int64), counts)
        out["t_min"] = np.repeat(picked["timestamp"][bounds[:k]], counts)        # first / last row after the channel sort
        out["t_max"] = np.repeat(picked["timestamp"][bounds[1 : k + 1] - 1], counts)
        out["n_hits"] = np.repeat(counts, counts)
    return out


def static_rows(rows: np.ndarray, window_ns: float) -> np.ndarray:
    return rows_of(rows, *events_of(rows, window_ns))


class NumpyDfStream:
    """The stream's rule: push(rows, horizon, final) -> (rows of the closed prefix, rows carried)."""

    def __init__(self, window_ns: float):
        self.window_ps = float(window_ns) * 1e3
        self.window_ns = float(window_ns)
        self.carry = np.zeros(0, dtype=DF_ROW_DTYPE)
        self.next_event = 0
        self.max_carry = 0

    def push(self, rows, horizon: int, final: bool = False):
        new = np.zeros(0, dtype=DF_ROW_DTYPE) if rows is None else np.asarray(rows)
        table = np.concatenate([self.carry, new])
        order, bounds = events_of(table, self.window_ns)
        n_events = len(bounds) - 1
        anchors = np.sort(table["timestamp"], kind="stable")[bounds[:-1]].astype(np.float64)
        closed = np.ones(n_events, dtype=bool) if final else float(np.int64(horizon)) > anchors + self.window_ps
        k = n_events if closed.all() else int(np.argmin(closed))             # the closed prefix
        out = rows_of(table, order, bounds, self.next_event, k)
        keep = np.ones(len(table), dtype=bool)
        keep[order[: int(bounds[k])]] = False
        self.carry = table[keep]                                              # original row order
        self.next_event += k
        self.max_carry = max(self.max_carry, len(self.carry))
        return out, len(self.carry)


def row_horizons(rows: np.ndarray, chunk_size: int) -> list:
    """Horizon of every chunk of `chunk_size` consecutive rows: the smallest timestamp among the rows of later chunks
    (the definition itself); HORIZON_END for the last."""
    ts = rows["timestamp"]
    return [int(ts[lo + chunk_size:].min()) if lo + chunk_size < len(rows) else HORIZON_END
            for lo in range(0, len(rows), chunk_size)]


def stream_rows(push, rows: np.ndarray, chunk_size: int, carries: list | None = None) -> np.ndarray:
    """All rows `push(rows, horizon, final) -> (rows, n_carry)` delivers for `rows` in chunks of chunk_size, the last
    chunk pushed final."""
    horizons = row_horizons(rows, chunk_size)
    parts = []
    for k, lo in enumerate(range(0, len(rows), chunk_size)):
        out, n_carry = push(rows[lo : lo + chunk_size], horizons[k], k == len(horizons) - 1)
        parts.append(out)
        if carries is not None:
            carries.append(n_carry)
    if horizons:
        assert n_carry == 0
    return np.concatenate(parts) if parts else np.zeros(0, dtype=DF_EVENT_ROW_DTYPE)


# ---- the recorded frames --------------------------------------------------------------------------------------------
def fixture():
    return E.load()


def fixture_setup(z, case: str) -> dict:
    return json.loads(str(z[f"{case}/setup"]))


def fixture_rows(z, case: str) -> tuple[np.ndarray, float]:
    """(DF_ROW_DTYPE rows of the case's table in table order, df_events' window in ns): the columns HipDataFramePlugin
    takes, before its sort."""
    setup = fixture_setup(z, case)
    table, bf = z[f"table/{setup['table']}"], z["bf"]
    out = np.zeros(len(table), dtype=DF_ROW_DTYPE)
    out["timestamp"], out["record_id"] = table["timestamp"], table["record_id"]
    out["board"], out["channel"] = table["board"], table["channel"]
    for name in ("area", "height", "amp", "max_abs_diff"):
        out[name] = bf[name]
    return out, float(setup["config"]["df_events"]["time_window_ns"])


def pairing_args(z, case: str) -> dict:
    """What HipPairedEventsPlugin reads from the case's configuration."""
    cfg = fixture_setup(z, case)["config"]
    return {"time_window_ns": cfg.get("time_window_ns", 100.0), "n_channels": cfg.get("n_channels", 2),
            "start_channel_slice": cfg.get("start_channel_slice", 6)}


# ---- a device double for the plugin tests ------------------------------------------------------------------------------
class DfEventOracleSession(OracleSession):
    """OracleSession that answers basic_features with rows made from the uploaded records (height = record_id, area =
    timestamp mod 1000, ...) and the df_events stream calls with NumpyDfStream; every call is recorded in `calls`."""

    def __init__(self, device_id: int = 0, log=None, uploads=None, calls=None):
        super().__init__(device_id, log, uploads)
        self.calls = [] if calls is None else calls
        self._stream = None

    def upload_pool(self, pool):
        self.calls.append(("upload_pool", int(pool.size), self))
        super().upload_pool(pool)

    def upload_records(self, rec, thr=10.0):
        self.calls.append(("upload_records", len(rec), self))
        super().upload_records(rec, thr)

    def basic_features(self, source=0, height_range=(40, 90), area_range=(0, None), fixed_baseline=None, out=None):
        rec = self._rec
        self.calls.append(("basic_features", len(rec), tuple(height_range), tuple(area_range),
                           None if fixed_baseline is None else np.array(fixed_baseline), self))
        return oracle_features(rec, fixed_baseline)

    def df_event_stream_begin(self, time_window_ns):
        self.calls.append(("begin", float(time_window_ns), self))
        self._stream = NumpyDfStream(time_window_ns)

    def df_event_stream_push(self, rows, horizon_ts, final=False):
        assert self._stream is not None, "push without begin"
        self.calls.append(("push", 0 if rows is None else len(rows), int(horizon_ts), bool(final), self))
        return self._stream.push(rows, horizon_ts, final)

    def df_event_stream_end(self):
        self.calls.append(("end", self))
        self._stream = None


def oracle_features(rec: np.ndarray, fixed_baseline=None) -> np.ndarray:
    """The double's BASIC_FEATURES_DTYPE rows: functions of the record alone, event_index counting the pass from 0."""
    out = np.zeros(len(rec), dtype=BASIC_FEATURES_DTYPE)
    out["height"] = rec["record_id"] % 977 if "record_id" in rec.dtype.names else 0.0
    out["amp"] = rec["event_length"]
    out["area"] = rec["timestamp"] % 1000
    out["max_abs_diff"] = 0.0 if fixed_baseline is None else np.nan_to_num(fixed_baseline, nan=-1.0)
    out["timestamp"], out["board"], out["channel"] = rec["timestamp"], rec["board"], rec["channel"]
    out["event_index"] = np.arange(len(rec))
    return out


def df_event_pool(device_ids=(0,), **kw):
    from waveformanalysis_amd.device import DevicePool

    log, uploads, calls = [], [], []
    pool = DevicePool(device_ids=list(device_ids),
                      session_factory=lambda dev: DfEventOracleSession(dev, log, uploads, calls), **kw)
    pool.log, pool.uploads, pool.calls = log, uploads, calls
    return pool


__all__ = ["FIXTURE_CASES", "HORIZON_END", "make_rows", "events_of", "rows_of", "static_rows", "NumpyDfStream",
           "row_horizons", "stream_rows", "fixture", "fixture_rows", "pairing_args", "DfEventOracleSession",
           "oracle_features", "df_event_pool"]
