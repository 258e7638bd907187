"""The event stream's rule restated in numpy, and builders for hand-made hit rows.

`static_events` is the static grouping (lexsort by abs_start, running maximum of abs_end, second lexsort inside events);
`NumpyStream` is the stream on top of it: carry ++ new rows, closed prefix under a horizon, carry in original row order.
Both are written against the rule, not against the library: the CPU tests compare them with each other and with the
frames the reference recorded, the GPU tests compare the library with its own static pass.
"""

from __future__ import annotations

import math
import os

import numpy as np

from tests.stream_hits_util import OracleSession
from waveformanalysis_amd.dtypes import EVENT_HIT_DTYPE, THRESHOLD_HIT_DTYPE

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_TABLES = ("grouping_v1725", "grouping_vx2730")
PER_HIT = (("dt", "dt"), ("boards", "board"), ("channels", "channel"), ("heights", "height"), ("integrals", "integral"),
           ("timestamps", "timestamp"), ("record_ids", "record_id"), ("sample_starts", "edge_start"),
           ("sample_ends", "edge_end"))


def golden(name: str):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    return z["hits"], [float(w) for w in z["windows"]], z


def windows_of(rows: np.ndarray):
    t = rows["timestamp"].astype(np.float64)
    p = rows["position"].astype(np.float64)
    dps = rows["dt"].astype(np.float64) * 1e3
    return t + (rows["edge_start"].astype(np.float64) - p) * dps, t + (rows["edge_end"].astype(np.float64) - p) * dps


def static_events(hits: np.ndarray, window_ns: float) -> dict:
    """order (hit indices, event-major), event_start, t_min, t_max (truncated) and hi (float max abs_end) per event."""
    n = len(hits)
    if n == 0:
        z = np.zeros(0, dtype=np.int64)
        return {"order": z, "event_start": np.zeros(1, dtype=np.int64), "t_min": z, "t_max": z, "hi": np.zeros(0)}
    a0, a1 = windows_of(hits)
    gap = float(window_ns) * 1e3
    first = np.lexsort((hits["record_id"], hits["timestamp"], hits["dt"], a0))
    run_max = np.maximum.accumulate(a1[first])
    opens = np.ones(n, dtype=bool)
    opens[1:] = a0[first][1:] > run_max[:-1] + gap
    event = np.empty(n, dtype=np.int64)
    event[first] = np.cumsum(opens) - 1
    order = np.lexsort((hits["record_id"], hits["timestamp"], a0, hits["dt"], hits["channel"], hits["board"], event))
    n_events = int(event.max()) + 1
    event_start = np.searchsorted(event[order], np.arange(n_events + 1))
    lo = np.minimum.reduceat(a0[order], event_start[:-1])
    hi = np.maximum.reduceat(a1[order], event_start[:-1])
    return {"order": order, "event_start": event_start.astype(np.int64), "t_min": lo.astype(np.int64),
            "t_max": hi.astype(np.int64), "hi": hi}


def rows_of(hits: np.ndarray, ev: dict, first_event: int = 0, n_events: int | None = None) -> np.ndarray:
    """EVENT_HIT_DTYPE rows of the first n_events events of a static_events result."""
    k = len(ev["t_min"]) if n_events is None else int(n_events)
    stop = int(ev["event_start"][k])
    counts = np.diff(ev["event_start"][: k + 1])
    out = np.zeros(stop, dtype=EVENT_HIT_DTYPE)
    out["event_id"] = np.repeat(first_event + np.arange(k, dtype=np.int64), counts)
    out["t_min"] = np.repeat(ev["t_min"][:k], counts)
    out["t_max"] = np.repeat(ev["t_max"][:k], counts)
    picked = hits[ev["order"][:stop]]
    for name in THRESHOLD_HIT_DTYPE.names:
        out[name] = picked[name]
    return out


def static_rows(hits: np.ndarray, window_ns: float) -> np.ndarray:
    return rows_of(hits, static_events(hits, window_ns))


class NumpyStream:
    """The stream's rule: push(rows, horizon) -> (rows of the closed prefix, rows carried)."""

    def __init__(self, window_ns: float):
        self.window_ns = float(window_ns)
        self.carry = np.zeros(0, dtype=THRESHOLD_HIT_DTYPE)
        self.next_event = 0
        self.max_carry = 0

    def push(self, rows, horizon: float):
        new = np.zeros(0, dtype=THRESHOLD_HIT_DTYPE) if rows is None else np.asarray(rows)
        table = np.concatenate([self.carry, new])
        ev = static_events(table, self.window_ns)
        closed = ev["hi"] + self.window_ns * 1e3 < horizon
        k = len(closed) if closed.all() else int(np.argmin(closed))      # the closed prefix
        out = rows_of(table, ev, self.next_event, k)
        keep = np.ones(len(table), dtype=bool)
        keep[ev["order"][: int(ev["event_start"][k])]] = False
        self.carry = table[keep]                                          # original row order
        self.next_event += k
        self.max_carry = max(self.max_carry, len(self.carry))
        return out, len(self.carry)


def row_horizons(hits: np.ndarray, chunk_size: int) -> list:
    """Horizon of every chunk of `chunk_size` consecutive rows: the smallest abs_start among the rows of later chunks
    (the definition itself); +inf for the last."""
    a0, _ = windows_of(hits)
    bounds = list(range(0, len(hits), chunk_size))
    return [float(a0[lo + chunk_size:].min()) if lo + chunk_size < len(hits) else math.inf for lo in bounds]


def stream_rows(push, hits: np.ndarray, chunk_size: int, horizons: list | None = None) -> np.ndarray:
    """All rows `push(rows, horizon) -> (rows, n_carry)` delivers for `hits` in chunks of chunk_size, plus the flush."""
    horizons = row_horizons(hits, chunk_size) if horizons is None else horizons
    parts = []
    for k, lo in enumerate(range(0, len(hits), chunk_size)):
        parts.append(push(hits[lo : lo + chunk_size], horizons[k])[0])
    out, n_carry = push(None, math.inf)
    assert n_carry == 0
    parts.append(out)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=EVENT_HIT_DTYPE)


def make_hits(specs) -> np.ndarray:
    """THRESHOLD_HIT_DTYPE rows from (abs_start_ps, length_ps, board, channel[, dt]) tuples: position 10, edge_start 10,
    so that timestamp = abs_start, and edge_end = 10 + length / (dt * 1e3); record_id = row index, height = row index."""
    out = np.zeros(len(specs), dtype=THRESHOLD_HIT_DTYPE)
    for i, spec in enumerate(specs):
        start, length, board, channel = spec[:4]
        dt = spec[4] if len(spec) > 4 else 2
        assert length % (dt * 1000) == 0
        out[i] = (10, float(i), 1.0, 10, 10 + length // (dt * 1000), 0.0, dt, 0.0, 0.0, start, board, channel, i)
    return out


# ---- device doubles -----------------------------------------------------------------------------------------------------
class EventOracleSession(OracleSession):
    """OracleSession that also answers the event stream calls with NumpyStream and records them in `calls`."""

    def __init__(self, device_id: int = 0, log=None, uploads=None, calls=None):
        super().__init__(device_id, log, uploads)
        self.calls = [] if calls is None else calls
        self._stream = None

    def event_stream_begin(self, time_window_ns):
        self.calls.append(("begin", float(time_window_ns), self))
        self._stream = NumpyStream(time_window_ns)

    def event_stream_push(self, rows, horizon):
        assert self._stream is not None, "push without begin"
        self.calls.append(("push", 0 if rows is None else len(rows), float(horizon), self))
        return self._stream.push(rows, horizon)

    def event_stream_end(self):
        self.calls.append(("end", self))
        self._stream = None


def event_pool(device_ids=(0,), **kw):
    from waveformanalysis_amd.device import DevicePool

    log, uploads, calls = [], [], []
    pool = DevicePool(device_ids=list(device_ids),
                      session_factory=lambda dev: EventOracleSession(dev, log, uploads, calls), **kw)
    pool.log, pool.uploads, pool.calls = log, uploads, calls
    return pool
