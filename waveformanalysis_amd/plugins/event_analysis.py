"""HipGroupedEventsPlugin / HipPairedEventsPlugin -- drop-ins for GroupedEventsPlugin and PairedEventsPlugin
(reference: waveform_analysis/core/plugins/builtin/cpu/event_analysis.py:23-66,109-144, which call
EventAnalyzer.group_events / pair_events, core/processing/analyzer.py:42-111).

df_events groups the df rows on the GPU (wfa_group_multi_channel_*: stable sort by timestamp, the fixed-window chain,
stable sort by (event, channel)) and returns the reference's table with one ragged array per event in each of
`channels`, `areas`, `heights` and `timestamps`.  Those object columns are built on the host, one basic slice of an
event-major array per event and column: this is the part of the stage whose cost grows with the number of events.

df_paired filters the events by their time span and takes the first `n_channels` areas / heights of every event by
position.  It reads the flat event-major arrays df_events built (remembered per returned frame, see `_remember`) and
only falls back to concatenating the ragged columns for a frame from elsewhere, such as a cache reload.
"""

from __future__ import annotations

import threading
import weakref
from typing import Any

import numpy as np

from ..event_grouping import MULTI_CHANNEL_COLUMNS, group_multi_channel_order
from ..plugin_api import Option, Plugin
from . import _common as K

# id(df_events frame) -> (weakref to the frame, flat event-major arrays); the entry goes with the frame
_flat_memo: dict[int, tuple[Any, dict]] = {}
_memo_lock = threading.Lock()


def _remember(frame, flat: dict) -> None:
    key = id(frame)

    def _drop(_ref, key=key):
        with _memo_lock:
            entry = _flat_memo.get(key)
            if entry is not None and entry[0] is _ref:
                del _flat_memo[key]

    with _memo_lock:
        _flat_memo[key] = (weakref.ref(frame, _drop), flat)


def _recall(frame) -> dict | None:
    with _memo_lock:
        entry = _flat_memo.get(id(frame))
    if entry is None or entry[0]() is not frame:
        return None
    return entry[1]


def _ragged(flat: np.ndarray, pieces: list) -> np.ndarray:
    """Object array of `flat[a:b]` for each slice in `pieces` (views; np.split costs about four times as much)."""
    out = np.empty(len(pieces), dtype=object)
    out[:] = list(map(flat.__getitem__, pieces))
    return out


def build_events_frame(order: np.ndarray, bounds: np.ndarray, ts_in: np.ndarray, ch_in: np.ndarray,
                       area_in: np.ndarray, height_in: np.ndarray):
    """(MULTI_CHANNEL_COLUMNS frame, flat arrays) of one grouping: event e holds input rows order[bounds[e]:bounds[e+1]]."""
    import pandas as pd

    ts_o, ch_o = ts_in[order], ch_in[order]
    ar_o, he_o = area_in[order], height_in[order]
    bounds = np.asarray(bounds, dtype=np.int64)
    starts, ends = bounds[:-1], bounds[1:]
    n_events = len(starts)
    bl = bounds.tolist()
    pieces = list(map(slice, bl[:-1], bl[1:]))
    frame = pd.DataFrame({
        "event_id": np.arange(n_events, dtype=np.int64),
        "t_min": ts_o[starts].astype(np.int64),        # first / last row after the channel sort, as the reference
        "t_max": ts_o[ends - 1].astype(np.int64),
        "dt/ns": (ts_o[ends - 1] - ts_o[starts]) / 1e3,
        "n_hits": np.diff(bounds).astype(np.int32),
        "channels": _ragged(ch_o, pieces),
        "areas": _ragged(ar_o, pieces),
        "heights": _ragged(he_o, pieces),
        "timestamps": _ragged(ts_o, pieces),
    })
    flat = {"bounds": bounds, "timestamps": ts_o, "areas": ar_o, "heights": he_o}
    return frame, flat


class HipGroupedEventsPlugin(K.HipPlugin):
    """Group the df rows across channels: a cluster takes every row within `time_window_ns` of its first row
    (after a stable sort by timestamp), and its rows are ordered by channel (stable).  The reference's sorts are
    unstable, so only the order of equal timestamps / equal channels inside an event can differ.
    `use_numba` and `n_processes` from the context config are accepted and ignored."""

    provides = "df_events"
    algorithmic_bytes = (0, 0, 80)  # device pass: bytes per sample, per record, per df row
    depends_on = ["df"]
    description = "Group events across channels within a configurable time window (GPU grouping)."
    version = "0.0.0+hip1"
    save_when = "always"
    options = {
        "time_window_ns": Option(default=100.0, type=float),
    }

    def compute(self, context: Any, run_id: str, **kwargs) -> Any:
        import pandas as pd

        df = context.get_data(run_id, "df")
        tw = context.get_config(self, "time_window_ns")
        if tw is None:  # EventAnalyzer keeps its 100 ns
            tw = 100.0
        grouped = group_multi_channel_order(df, tw, session=K.note_session(K._device_pool(context).session()))
        if grouped is None:
            return pd.DataFrame(columns=MULTI_CHANNEL_COLUMNS)
        frame, flat = build_events_frame(*grouped)
        _remember(frame, flat)
        return frame


def _flat_from_columns(df_events, areas_key: str, heights_key: str) -> dict:
    """Flat arrays of ragged columns (a frame df_events did not build here): per column its own lengths."""
    out = {}
    for name, key in (("timestamps", "timestamps"), ("areas", areas_key), ("heights", heights_key)):
        values = [x if isinstance(x, (list, np.ndarray)) else () for x in df_events[key].to_list()]
        lens = np.fromiter(map(len, values), dtype=np.int64, count=len(values))
        bounds = np.zeros(len(values) + 1, dtype=np.int64)
        np.cumsum(lens, out=bounds[1:])
        flat = np.concatenate([np.asarray(v) for v in values]) if bounds[-1] > 0 else np.zeros(0)
        out[name] = (flat, bounds)
    return out


def pair_events(df_events, time_window_ns: float, n_channels: int = 2, start_channel_slice: int = 6):
    """EventAnalyzer.pair_events (analyzer.py:67-111) on flat arrays: the events whose span `dt/ns` <= the window,
    with delta_t = (timestamps[-1] - timestamps[0]) / 1000 and area_ch{s+i} / height_ch{s+i} = the i-th entry of the
    event's areas / heights (NaN past its end) for i < n_channels.  No derived column when no event passes."""
    within = df_events["dt/ns"] <= time_window_ns
    paired = df_events[within].copy()
    if paired.empty:
        return paired
    areas_key = "areas" if "areas" in paired.columns else "charges"
    heights_key = "heights" if "heights" in paired.columns else "peaks"
    keep = np.flatnonzero(within.to_numpy())
    flat = _recall(df_events) if (areas_key, heights_key) == ("areas", "heights") else None
    if flat is not None and len(flat["bounds"]) == len(df_events) + 1:
        b = flat["bounds"]
        cols = {name: (flat[name], b[keep], b[keep + 1]) for name in ("timestamps", "areas", "heights")}
    else:
        built = _flat_from_columns(paired, areas_key, heights_key)
        cols = {name: (f, b[:-1], b[1:]) for name, (f, b) in built.items()}
    if "delta_t" not in paired.columns:
        ts, a, e = cols["timestamps"]
        paired["delta_t"] = (ts[e - 1] - ts[a]) / 1000.0
    for i in range(n_channels):
        for prefix, name in (("area_ch", "areas"), ("height_ch", "heights")):
            values, a, e = cols[name]
            present = (e - a) > i
            if present.all():  # pandas keeps the element dtype when no NaN is mixed in
                col = values[a + i]
            else:
                col = np.full(len(a), np.nan, dtype=np.float64)
                col[present] = values[a[present] + i]
            paired[f"{prefix}{start_channel_slice + i}"] = col
    return paired


class HipPairedEventsPlugin(Plugin):
    """Keep the grouped events whose time span is within the global `time_window_ns` (context.config, default
    100 ns -- not df_events' own option) and add delta_t and the per-position area / height columns
    (`n_channels`, default 2, starting at `start_channel_slice`, default 6, both from context.config).  Host table
    work on the flat arrays behind df_events; the reference applies a Python function per event and column."""

    provides = "df_paired"
    depends_on = ["df_events"]
    description = "Pair grouped events across channels for coincidence analysis."
    version = "0.0.0+hip1"
    save_when = "always"

    def compute(self, context: Any, run_id: str, **kwargs) -> Any:
        df_events = context.get_data(run_id, "df_events")
        n_channels = context.config.get("n_channels", 2)
        start_channel_slice = context.config.get("start_channel_slice", 6)
        time_window_ns = context.config.get("time_window_ns", 100.0)
        if time_window_ns is None:  # EventAnalyzer keeps its 100 ns
            time_window_ns = 100
        return pair_events(df_events, time_window_ns, n_channels=n_channels, start_channel_slice=start_channel_slice)


__all__ = ["HipGroupedEventsPlugin", "HipPairedEventsPlugin", "build_events_frame", "pair_events"]
