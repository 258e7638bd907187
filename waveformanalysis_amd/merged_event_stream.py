"""HipHitMergedGroupedStream -- `hit_grouped` over `hit_merged`, chunk by chunk: the last link of the streaming hit chain.

The static hit_grouped consumes hit_merged whenever that product is registered, so with merging on
(merge_gap_ns > 0) the static chain always groups merged hits.  This stream does the same without the merged rows ever
visiting the host.  One push (threshold hit rows, H) does two steps on one session (wfa_merged_event_stream_*,
DeviceSession.merged_event_stream_begin / _push / _end):

1. the merge step -- the rule of hit_merged_stream (merge_stream.py): clusters close, the hits of the open ones stay in
   row order, open_start = the smallest computed abs_start still carried;
2. the group step -- the merged rows of the clusters just closed go behind the event carry in the merge step's delivery
   order ((board, channel), then chain order) and the grouping pass of the static entry runs over carry ++ new rows.
   A merged row with sample_start >= 0 and sample_end >= 0 takes the anchor formula; any other (its cluster spans
   records) takes min abs_start / max abs_end of its member hits, computed on the device when the cluster closes and
   carried with the row: the abs_start_fix / abs_end_fix of event_grouping._component_windows.  An event closes iff
   max(abs_end) + time_window_ns * 1e3 < G, strictly, under the grouping horizon

       G = max(G of the previous push, min(H, open_start'))

   because every merged row still to come starts at a carried hit or at a hit not yet seen.  open_start' is open_start
   itself below 2^53 ps, where min(H, open_start) never falls and the outer max changes nothing; beyond, it is open_start
   lowered by `open_start_margin`.

All pushes together give the static hit_grouped on hit_merged, whatever the chunk size.
"""

from __future__ import annotations

import math

import numpy as np

from .dtypes import EVENT_MERGED_HIT_DTYPE
from .event_stream import HitPushStream, events_frame
from .plugins.hit_grouped import HipHitGroupedPlugin
from .plugins.hit_merge import MERGE_OPTIONS
from .streaming import HipThresholdHitStream


def open_start_margin(horizon_margin_ps: float) -> float:
    """What to subtract from open_start so that no merged row still to come starts below it, given the run's
    `horizon_margin` (two ulps of the run's magnitude V beyond 2^53 ps, 0 below).  open_start is a computed member
    window; a future row's abs_start is either such a window again (a cluster that spans records: the very same
    float64) or the anchor formula of a one-record cluster, whose exact value is the exact start of the cluster's first
    member.  Each computed window lies within three roundings -- float(timestamp), the product, the sum, half an ulp of
    V each -- of its exact value, so the two differ by at most 3 ulp(V) = 1.5 * horizon_margin."""
    return 1.5 * float(horizon_margin_ps)


def lowered_open_start(open_start: float, horizon_margin_ps: float) -> float:
    """open_start' of the rule: open_start below 2^53 ps (margin 0) and for +inf (nothing carried), else
    nextafter(open_start - open_start_margin, -inf) (the subtraction rounds to nearest: one more step down)."""
    open_start = float(open_start)
    if not horizon_margin_ps > 0 or open_start == math.inf:
        return open_start
    return float(np.nextafter(open_start - open_start_margin(horizon_margin_ps), -np.inf))


def group_horizon(horizon: float, open_start: float, horizon_margin_ps: float = 0.0, previous: float = -math.inf) -> float:
    """G of one push: max(previous G, min(H, open_start'))."""
    return max(float(previous), min(float(horizon), lowered_open_start(open_start, horizon_margin_ps)))


def merged_events_frame(rows: np.ndarray):
    """The reference's hit_grouped DataFrame (EVENT_COLUMNS) from EVENT_MERGED_HIT_DTYPE rows; sample_starts /
    sample_ends come from sample_start / sample_end, as the static plugin takes them from hit_merged."""
    return events_frame(rows, ("sample_start", "sample_end"))


class HipHitMergedGroupedStream(HitPushStream):
    """compute() = the coincidence events of the merged hits of the records stream, delivered as they close (HitPushStream
    with wfa_merged_event_stream_*).

    A result chunk holds the EVENT_MERGED_HIT_DTYPE rows of the events one push closed, bounds
    [min t_min, max t_max + 1); a push that closes nothing yields nothing.  Metadata: `first_event`, `n_merge_carry`
    (hits of open clusters on the device) and `n_event_carry` (merged rows of open events), `group_horizon` (G), and
    `hit_index` (int64) with `first_component`: the members of every cluster the merge step closed since the previous
    delivered chunk, concatenated, and their offset in the concatenation over all chunks.  A row's component_offset /
    component_count address that concatenation, which is the component sequence hit_merged_stream delivers; a row's
    members may therefore have arrived with an earlier chunk.  `merged_events_frame(all rows)` is the DataFrame of
    HipHitGroupedPlugin on the static merge chain under the same configuration.

    Options: those of hit_threshold_stream, `merge_gap_ns` / `max_total_width_ns` with hit_merged's names and defaults,
    `time_window_ns` / `dt` with hit_grouped's.  The stream's rows always carry dt, so `dt` is read for parity only.

    Refused on the host, before any upload: a negative gap, width or window, and a device pool with fewer than three
    sessions (two for the hit ring, one for merge and grouping)."""

    provides = "hit_merged_grouped_stream"
    description = "Coincidence events of the merged hits of the records stream, delivered as they close (HIP, gfx950)."
    output_dtype = EVENT_MERGED_HIT_DTYPE
    output_data_kind = "events"
    output_time_field = "t_min"
    output_endtime_field = "t_max"
    role = "merge and grouping"

    options = {**HipThresholdHitStream.options, **MERGE_OPTIONS, **HipHitGroupedPlugin.options}

    def _check_cfg(self, cfg: dict) -> None:
        for name in ("merge_gap_ns", "max_total_width_ns", "time_window_ns"):
            cfg[name] = float(cfg[name])
            if not cfg[name] >= 0:
                raise ValueError(f"{name} must be >= 0")

    counters = ("events", "components")

    def _new_stats(self) -> dict:
        self._pending_index: list = []
        self._delivered_components = 0
        return super()._new_stats()

    def _run_margin(self, margin: float) -> None:
        self._margin = float(margin)

    def _begin(self, sess, cfg: dict) -> None:
        sess.merged_event_stream_begin(cfg["merge_gap_ns"], cfg["max_total_width_ns"], cfg["time_window_ns"],
                                       getattr(self, "_margin", 0.0))

    def _end(self, sess) -> None:
        sess.merged_event_stream_end()

    def _push(self, sess, rows, horizon: float, run_id: str, stats: dict):
        out, hit_index, n_merge_carry, n_event_carry, g = sess.merged_event_stream_push(rows, horizon)
        # (hits of open clusters + merged rows of open events: what the device holds between pushes)
        self._count_push(stats, rows, len(out), int(n_merge_carry) + int(n_event_carry))
        stats["components"] += len(hit_index)
        if len(hit_index):
            self._pending_index.append(hit_index)
        if len(out) == 0:
            return None
        members = np.concatenate(self._pending_index) if self._pending_index else np.zeros(0, dtype=np.int64)
        first_component = self._delivered_components
        self._pending_index = []
        self._delivered_components += len(members)
        return self._events_chunk(out, run_id, stats, n_merge_carry=int(n_merge_carry), n_event_carry=int(n_event_carry),
                                  group_horizon=float(g), hit_index=members, first_component=first_component)


__all__ = ["HipHitMergedGroupedStream", "merged_events_frame", "group_horizon", "lowered_open_start", "open_start_margin",
           "EVENT_MERGED_HIT_DTYPE"]
