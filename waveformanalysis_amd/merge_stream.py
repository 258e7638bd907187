"""HipHitMergedStream -- `hit_merged` chunk by chunk: the merged hits of the records stream, with the hits of the
clusters still open kept on the device between chunks.

The reference merges the run's whole hit table at once (cpu/hit_merge.py:115-181): per hardware channel, ascending
(board, channel), the hits are ordered stably by abs_start and chained greedily -- a hit joins the current cluster iff
merge_gap_ns > 0, its dt equals the previous member's, abs_start - cluster_end <= gap and the total width stays within
max_total_width_ns.  Clusters are contiguous runs of a channel's sorted table, and a chain restarted at any cluster head
reproduces the rest.  So a cluster can be emitted as soon as no later hit can precede or join it.  With a horizon H (every
hit not yet seen has computed abs_start >= H) and F = the rows of the channel with abs_start < H, strictly, a cluster at
sorted positions [a, b) is closed iff b <= F and one of: b < F (the hit that broke the chain is itself final);
merge_gap_ns <= 0 (nothing ever joins); H - cluster_end > gap in float64 (a later hit's computed gap is at least that:
float subtraction is monotone).  Closed clusters are a prefix of every channel's clusters and final; the hits of all others
(the carry) stay in their original row order, so that ties of the stable sort fall where the whole table would put them,
and are chained again together with the next chunk's hits.  After the last chunk H = +inf closes everything.

The static tables are channel-major over the whole run, an order a stream cannot deliver.  The stream's merged rows are
ordered by (board, channel), then chain order, within one push; `component_offset` counts through the stream's own
component sequence, and `hit_index` is a row's position among all rows pushed, which is its index in the static
hit_threshold table because the hit stream's chunks concatenate to it.  `static_tables` puts all of it into the static
order: the result equals hit_merged, hit_merge_clusters and hit_merged_components byte for byte, whatever the chunk size.

The device part is wfa_merge_stream_* (DeviceSession.merge_stream_begin / _push / _end).

The events of these rows come from hit_merged_grouped_stream (merged_event_stream.py): one push there is this stream's
merge step followed by the grouping step on the same session, the merged rows handed over in HBM, under the grouping
horizon min(H, open_start) -- `open_start` (the smallest abs_start still carried) is what this stream reports with every
chunk.  hit_grouped_stream itself keeps refusing merge_gap_ns > 0.  Not built: a device-to-device hand-over of the hit
rows, several merging devices.
"""

from __future__ import annotations

import numpy as np

from .chunk import Chunk
from .dtypes import HIT_MERGE_CLUSTERS_DTYPE, HIT_MERGED_COMPONENTS_DTYPE, HIT_MERGED_DTYPE
from .event_stream import HitPushStream
from .plugins.hit_merge import MERGE_OPTIONS
from .streaming import HipThresholdHitStream


def static_tables(merged_rows: np.ndarray, hit_index: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """All merged rows and member indices a stream delivered, concatenated in delivery order -> the static
    (hit_merged, hit_merge_clusters, hit_merged_components): the merged rows stably sorted by (board, channel),
    component_offset rewritten as the exclusive running sum of component_count, the members moved with their clusters."""
    merged_rows = np.asarray(merged_rows)
    hit_index = np.asarray(hit_index, dtype=np.int64)
    counts = merged_rows["component_count"].astype(np.int64)
    if int(counts.sum()) != len(hit_index):
        raise ValueError(f"{len(hit_index)} component rows for clusters of {int(counts.sum())} members")
    order = np.lexsort((merged_rows["channel"], merged_rows["board"]))   # (stable: delivery order inside a channel)
    merged = merged_rows[order].copy()
    counts = counts[order]
    ends = np.cumsum(counts)
    merged["component_offset"] = ends - counts
    # member k of output cluster j sits at (start of cluster order[j] in the delivered sequence) + k
    delivered_start = np.cumsum(merged_rows["component_count"].astype(np.int64)) - merged_rows["component_count"]
    cluster_of = np.repeat(np.arange(len(merged), dtype=np.int64), counts)
    within = np.arange(len(hit_index), dtype=np.int64) - np.repeat(ends - counts, counts)
    members = hit_index[np.repeat(delivered_start[order], counts) + within]
    clusters = np.zeros(len(members), dtype=HIT_MERGE_CLUSTERS_DTYPE)
    clusters["cluster_index"], clusters["hit_index"] = cluster_of, members
    components = np.zeros(len(members), dtype=HIT_MERGED_COMPONENTS_DTYPE)
    components["merged_index"], components["hit_index"] = cluster_of, members
    return merged, clusters, components


def merged_bounds(rows: np.ndarray) -> tuple[int, int]:
    """[start, end) of a result chunk: the smallest anchor timestamp and the largest + 1.  (A merged row stores its
    anchor hit, not its extent, and a cluster that spans records has no sample window to derive one from.)"""
    ts = rows["timestamp"]
    return int(ts.min()), int(ts.max()) + 1


class HipHitMergedStream(HitPushStream):
    """compute() = the merged hits of the records stream, delivered as their clusters close (HitPushStream with
    wfa_merge_stream_*).

    A result chunk holds the HIT_MERGED_DTYPE rows of the clusters one push closed; a push that closes nothing yields
    nothing.  Its metadata carries `hit_index` (int64, the members of the chunk's clusters, in the rows' order),
    `first_component` (= component_offset of its first row), `n_carry` (hits still on the device) and `open_start`
    (their smallest abs_start in ps, +inf if none).  Bounds: [min timestamp, max timestamp + 1) of the rows' anchors
    (`merged_bounds`); like the event stream's chunks they follow the data and may overlap between chunks.
    `static_tables(all rows, all hit_index)` gives what HipHitMergePlugin, HipHitMergeClustersPlugin and
    HipHitMergedComponentsPlugin give on HipThresholdHitPlugin's rows under the same configuration.

    Options: those of hit_threshold_stream, and `merge_gap_ns` / `max_total_width_ns` / `dt` with hit_merged's names and
    defaults.  The stream's rows always carry dt (the records'), so `dt` is read for parity only.

    Refused on the host, before any upload: a negative gap or width, and a device pool with fewer than three sessions
    (two for the ring, one for the merge)."""

    provides = "hit_merged_stream"
    description = "Merged threshold hits of the records stream, delivered as their clusters close (HIP, gfx950)."
    output_dtype = HIT_MERGED_DTYPE
    output_data_kind = "hits"
    output_time_field = "timestamp"
    output_endtime_field = "timestamp"
    role = "merge"

    options = {**HipThresholdHitStream.options, **MERGE_OPTIONS}

    def _check_cfg(self, cfg: dict) -> None:
        for name in ("merge_gap_ns", "max_total_width_ns"):
            cfg[name] = float(cfg[name])
            if not cfg[name] >= 0:
                raise ValueError(f"{name} must be >= 0")

    counters = ("components",)

    def _begin(self, sess, cfg: dict) -> None:
        sess.merge_stream_begin(cfg["merge_gap_ns"], cfg["max_total_width_ns"])

    def _end(self, sess) -> None:
        sess.merge_stream_end()

    def _push(self, sess, rows, horizon: float, run_id: str, stats: dict):
        out, hit_index, n_carry, open_start = sess.merge_stream_push(rows, horizon)
        self._count_push(stats, rows, len(out), n_carry)
        stats["components"] += len(hit_index)
        if len(out) == 0:
            return None
        start, end = merged_bounds(out)
        result = Chunk(out, start, end, run_id, self.provides, data_kind=self.output_data_kind, time_field="timestamp",
                       endtime_field="timestamp",
                       metadata={"hit_index": hit_index, "first_component": int(out["component_offset"][0]),
                                 "n_carry": int(n_carry), "open_start": float(open_start)})
        self._validate_chunk(result)
        return result


__all__ = ["HipHitMergedStream", "static_tables", "merged_bounds", "HIT_MERGED_DTYPE"]
