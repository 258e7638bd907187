"""Wall time of the merged-event stream against what a user must do today for the events of merged hits: host chunks in,
host event rows out.

Data: the run of tools/merge_stream_time.py -- a synthetic V1725 run (synth.make_run, uniform L = 800) cut into
bench-sized chunks (`--chunk-records`, default 50 000 = 4e7 samples per chunk), SG(11, 2) and one threshold for every
record, hit ring of two sessions on device 0 -- merged with `--gap-ns` (default 20) and hit_merged's default width cap,
grouped with `--window-ns` (default 100).  Two ways:

  static    HipThresholdHitStream.run_chunks, the chunks' rows concatenated on the host, then the static hit_merged chain
            (compute_cluster_rows, compute_merged_rows, compute_component_rows) and the static hit_grouped on it
            (group_hit_windows_flat with the components: fix windows on the host, columns up, order and event tables
            back), the event rows gathered through `order` on the host;
  stream    HipHitMergedGroupedStream.run_chunks: every chunk's rows pushed to the one merge-and-grouping session as they
            arrive, the delivered rows concatenated.

After `--warmup` rounds the two ways alternate for `--repeats` rounds; per way the median, the fastest and the slowest
round and the time from the start of a round to its first event rows (static: the end of the grouping pass).  The stream
also reports its largest carry, the bytes of hit rows it uploads again (60 B per row), its output bytes and, from one
more round with the kernel timers of the push session on (`profile_pushes`), the device time of a push.  The rows of the
two ways must be equal in every field but component_offset (the stream's offsets count through its own component
sequence), and the members those offsets address must be the same hits.

    python tools/merged_event_stream_time.py [--records 400000] [--chunk-records 50000] [--gap-ns 20] [--window-ns 100]
                                             [--warmup 2] [--repeats 7]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from waveformanalysis_amd import synth  # noqa: E402
from waveformanalysis_amd.device import DevicePool  # noqa: E402
from waveformanalysis_amd.dtypes import EVENT_MERGED_HIT_DTYPE, HIT_MERGED_DTYPE  # noqa: E402
from waveformanalysis_amd.event_grouping import group_hit_windows_flat  # noqa: E402
from waveformanalysis_amd.hit_merge import compute_cluster_rows, compute_component_rows, compute_merged_rows  # noqa: E402
from waveformanalysis_amd.merged_event_stream import HipHitMergedGroupedStream  # noqa: E402
from waveformanalysis_amd.plugin_api import SimpleContext  # noqa: E402
from waveformanalysis_amd.streaming import HipThresholdHitStream, records_to_chunks  # noqa: E402


def merged_event_rows(merged: np.ndarray, flat: dict) -> np.ndarray:
    """EVENT_MERGED_HIT_DTYPE rows from the flat form of the static pass over a hit_merged table."""
    order, es = np.asarray(flat["order"], dtype=np.int64), np.asarray(flat["event_start"], dtype=np.int64)
    counts = np.diff(es)
    out = np.zeros(len(order), dtype=EVENT_MERGED_HIT_DTYPE)
    out["event_id"] = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    out["t_min"] = np.repeat(np.asarray(flat["t_min"], dtype=np.int64), counts)
    out["t_max"] = np.repeat(np.asarray(flat["t_max"], dtype=np.int64), counts)
    picked = merged[order]
    for name in HIT_MERGED_DTYPE.names:
        out[name] = picked[name]
    return out


def members_of(rows: np.ndarray, hit_index: np.ndarray) -> np.ndarray:
    """The member hits of every row, concatenated in row order."""
    counts = rows["component_count"].astype(np.int64)
    start = np.cumsum(counts) - counts
    return hit_index[np.repeat(rows["component_offset"] - start, counts) + np.arange(int(counts.sum()))]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=400_000)
    ap.add_argument("--chunk-records", type=int, default=50_000)
    ap.add_argument("--gap-ns", type=float, default=20.0)
    ap.add_argument("--window-ns", type=float, default=100.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    rec, pool = synth.make_run(args.records, "v1725", cfg=5)
    L = int(rec["event_length"][0])
    rec["board"], rec["channel"] = 0, np.arange(len(rec)) % 3
    rec["baseline"] = pool.reshape(len(rec), L)[:, : synth.BASELINE_SAMPLES].mean(axis=1)
    chunks = records_to_chunks(rec, args.chunk_records, "run")
    ctx = SimpleContext({"use_filtered": True, "merge_gap_ns": args.gap_ns, "time_window_ns": args.window_ns},
                        {"records": rec, "wave_pool": pool})
    dp = DevicePool([0])
    hit_stream = HipThresholdHitStream(device_pool=dp)
    event_stream = HipHitMergedGroupedStream(device_pool=dp)
    width_ns = event_stream.cfg["max_total_width_ns"]

    def static_way():
        t0 = time.perf_counter()
        outs = hit_stream.run_chunks(chunks, ctx, "run", max_workers=2)
        hits = np.concatenate([o.data for o in outs])
        with dp.borrow() as sess:
            clusters = compute_cluster_rows(sess, hits, args.gap_ns, width_ns, None, "hit_merge_clusters")
            merged = compute_merged_rows(sess, hits, clusters, None, "hit_merged")
            t_merged = time.perf_counter() - t0
            components = compute_component_rows(merged, clusters)
            t_components = time.perf_counter() - t0
            flat = group_hit_windows_flat(merged, args.window_ns, component_rows=components, component_hits=hits, session=sess)
        first = time.perf_counter() - t0
        rows = merged_event_rows(merged, flat)
        index = np.asarray(components["hit_index"], dtype=np.int64)
        return (rows, index), time.perf_counter() - t0, first, (t_merged, t_components)

    def stream_way():
        t0 = time.perf_counter()
        first: list = []
        outs = list(event_stream.run_chunks(chunks, ctx, "run", max_workers=2, first_event_time=first))
        rows = np.concatenate([o.data for o in outs])
        index = np.concatenate([o.metadata["hit_index"] for o in outs])
        return (rows, index), time.perf_counter() - t0, (first[0] - t0 if first else float("nan")), None

    ways = {"static": static_way, "stream": stream_way}
    times = {name: [] for name in ways}
    firsts = {name: [] for name in ways}
    static_parts = []
    tables = {}
    for rnd in range(args.warmup + args.repeats):
        for name, way in ways.items():
            out, total, first, parts = way()
            if rnd >= args.warmup:
                times[name].append(total)
                firsts[name].append(first)
                if parts:
                    static_parts.append(parts)
            tables[name] = out
    (a_rows, a_index), (b_rows, b_index) = tables["static"], tables["stream"]
    assert len(a_rows) == len(b_rows), "the two ways give different tables"
    for name in EVENT_MERGED_HIT_DTYPE.names:
        assert name == "component_offset" or np.array_equal(a_rows[name], b_rows[name]), f"the two ways differ in {name}"
    assert np.array_equal(members_of(a_rows, a_index), members_of(b_rows, b_index)), "the two ways address different members"
    stats = dict(event_stream.stats)
    event_stream.profile_pushes = True
    stream_way()
    profile = event_stream.stats.get("profile", {})
    dp.close()
    for name, ts in times.items():
        print(json.dumps({"way": name, "chunks": len(chunks), "samples": int(pool.size), "hit_rows": int(len(a_index)),
                          "merged_rows": int(len(a_rows)), "events": int(a_rows["event_id"][-1]) + 1 if len(a_rows) else 0,
                          "gap_ns": args.gap_ns, "window_ns": args.window_ns,
                          "median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5),
                          "max_s": round(max(ts), 5), "first_event_s_median": round(statistics.median(firsts[name]), 5),
                          "rounds": len(ts)}))
    print(json.dumps({"static_merged_rows_after_s_median": round(statistics.median(p[0] for p in static_parts), 5),
                      "static_components_after_s_median": round(statistics.median(p[1] for p in static_parts), 5)}))
    push_ms = sum(ms for ms, _n in profile.values())
    print(json.dumps({"stream_pushes": stats["pushes"], "max_carry_rows": stats["max_carry"],
                      "row_reupload_bytes": 60 * stats["rows_in"],
                      "output_bytes": 96 * stats["rows_out"] + 8 * stats["components"],
                      "push_device_ms_total": round(push_ms, 3),
                      "push_device_ms_per_push": round(push_ms / max(stats["pushes"], 1), 3),
                      "push_profile_ms": {k: round(ms, 3) for k, (ms, _n) in profile.items()}}))
    print(json.dumps({"stream_over_static": round(statistics.median(times["stream"]) / statistics.median(times["static"]), 4)}))


if __name__ == "__main__":
    main()
