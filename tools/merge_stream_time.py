"""Wall time of the merge stream against the static way to the same merged hits: host chunks in, host tables out.

Data: the run of tools/event_stream_time.py -- a synthetic V1725 run (synth.make_run, uniform L = 800) cut into
bench-sized chunks (`--chunk-records`, default 50 000 = 4e7 samples per chunk), SG(11, 2) and one threshold for every
record, hit ring of two sessions on device 0 -- merged with `--gap-ns` (default 20) and hit_merged's default width cap.
Two ways:

  static    HipThresholdHitStream.run_chunks, the chunks' rows concatenated on the host, then what the three static
            plugins do: compute_cluster_rows (one upload of the table's columns, sort + chain, index tables back),
            compute_merged_rows (columns up again, per-cluster reductions back) and compute_component_rows;
  stream    HipHitMergedStream.run_chunks: every chunk's rows pushed to the merge session as they arrive; the time
            includes `static_tables` over everything delivered, so both ways end with the same three tables.

After `--warmup` rounds the two ways alternate for `--repeats` rounds; per way the median, the fastest and the slowest
round and the time from the start of a round to its first merged rows (static: the end of compute_merged_rows).  The
stream also reports its largest carry, the bytes of hit rows it uploads again (60 B per row), and, from one more round
with the kernel timers of the merge session on, the device time of a push.  The tables of the two ways must be equal,
byte for byte.

    python tools/merge_stream_time.py [--records 400000] [--chunk-records 50000] [--gap-ns 20] [--warmup 2] [--repeats 7]
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
from waveformanalysis_amd.hit_merge import compute_cluster_rows, compute_component_rows, compute_merged_rows  # noqa: E402
from waveformanalysis_amd.merge_stream import HipHitMergedStream, static_tables  # noqa: E402
from waveformanalysis_amd.plugin_api import SimpleContext  # noqa: E402
from waveformanalysis_amd.streaming import HipThresholdHitStream, records_to_chunks  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=400_000)
    ap.add_argument("--chunk-records", type=int, default=50_000)
    ap.add_argument("--gap-ns", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    rec, pool = synth.make_run(args.records, "v1725", cfg=5)
    L = int(rec["event_length"][0])
    rec["board"], rec["channel"] = 0, np.arange(len(rec)) % 3
    rec["baseline"] = pool.reshape(len(rec), L)[:, : synth.BASELINE_SAMPLES].mean(axis=1)
    chunks = records_to_chunks(rec, args.chunk_records, "run")
    ctx = SimpleContext({"use_filtered": True, "merge_gap_ns": args.gap_ns}, {"records": rec, "wave_pool": pool})
    dp = DevicePool([0])
    hit_stream = HipThresholdHitStream(device_pool=dp)
    merge_stream = HipHitMergedStream(device_pool=dp)
    width_ns = merge_stream.cfg["max_total_width_ns"]

    def static_way():
        t0 = time.perf_counter()
        outs = hit_stream.run_chunks(chunks, ctx, "run", max_workers=2)
        hits = np.concatenate([o.data for o in outs])
        with dp.borrow() as sess:
            clusters = compute_cluster_rows(sess, hits, args.gap_ns, width_ns, None, "hit_merge_clusters")
            merged = compute_merged_rows(sess, hits, clusters, None, "hit_merged")
        first = time.perf_counter() - t0
        components = compute_component_rows(merged, clusters)
        return (merged, clusters, components), time.perf_counter() - t0, first

    def stream_way():
        t0 = time.perf_counter()
        first: list = []
        outs = list(merge_stream.run_chunks(chunks, ctx, "run", max_workers=2, first_event_time=first))
        tables = static_tables(np.concatenate([o.data for o in outs]), np.concatenate([o.metadata["hit_index"] for o in outs]))
        return tables, time.perf_counter() - t0, (first[0] - t0 if first else float("nan"))

    ways = {"static": static_way, "stream": stream_way}
    times = {name: [] for name in ways}
    firsts = {name: [] for name in ways}
    tables = {}
    for rnd in range(args.warmup + args.repeats):
        for name, way in ways.items():
            out, total, first = way()
            if rnd >= args.warmup:
                times[name].append(total)
                firsts[name].append(first)
            tables[name] = out
    for a, b in zip(tables["static"], tables["stream"]):
        assert a.tobytes() == b.tobytes(), "the two ways give different tables"
    stats = dict(merge_stream.stats)
    merge_stream.profile_pushes = True
    stream_way()
    profile = merge_stream.stats.get("profile", {})
    dp.close()
    merged, clusters, _components = tables["stream"]
    for name, ts in times.items():
        print(json.dumps({"way": name, "chunks": len(chunks), "samples": int(pool.size), "hit_rows": int(len(clusters)),
                          "merged_rows": int(len(merged)), "gap_ns": args.gap_ns,
                          "median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5),
                          "max_s": round(max(ts), 5), "first_merged_s_median": round(statistics.median(firsts[name]), 5),
                          "rounds": len(ts)}))
    push_ms = sum(ms for ms, _n in profile.values())
    print(json.dumps({"stream_pushes": stats["pushes"], "max_carry_rows": stats["max_carry"],
                      "row_reupload_bytes": 60 * stats["rows_in"],
                      "output_bytes": 72 * stats["rows_out"] + 8 * stats["components"],
                      "push_device_ms_total": round(push_ms, 3),
                      "push_device_ms_per_push": round(push_ms / max(stats["pushes"], 1), 3),
                      "push_profile_ms": {k: round(ms, 3) for k, (ms, _n) in profile.items()}}))
    print(json.dumps({"stream_over_static": round(statistics.median(times["stream"]) / statistics.median(times["static"]), 4)}))


if __name__ == "__main__":
    main()
