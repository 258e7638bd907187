"""Wall time of the event stream against the static way to the same events: host chunks in, host event rows out.

Data: the run of tools/stream_groups_time.py's one-group case -- a synthetic V1725 run (synth.make_run, uniform L = 800)
cut into bench-sized chunks (`--chunk-records`, default 50 000 = 4e7 samples per chunk), SG(11, 2) and one threshold for
every record, hit ring of two sessions on device 0 -- grouped with a window of `--window-ns` (default 100).  Two ways:

  static    HipThresholdHitStream.run_chunks, the chunks' rows concatenated on the host, group_hit_windows_flat over the
            whole table (one upload of its columns, one grouping pass), EVENT_HIT_DTYPE rows built on the host;
  stream    HipHitGroupedStream.run_chunks: every chunk's rows pushed to the grouping session as they arrive.

After `--warmup` rounds the two ways alternate for `--repeats` rounds; per way the median, the fastest and the slowest
round and the time from the start of a round to its first delivered event rows (static: the end of the grouping).  The
stream also reports its largest carry, the bytes of hit rows it uploads again (60 B per row), and, from one more round
with the kernel timers of the grouping session on, the device time of a push.  The rows of the two ways must be equal,
byte for byte.

    python tools/event_stream_time.py [--records 400000] [--chunk-records 50000] [--window-ns 100] [--warmup 2] [--repeats 7]
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
from waveformanalysis_amd.event_grouping import group_hit_windows_flat  # noqa: E402
from waveformanalysis_amd.event_stream import HipHitGroupedStream, event_rows  # noqa: E402
from waveformanalysis_amd.plugin_api import SimpleContext  # noqa: E402
from waveformanalysis_amd.streaming import HipThresholdHitStream, records_to_chunks  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=400_000)
    ap.add_argument("--chunk-records", type=int, default=50_000)
    ap.add_argument("--window-ns", type=float, default=100.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    rec, pool = synth.make_run(args.records, "v1725", cfg=5)
    L = int(rec["event_length"][0])
    rec["board"], rec["channel"] = 0, np.arange(len(rec)) % 3
    rec["baseline"] = pool.reshape(len(rec), L)[:, : synth.BASELINE_SAMPLES].mean(axis=1)
    chunks = records_to_chunks(rec, args.chunk_records, "run")
    ctx = SimpleContext({"use_filtered": True, "time_window_ns": args.window_ns}, {"records": rec, "wave_pool": pool})
    dp = DevicePool([0])
    hit_stream = HipThresholdHitStream(device_pool=dp)
    event_stream = HipHitGroupedStream(device_pool=dp)

    def static_way():
        t0 = time.perf_counter()
        outs = hit_stream.run_chunks(chunks, ctx, "run", max_workers=2)
        hits = np.concatenate([o.data for o in outs])
        with dp.borrow() as sess:
            flat = group_hit_windows_flat(hits, args.window_ns, session=sess)
        first = time.perf_counter() - t0
        rows = event_rows(hits, flat)
        return rows, time.perf_counter() - t0, first

    def stream_way():
        t0 = time.perf_counter()
        first: list = []
        outs = list(event_stream.run_chunks(chunks, ctx, "run", max_workers=2, first_event_time=first))
        rows = np.concatenate([o.data for o in outs])
        return rows, time.perf_counter() - t0, (first[0] - t0 if first else float("nan"))

    ways = {"static": static_way, "stream": stream_way}
    times = {name: [] for name in ways}
    firsts = {name: [] for name in ways}
    tables = {}
    for rnd in range(args.warmup + args.repeats):
        for name, way in ways.items():
            rows, total, first = way()
            if rnd >= args.warmup:
                times[name].append(total)
                firsts[name].append(first)
            tables[name] = rows
    assert tables["static"].tobytes() == tables["stream"].tobytes(), "the two ways give different rows"
    stats = dict(event_stream.stats)
    event_stream.profile_pushes = True
    stream_way()
    profile = event_stream.stats.get("profile", {})
    dp.close()
    rows = tables["stream"]
    for name, ts in times.items():
        print(json.dumps({"way": name, "chunks": len(chunks), "samples": int(pool.size), "hit_rows": int(len(rows)),
                          "events": int(rows["event_id"][-1]) + 1 if len(rows) else 0, "window_ns": args.window_ns,
                          "median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5),
                          "max_s": round(max(ts), 5), "first_event_s_median": round(statistics.median(firsts[name]), 5),
                          "rounds": len(ts)}))
    push_ms = sum(ms for ms, _n in profile.values())
    print(json.dumps({"stream_pushes": stats["pushes"], "max_carry_rows": stats["max_carry"],
                      "row_reupload_bytes": 60 * stats["rows_in"], "event_rows_bytes": 84 * stats["rows_out"],
                      "push_device_ms_total": round(push_ms, 3),
                      "push_device_ms_per_push": round(push_ms / max(stats["pushes"], 1), 3),
                      "push_profile_ms": {k: round(ms, 3) for k, (ms, _n) in profile.items()}}))
    print(json.dumps({"stream_over_static": round(statistics.median(times["stream"]) / statistics.median(times["static"]), 4)}))


if __name__ == "__main__":
    main()
