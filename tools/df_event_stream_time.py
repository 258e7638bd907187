"""Wall time of the df_events stream against the static way to the same events: host chunks in, host events out.

Data: a synthetic V1725 run (synth.make_run: 16 channels, uniform L = 800) cut into bench-sized chunks
(`--chunk-records`, default 50 000 = 4e7 samples per chunk), grouped with a window of `--window-ns` (default 100).  Ways:

  static           the static chain on one session: the whole pool and records uploaded, basic_features, the df columns
                   sorted by timestamp (HipDataFramePlugin's frame), group_multi_channel_order on the device and
                   build_events_frame on the host (what HipGroupedEventsPlugin returns);
  stream_serial    HipGroupedEventsStream.run_chunks with one features session: chunk after chunk, every chunk's df rows
                   pushed to the grouping session;
  stream_parallel  the same with `--workers` feature workers (thread per session).

The stream delivers DF_EVENT_ROW_DTYPE rows; `frame_s` is the host time grouped_events_frame then takes to build the
static way's frame from all of them (not part of the stream's time).  After `--warmup` rounds the ways alternate for
`--repeats` rounds; per way the median, the fastest and the slowest round and the time from the start of a round to its
first delivered events (static: the end of the round).  The stream also reports its rows, events and largest carry and,
from one more round with the kernel timers of the grouping session on, the device time of a push.  The frames of the
ways must be equal.

    python tools/df_event_stream_time.py [--records 400000] [--chunk-records 50000] [--window-ns 100] [--workers 4]
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
import pandas as pd  # noqa: E402

from waveformanalysis_amd import _lib, synth  # noqa: E402
from waveformanalysis_amd.device import DevicePool  # noqa: E402
from waveformanalysis_amd.df_event_stream import HipGroupedEventsStream, grouped_events_frame  # noqa: E402
from waveformanalysis_amd.event_grouping import group_multi_channel_order  # noqa: E402
from waveformanalysis_amd.plugin_api import SimpleContext  # noqa: E402
from waveformanalysis_amd.plugins.basic_features import PEAK_RANGE  # noqa: E402
from waveformanalysis_amd.plugins.event_analysis import build_events_frame  # noqa: E402
from waveformanalysis_amd.streaming import records_to_chunks  # noqa: E402


def frames_equal(a: pd.DataFrame, b: pd.DataFrame) -> bool:
    if list(a.columns) != list(b.columns) or len(a) != len(b):
        return False
    for column in a.columns:
        if a[column].dtype != object:
            if not np.array_equal(a[column].to_numpy(), b[column].to_numpy()):
                return False
            continue
        if len(a) and not np.array_equal(np.concatenate(a[column].to_list()), np.concatenate(b[column].to_list()),
                                         equal_nan=True):
            return False
    return True


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=400_000)
    ap.add_argument("--chunk-records", type=int, default=50_000)
    ap.add_argument("--window-ns", type=float, default=100.0)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    rec, pool = synth.make_run(args.records, "v1725", cfg=5)
    chunks = records_to_chunks(rec, args.chunk_records, "run")
    ctx = SimpleContext({}, {"records": rec, "wave_pool": pool})
    dp = DevicePool([0])
    stream = HipGroupedEventsStream(device_pool=dp, time_window_ns=args.window_ns)

    def static_way():
        t0 = time.perf_counter()
        with dp.borrow() as sess:
            sess.upload_pool(pool)
            sess.upload_records(rec)
            bf = sess.basic_features(_lib.SRC_RAW, PEAK_RANGE, (0, None))
            df = pd.DataFrame({"timestamp": rec["timestamp"], "record_id": rec["record_id"], "area": bf["area"],
                               "height": bf["height"], "amp": bf["amp"], "max_abs_diff": bf["max_abs_diff"],
                               "board": rec["board"], "channel": rec["channel"]}).sort_values("timestamp", kind="stable")
            grouped = group_multi_channel_order(df, args.window_ns, session=sess)
        frame, _flat = build_events_frame(*grouped)
        total = time.perf_counter() - t0
        return frame, total, total

    def stream_way(workers):
        def way():
            t0 = time.perf_counter()
            first: list = []
            outs = list(stream.run_chunks(chunks, ctx, "run", max_workers=workers, first_event_time=first))
            rows = np.concatenate([o.data for o in outs])
            return rows, time.perf_counter() - t0, (first[0] - t0 if first else float("nan"))
        return way

    ways = {"static": static_way, "stream_serial": stream_way(1), "stream_parallel": stream_way(args.workers)}
    times = {name: [] for name in ways}
    firsts = {name: [] for name in ways}
    products, stats = {}, {}
    for rnd in range(args.warmup + args.repeats):
        for name, way in ways.items():
            product, total, first = way()
            if rnd >= args.warmup:
                times[name].append(total)
                firsts[name].append(first)
            products[name] = product
            if name != "static":
                stats[name] = dict(stream.stats)
    t0 = time.perf_counter()
    frame = grouped_events_frame(products["stream_parallel"])
    frame_s = time.perf_counter() - t0
    assert products["stream_serial"].tobytes() == products["stream_parallel"].tobytes(), "serial and parallel rows differ"
    assert frames_equal(frame, products["static"]), "the stream's frame differs from the static one"
    stream.profile_pushes = True
    stream_way(args.workers)()
    profile = stream.stats.get("profile", {})
    dp.close()
    rows = products["stream_parallel"]
    for name, ts in times.items():
        print(json.dumps({"way": name, "chunks": len(chunks), "samples": int(pool.size), "rows": int(len(rows)),
                          "events": int(rows["event_id"][-1]) + 1 if len(rows) else 0, "window_ns": args.window_ns,
                          "median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5),
                          "max_s": round(max(ts), 5), "first_event_s_median": round(statistics.median(firsts[name]), 5),
                          "rounds": len(ts)}))
    st = stats["stream_parallel"]
    push_ms = sum(ms for ms, _n in profile.values())
    print(json.dumps({"stream_pushes": st["pushes"], "max_carry_rows": max(s["max_carry"] for s in stats.values()),
                      "row_upload_bytes": 40 * st["rows_in"], "event_rows_bytes": 64 * st["rows_out"],
                      "frame_s": round(frame_s, 5), "workers": args.workers,
                      "push_device_ms_total": round(push_ms, 3),
                      "push_device_ms_per_push": round(push_ms / max(st["pushes"], 1), 3),
                      "push_profile_ms": {k: round(ms, 3) for k, (ms, _n) in profile.items()}}))
    static = statistics.median(times["static"])
    print(json.dumps({name + "_over_static": round(statistics.median(times[name]) / static, 4)
                      for name in ("stream_serial", "stream_parallel")}))


if __name__ == "__main__":
    main()
