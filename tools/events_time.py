"""Wall time of the df, df_events and df_paired plugins on a synthetic run, and of the device grouping pass alone.

    python tools/events_time.py [--rows 1250000] [--grouping-log2 20,25] [--repeat 5] [--skip-plugins]

The run: `rows` rows over 16 channels on one board, about one row per microsecond (exponential gaps), float32
area / height; df_events with the default 100 ns window.  The grouping lines time DeviceSession.group_multi_channel
(upload, sorts, window chain, download of order / bounds) on 2^k rows of the same kind, best of `repeat` after one
warm-up, the device time of the pass (HIP events around it, from after the uploads to the end of the second sort),
and the device scratch the pass held (the bytes release_scratch() gives back afterwards).
One JSON line per measurement.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_run(rows: int, seed: int = 7):
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.exponential(1e6, rows)).astype(np.int64) + 1_000_000  # ps
    table = np.zeros(rows, dtype=[("timestamp", "i8"), ("board", "i2"), ("channel", "i2"), ("record_id", "i8")])
    table["timestamp"] = ts
    table["channel"] = rng.integers(0, 16, rows)
    table["record_id"] = np.arange(rows)
    bf = np.zeros(rows, dtype=[("height", "f4"), ("amp", "f4"), ("area", "f4"), ("max_abs_diff", "f4")])
    bf["height"] = rng.uniform(5, 400, rows)
    bf["amp"] = bf["height"]
    bf["area"] = rng.uniform(0, 4000, rows)
    bf["max_abs_diff"] = rng.uniform(0, 90, rows)
    return table, bf


def time_plugins(rows: int) -> None:
    from waveformanalysis_amd.plugin_api import SimpleContext
    from waveformanalysis_amd.plugins import HipDataFramePlugin, HipGroupedEventsPlugin, HipPairedEventsPlugin

    table, bf = synthetic_run(rows)
    ctx = SimpleContext({}, {"st_waveforms": table, "basic_features": bf},
                        [HipDataFramePlugin(), HipGroupedEventsPlugin(), HipPairedEventsPlugin()])
    warm = SimpleContext({}, {"st_waveforms": table[:4096], "basic_features": bf[:4096]},
                         [HipDataFramePlugin(), HipGroupedEventsPlugin(), HipPairedEventsPlugin()])
    warm.get_data("warm", "df_paired")  # library load, device context, first launches
    for name in ("df", "df_events", "df_paired"):
        t0 = time.perf_counter()
        out = ctx.get_data("run", name)
        ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"stage": name, "rows": rows, "out_rows": len(out), "ms": round(ms, 1)}), flush=True)


def time_grouping(log2s, repeat: int) -> None:
    from waveformanalysis_amd.device import DeviceSession

    for k in log2s:
        n = 1 << k
        table, _ = synthetic_run(n, seed=k)
        ts, ch = table["timestamp"], table["channel"].astype(np.int64)
        with DeviceSession(0) as sess:
            sess.group_multi_channel(ts[:4096], ch[:4096], 1e5)
            best = float("inf")
            for _ in range(repeat + 1):
                t0 = time.perf_counter()
                _, bounds = sess.group_multi_channel(ts, ch, 1e5)
                best = min(best, time.perf_counter() - t0)
            sess.profile(True)  # device time of the count pass: after the uploads, sorts and window chain included
            sess.group_multi_channel(ts, ch, 1e5)
            device_ms = sum(ms for name, (ms, _) in sess.profile_report().items() if "group_multi_channel" in name)
            sess.profile(False)
            held = sess.release_scratch()
        print(json.dumps({"stage": "group_multi_channel", "rows": n, "events": len(bounds) - 1,
                          "ms": round(best * 1e3, 2), "device_pass_ms": round(device_ms, 2), "scratch_bytes": held,
                          "scratch_bytes_per_row": round(held / n, 1)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_250_000)
    ap.add_argument("--grouping-log2", default="20,25")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--skip-plugins", action="store_true")
    args = ap.parse_args()
    if not args.skip_plugins:
        time_plugins(args.rows)
    if args.grouping_log2:
        time_grouping([int(v) for v in args.grouping_log2.split(",")], args.repeat)


if __name__ == "__main__":
    main()
