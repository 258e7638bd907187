"""Wall time of the S1/S2 stream under per-channel settings: host arrays in, host s1_s2 rows out, three ways.

Data: the run of tools/s1s2_stream_time.py (replay.mirror_positive(*synth.make_run(records, "v1725", cfg=17)), uniform
L = 800, channels 0-15 of board 0) with its hit options and class ranges.  Per-channel configuration: three
Savitzky-Golay groups -- channels 0:1 and 0:5 SG(7, 3), 0:2 SG(9, 2), every other channel the run-wide SG(11, 2) -- and one
fixed-baseline channel (0:4, 8000.0).

  grouped  HipS1S2Stream with filter_source="wave_pool_filtered" and baseline_source="basic_features": per chunk one
           savgol_group call per group over the uploaded table, then find_peaks and peak_chain(fixed_baseline);
  single   HipS1S2Stream with both options at their defaults on the same records (one SG(11, 2) for the run, no fixed
           baseline): the calls of the stream before the options existed.  Another configuration, so another table;
  static   the plugin chain wave_pool_filtered -> hit -> waveform_width -> s1_s2 with basic_features on the side
           (hip_default(), wave_source="records") under the per-channel configuration, a new Context per round.

After `--warmup` rounds (every way once per round) the three ways alternate for `--repeats` rounds in one process; per
way the median, the fastest and the slowest round.  One JSON line per way, one with the ratios and whether the grouped
stream's table equals the static chain's byte for byte, then the device profile of one chunk of the grouped stream.

    python tools/s1s2_stream_settings_time.py [--records 100000] [--chunk-records 25000] [--workers 2] [--warmup 2]
                                              [--repeats 7]
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

from waveformanalysis_amd import replay, synth  # noqa: E402
from waveformanalysis_amd.device import DevicePool, default_pool  # noqa: E402
from waveformanalysis_amd.plugin_api import SimpleContext  # noqa: E402
from waveformanalysis_amd.plugins import hip_default  # noqa: E402
from waveformanalysis_amd.s1s2_stream import HipS1S2Stream  # noqa: E402

CONFIG = {"wave_source": "records", "height": 8.0, "prominence": 0.5, "width": 2, "distance": 2,
          "s1_width_range": (0.0, 80.0), "s2_width_range": (80.0, 5000.0), "s1_area_range": None,
          "s2_area_range": (500.0, 1e12)}
FILTER_CC = {"0:1": {"sg_window_size": 7, "sg_poly_order": 3}, "0:5": {"sg_window_size": 7, "sg_poly_order": 3},
             "0:2": {"sg_window_size": 9, "sg_poly_order": 2}}
BASELINE_CC = {"0:4": {"fixed_baseline": 8000.0}}
PER_CHANNEL = {**CONFIG, "wave_pool_filtered": {"channel_config": FILTER_CC},
               "basic_features": {"channel_config": BASELINE_CC}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000)
    ap.add_argument("--chunk-records", type=int, default=25_000)
    ap.add_argument("--workers", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    rec, pool = replay.mirror_positive(*synth.make_run(args.records, "v1725", cfg=17))
    data = {"records": rec, "wave_pool": pool}
    dp = DevicePool([0])
    grouped_stream = HipS1S2Stream(device_pool=dp, filter_source="wave_pool_filtered", baseline_source="basic_features")
    single_stream = HipS1S2Stream(device_pool=dp)
    streaming_config = {"chunk_size": args.chunk_records, "max_workers": args.workers, "parallel": args.workers > 1}

    def grouped():
        outs = grouped_stream.compute(SimpleContext(PER_CHANNEL, data), "run", streaming_config=streaming_config)
        return np.concatenate([o.data for o in outs])

    def single():
        outs = single_stream.compute(SimpleContext(CONFIG, data), "run", streaming_config=streaming_config)
        return np.concatenate([o.data for o in outs])

    def static():
        default_pool().session().forget_resident()  # a new run: its pool goes up again
        ctx = SimpleContext(PER_CHANNEL, data, plugins=hip_default())
        return ctx.get_data("run", "s1_s2")

    ways = {"grouped": grouped, "single": single, "static": static}
    times = {name: [] for name in ways}
    tables = {}
    for rnd in range(args.warmup + args.repeats):
        for name, run in ways.items():
            t0 = time.perf_counter()
            tables[name] = run()
            dt = time.perf_counter() - t0
            if rnd >= args.warmup:
                times[name].append(dt)
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        streamed = name != "static"
        print(json.dumps({"way": name, "records": len(rec), "samples": int(pool.size), "rows": int(len(tables[name])),
                          "chunk_records": args.chunk_records if streamed else None,
                          "workers": args.workers if streamed else None,
                          "median_s": round(med[name], 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5),
                          "gsamples_per_s": round(pool.size / med[name] / 1e9, 3), "rounds": len(ts)}), flush=True)
    print(json.dumps({"grouped_over_single": round(med["grouped"] / med["single"], 4),
                      "grouped_over_static": round(med["grouped"] / med["static"], 4),
                      "tables_equal": tables["grouped"].tobytes() == tables["static"].tobytes(),
                      "settings_seen": tables["grouped"].tobytes() != tables["single"].tobytes()}), flush=True)

    # device profile of one chunk of the grouped stream
    chunk = next(grouped_stream._data_to_chunks(rec, "run"))
    dp.close()
    one = DevicePool([0], max_sessions=1)  # one session: the one compute_chunk borrows is the one profiled
    grouped_stream.device_pool = one
    grouped_stream.compute_chunk(chunk, SimpleContext(PER_CHANNEL, data), "run")  # (buffers sized, plan slots stored)
    with one.borrow() as sess:
        sess.profile(True)
    grouped_stream.compute_chunk(chunk, SimpleContext(PER_CHANNEL, data), "run")
    with one.borrow() as sess:
        report = sess.profile_report()
        sess.profile(False)
    print(json.dumps({"chunk_profile_ms": {k: round(ms, 4) for k, (ms, _n) in report.items()},
                      "chunk_records": len(chunk.data), "chunk_samples": int(chunk.data["event_length"].sum())}))
    one.close()


if __name__ == "__main__":
    main()
