"""Wall time of the S1/S2 chain of the records route: host arrays in, host s1_s2 rows out, two ways.

Data: a synthetic positive-pulse run, replay.mirror_positive(*synth.make_run(records, "v1725", cfg=17)) (uniform
L = 800), with the hit options and class ranges of the config-5 replay.

  static   the plugin chain wave_pool_filtered -> hit -> waveform_width -> s1_s2 with basic_features on the side
           (hip_default(), wave_source="records") on a new Context per round: every table crosses the bus;
  stream   HipS1S2Stream over the same arrays in chunks of `--chunk-records` records, `--workers` worker threads:
           the chunk's samples and records up, the labelled rows down.

After `--warmup` rounds (every way once per round: buffers sized, clocks up) the two ways alternate for `--repeats`
rounds in one process; per way the median, the fastest and the slowest round and Gsamples/s at the median.  One JSON
line per way, one with the ratio and whether the tables are equal byte for byte, then the device profile of one chunk
of the stream.

    python tools/s1s2_stream_time.py [--records 100000] [--chunk-records 25000] [--workers 2] [--warmup 2] [--repeats 7]
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
    stream = HipS1S2Stream(device_pool=dp)
    streaming_config = {"chunk_size": args.chunk_records, "max_workers": args.workers, "parallel": args.workers > 1}

    def static():
        default_pool().session().forget_resident()  # a new run: its pool goes up again
        ctx = SimpleContext(CONFIG, data, plugins=hip_default())
        return ctx.get_data("run", "s1_s2")

    def streamed():
        outs = stream.compute(SimpleContext(CONFIG, data), "run", streaming_config=streaming_config)
        return np.concatenate([o.data for o in outs])

    ways = {"static": static, "stream": streamed}
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
        print(json.dumps({"way": name, "records": len(rec), "samples": int(pool.size), "rows": int(len(tables[name])),
                          "chunk_records": args.chunk_records if name == "stream" else None,
                          "workers": args.workers if name == "stream" else None,
                          "median_s": round(med[name], 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5),
                          "gsamples_per_s": round(pool.size / med[name] / 1e9, 3), "rounds": len(ts)}))
    print(json.dumps({"stream_over_static": round(med["stream"] / med["static"], 4),
                      "tables_equal": tables["stream"].tobytes() == tables["static"].tobytes()}))

    # device profile of one chunk of the stream
    chunk = next(stream._data_to_chunks(rec, "run"))
    dp.close()
    one = DevicePool([0], max_sessions=1)  # one session: the one compute_chunk borrows is the one profiled
    stream.device_pool = one
    stream.compute_chunk(chunk, SimpleContext(CONFIG, data), "run")  # (buffers sized)
    with one.borrow() as sess:
        sess.profile(True)
    stream.compute_chunk(chunk, SimpleContext(CONFIG, data), "run")
    with one.borrow() as sess:
        report = sess.profile_report()
        sess.profile(False)
    print(json.dumps({"chunk_profile_ms": {k: round(ms, 4) for k, (ms, _n) in report.items()},
                      "chunk_records": len(chunk.data), "chunk_samples": int(chunk.data["event_length"].sum())}))
    one.close()


if __name__ == "__main__":
    main()
