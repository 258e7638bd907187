"""Wall time of the streaming hit ring under per-channel filter settings: host chunks in, host hit rows out.

Data: a synthetic V1725 run (synth.make_run, uniform L = 800) cut into bench-sized chunks (`--chunk-records`, default
50 000 = 4e7 samples per chunk); the records' channels are rewritten to k % 3 of board 0 and the three channels take the
Savitzky-Golay pairs (11, 2), (7, 3) and (21, 4) -- the last one outside the streaming kernel's windows -- with thresholds
10 / 8 / 10.  The ring (HipThresholdHitStream.run_chunks, two sessions on device 0) runs the chunk list in two ways:

  one_group     the default path: SG(11, 2) and one threshold for every record, one queued pass per chunk;
  queued        filter_source="wave_pool_filtered": the three groups through one wfa_hits_enqueue_groups per chunk.

After `--warmup` rounds (every way once per round: buffers sized, clocks up) the two ways alternate for `--repeats`
rounds; per way the median, the fastest and the slowest round, Gsamples/s at the median, and the median host time one
chunk spends in _stage (uploads, queueing and whatever the host waits for there).  One JSON line per way, then one with
the ratio.

    python tools/stream_groups_time.py [--records 400000] [--chunk-records 50000] [--warmup 2] [--repeats 7]
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
from waveformanalysis_amd.plugin_api import SimpleContext  # noqa: E402
from waveformanalysis_amd.plugins import HipWavePoolFilteredPlugin  # noqa: E402
from waveformanalysis_amd.streaming import HipThresholdHitStream, records_to_chunks  # noqa: E402

FILTER_CC = {"0:1": {"sg_window_size": 7, "sg_poly_order": 3}, "0:2": {"sg_window_size": 21, "sg_poly_order": 4}}
HIT_CC = {"0:1": {"threshold": 8.0}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=400_000)
    ap.add_argument("--chunk-records", type=int, default=50_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    rec, pool = synth.make_run(args.records, "v1725", cfg=5)
    L = int(rec["event_length"][0])
    rec["board"], rec["channel"] = 0, np.arange(len(rec)) % 3
    rec["baseline"] = pool.reshape(len(rec), L)[:, : synth.BASELINE_SAMPLES].mean(axis=1)
    chunks = records_to_chunks(rec, args.chunk_records, "run")
    data = {"records": rec, "wave_pool": pool}
    grouped = {"use_filtered": True, "filter_source": "wave_pool_filtered", "channel_config": HIT_CC}
    ctx_one = SimpleContext({"hit_threshold_stream": {"use_filtered": True}}, data)
    ctx_groups = SimpleContext({"hit_threshold_stream": grouped, "wave_pool_filtered": {"channel_config": FILTER_CC}}, data,
                               plugins=[HipWavePoolFilteredPlugin()])
    dp = DevicePool([0])
    ways = {
        "one_group": (HipThresholdHitStream(device_pool=dp), ctx_one),
        "queued": (HipThresholdHitStream(device_pool=dp), ctx_groups),
    }
    times = {name: [] for name in ways}
    stage = {name: [] for name in ways}     # host time inside _stage per chunk: uploads + whatever the host waits for
    tables = {}
    for rnd in range(args.warmup + args.repeats):
        for name, (plugin, ctx) in ways.items():
            t0 = time.perf_counter()
            timeline = []
            outs = plugin.run_chunks(chunks, ctx, "run", max_workers=2, timeline=timeline)  # every chunk's rows on the host
            dt = time.perf_counter() - t0
            if rnd >= args.warmup:
                times[name].append(dt)
                stage[name] += [queued - begin for _k, begin, queued, _collected in timeline]
            tables[name] = np.concatenate([o.data for o in outs])
    dp.close()
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        print(json.dumps({"way": name, "chunks": len(chunks), "samples": int(pool.size), "rows": int(len(tables[name])),
                          "median_s": round(med[name], 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5),
                          "gsamples_per_s": round(pool.size / med[name] / 1e9, 3), "rounds": len(ts),
                          "stage_ms_per_chunk_median": round(1e3 * statistics.median(stage[name]), 3)}))
    print(json.dumps({"queued_over_one_group": round(med["queued"] / med["one_group"], 4)}))


if __name__ == "__main__":
    main()
