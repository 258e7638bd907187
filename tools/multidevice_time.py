"""End-to-end time of per-record plugin calls across device sets: host records + pool in, host output out.

Data: the synthetic V1725 chunk of 10^9 samples (synth.make_run).  Legs (--legs, default all three):
  hit_threshold       fused Savitzky-Golay route (use_filtered + fuse_filter) on wave_pool;
  wave_pool_filtered  Butterworth (0.01-0.2 at fs 0.5, order 4), unfused: the float32 pool comes back to the host;
  hit                 find_peaks on wave_pool_filtered (the devices=None output of the leg above).
Device sets: devices=None, [0], [0,1], [0..3], [0..7], limited to the visible devices.  For each leg and set: the first
call, the median of the next calls with the input pool uploaded again (a new view of the same memory: the residency
rule keys on the array object), and the median of calls with the pool resident.  Gsamples/s over the whole call, and
the H2D rate of the last upload of every session.  Every set's output is checked byte-identical to devices=None.  One
JSON line per leg and set.

    python tools/multidevice_time.py [--samples 1e9] [--calls 5] [--legs hit_threshold,wave_pool_filtered,hit]
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

from waveformanalysis_amd import multidevice as MD, synth  # noqa: E402
from waveformanalysis_amd.device import default_pool, device_count  # noqa: E402
from waveformanalysis_amd.plugin_api import SimpleContext  # noqa: E402
from waveformanalysis_amd.plugins import (  # noqa: E402
    HipHitFinderPlugin,
    HipThresholdHitPlugin,
    HipWavePoolFilteredPlugin,
)

# leg -> (plugin, the input whose array object is swapped between calls, configuration)
LEGS = {
    "hit_threshold": (HipThresholdHitPlugin, "wave_pool", {"use_filtered": True, "fuse_filter": True}),
    "wave_pool_filtered": (HipWavePoolFilteredPlugin, "wave_pool",
                           {"filter_type": "BW", "lowcut": 0.01, "highcut": 0.2, "fs": 0.5, "filter_order": 4}),
    "hit": (HipHitFinderPlugin, "wave_pool_filtered", {"use_filtered": True}),
}


def _sessions(ctx, devices):
    if devices is None:
        return [default_pool().session()]
    return MD.sharded_run(ctx, devices).sessions


def time_set(leg, data, devices, calls, want=None):
    plugin_cls, swapped, config = LEGS[leg]
    ctx = SimpleContext({"wave_source": "records", "devices": devices, **config}, dict(data))
    plugin = plugin_cls()
    pool = data[swapped]

    def call(p):
        ctx._data[swapped] = p
        t0 = time.perf_counter()
        out = plugin.compute(ctx, "run")
        dt = time.perf_counter() - t0
        plugin.cleanup(ctx)
        return out, dt

    rows, first = call(pool[:])
    same = None if want is None else bool(len(rows) == len(want) and rows.tobytes() == want.tobytes())
    upload = [call(pool[:])[1] for _ in range(calls)]
    h2d = [round(s.last_h2d_rate(), 1) for s in _sessions(ctx, devices)]
    resident_pool = pool[:]
    call(resident_pool)
    resident = [call(resident_pool)[1] for _ in range(calls)]
    MD.close_sharded_runs(ctx)
    n = pool.size
    med_u, med_r = statistics.median(upload), statistics.median(resident)
    out = {"leg": leg, "devices": devices, "rows": int(len(rows)), "identical_to_single": same,
           "first_s": round(first, 4), "median_s": round(med_u, 4), "gsamples_per_s": round(n / med_u / 1e9, 2),
           "resident_median_s": round(med_r, 4), "resident_gsamples_per_s": round(n / med_r / 1e9, 2),
           "h2d_GBps_per_session": h2d}
    return rows, out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=float, default=1e9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated: " + ", ".join(LEGS))
    args = ap.parse_args()
    legs = [leg.strip() for leg in args.legs.split(",") if leg.strip()]
    unknown = [leg for leg in legs if leg not in LEGS]
    if unknown:
        ap.error(f"unknown legs {unknown}")
    L = synth.PRESETS["v1725"][0]
    t0 = time.perf_counter()
    rec, pool = synth.make_run(int(args.samples) // L, "v1725", cfg=0)
    print(json.dumps({"records": len(rec), "samples": int(pool.size), "synth_s": round(time.perf_counter() - t0, 1),
                      "visible_devices": device_count()}), flush=True)
    n_dev = device_count()
    sets = [None] + [list(range(k)) for k in (1, 2, 4, 8) if k <= n_dev]
    data = {"records": rec, "wave_pool": pool}
    for leg in legs:
        if leg == "hit" and "wave_pool_filtered" not in data:  # its input: one devices=None filter call
            fctx = SimpleContext({"wave_source": "records", **LEGS["wave_pool_filtered"][2]}, dict(data))
            data["wave_pool_filtered"] = HipWavePoolFilteredPlugin().compute(fctx, "run")
        want = None
        for devices in sets:
            rows, line = time_set(leg, data, devices, args.calls, want)
            if devices is None:
                want = rows
                if leg == "wave_pool_filtered":
                    data["wave_pool_filtered"] = rows
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
