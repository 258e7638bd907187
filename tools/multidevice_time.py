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

The `dense` leg times the default route (wave_source="auto") on the array tools/dense_time.py uses (`--dense-records` x
800 samples, default 625 000 = 5e8 samples, the positive twin of the synthetic V1725 run): the chain hit_threshold ->
basic_features -> waveform_width_integral -> hit -> waveform_width, then filtered_waveforms on its own, with
devices=None, [0] and every visible device.  Per set, on one context: the first run (rows uploaded), then `--calls`
repetitions with the context's results forgotten and the rows resident; wall time of the chain and of every plugin,
pool uploads per session, tables compared byte for byte with devices=None.

    python tools/multidevice_time.py [--samples 1e9] [--calls 5] [--legs hit_threshold,wave_pool_filtered,hit,dense]
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
    HipBasicFeaturesPlugin,
    HipFilteredWaveformsPlugin,
    HipHitFinderPlugin,
    HipThresholdHitPlugin,
    HipWaveformWidthIntegralPlugin,
    HipWaveformWidthPlugin,
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


DENSE_CHAIN = ("hit_threshold", "basic_features", "waveform_width_integral", "hit", "waveform_width")


def dense_set(st, rec, devices, calls, want=None):
    """The dense chain and filtered_waveforms on one context with `devices`: (tables of the first run, JSON line)."""
    ctx = SimpleContext({"hit": {"use_filtered": False}, "devices": devices}, {"st_waveforms": st, "records": rec},
                        plugins=[HipThresholdHitPlugin(), HipBasicFeaturesPlugin(), HipWaveformWidthIntegralPlugin(),
                                 HipHitFinderPlugin(), HipWaveformWidthPlugin(), HipFilteredWaveformsPlugin()])
    sessions = _sessions(ctx, devices)
    if devices is None:
        sessions[0].forget_resident()  # the calling thread's session outlives the sets: start from an empty one

    def once():
        ctx._results.clear()
        before = [s.uploads for s in sessions]
        took, tables = {}, {}
        for name in DENSE_CHAIN + ("filtered_waveforms",):
            t0 = time.perf_counter()
            tables[name] = ctx.get_data("run", name)
            took[name] = time.perf_counter() - t0
        return tables, took, [s.uploads - b for s, b in zip(sessions, before)]

    def chain_s(took):
        return sum(took[name] for name in DENSE_CHAIN)

    tables, first, first_uploads = once()
    same = None if want is None else all(tables[k].tobytes() == want[k].tobytes() for k in tables)
    repeats = [once()[1:] for _ in range(calls)]  # (the tables of a repetition are dropped: filtered_waveforms is large)
    MD.close_sharded_runs(ctx)
    walls = [chain_s(took) for took, _u in repeats]
    line = {"leg": "dense", "devices": devices, "rows": len(st), "samples": int(st["wave"].size),
            "table_rows": {k: len(tables[k]) for k in DENSE_CHAIN}, "identical_to_single": same,
            "first_chain_s": round(chain_s(first), 4), "first_uploads_per_session": first_uploads,
            "chain_s": {"median": round(statistics.median(walls), 4), "min": round(min(walls), 4),
                        "max": round(max(walls), 4)},
            "plugins_s": {k: round(statistics.median(took[k] for took, _u in repeats), 4) for k in first},
            "first_filtered_waveforms_s": round(first["filtered_waveforms"], 4),
            "uploads_per_session": repeats[-1][1]}
    return tables, line


def dense_leg(n_records, calls) -> None:
    from waveformanalysis_amd import replay

    rec, pool = replay.mirror_positive(*synth.make_run(n_records, "v1725", cfg=7))
    st = replay.st_waveforms_from_records(rec, pool)
    del pool
    n_dev = device_count()
    want = None
    for devices in [None, [0]] + ([list(range(n_dev))] if n_dev > 1 else []):
        tables, line = dense_set(st, rec, devices, calls, want)
        want = tables if devices is None else want
        print(json.dumps(line), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=float, default=1e9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--dense-records", type=int, default=625000)
    ap.add_argument("--legs", default=",".join(LEGS) + ",dense", help="comma-separated: " + ", ".join(LEGS) + ", dense")
    args = ap.parse_args()
    legs = [leg.strip() for leg in args.legs.split(",") if leg.strip()]
    unknown = [leg for leg in legs if leg not in LEGS and leg != "dense"]
    if unknown:
        ap.error(f"unknown legs {unknown}")
    if "dense" in legs:
        legs.remove("dense")
        dense_leg(args.dense_records, args.calls)
        if not legs:
            return
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
