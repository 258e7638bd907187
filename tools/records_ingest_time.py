"""Raw VX2730 CSV files -> records + wave_pool -> hit_threshold: time of each leg on one GPU.

    python tools/records_ingest_time.py [--samples 1e8] [--files 4] [--parts 8] [--reps 3]

Prints, for synthetic files of rows of 1000 samples (header row in the first file of each channel):
  one_part   build_records_from_vx2730_files with the whole text in one decode call (text GB/s of the build)
  n_parts    the same build cut into --parts parts through the sample arena (text GB/s)
  plugins    HipRecordsPlugin + HipWavePoolPlugin through a context (raw files -> bundle)
  hits_resident  hit_threshold right after the build, on the pool the gather left on the device
  hits_upload    the same pass on the same pool handed over as plain data (one more upload)
Times are wall seconds of the host call (median of --reps); the files are read from the page cache.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveformanalysis_amd import records_builder as RB  # noqa: E402
from waveformanalysis_amd.device import default_pool  # noqa: E402
from waveformanalysis_amd.plugin_api import SimpleContext  # noqa: E402
from waveformanalysis_amd.plugins import HipThresholdHitPlugin  # noqa: E402
from waveformanalysis_amd.plugins.records import HipRecordsPlugin, HipWavePoolPlugin  # noqa: E402

L = 1000
HEADER = b"BOARD;CHANNEL;TIMETAG;ENERGY;ENERGYSHORT;FLAGS;PROBE_CODE;SAMPLES\n"


def make_files(root: str, n_samples: int, n_files: int, seed: int = 0) -> list[list[str]]:
    """n_files files over 2 channel lists; rows drawn from a block of 256 distinct noisy pulses."""
    rng = np.random.default_rng(seed)
    block = np.clip(8000 + np.round(rng.normal(0, 3, (256, L))), 0, 16383).astype(np.int64)
    block[:, 300:320] -= rng.integers(20, 2000, (256, 1))
    bodies = [";".join(map(str, row)).encode() for row in block.tolist()]
    rows_per_file = max(1, n_samples // (L * n_files))
    groups: list[list[str]] = [[], []]
    for f in range(n_files):
        ch = f % 2
        ts = np.sort(rng.integers(0, 10**12, rows_per_file))
        pick = rng.integers(0, 256, rows_per_file)
        text = b"".join(b"0;%d;%d;0;0;0x4000;1;%s\n" % (ch, t, bodies[p]) for t, p in zip(ts.tolist(), pick.tolist()))
        path = os.path.join(root, f"DataR_CH{ch}@ingest_{f}.CSV")
        with open(path, "wb") as fh:
            fh.write((HEADER if not groups[ch] else b"") + text)
        groups[ch].append(path)
    return groups


def median_time(fn, reps: int) -> tuple[float, object]:
    times, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=float, default=1e8)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="wfa_ingest_") as root:
        groups = make_files(root, int(args.samples), args.files)
        text_bytes = sum(os.path.getsize(p) for g in groups for p in g)
        sess = default_pool().session()
        RB.build_records_from_vx2730_files(groups, 2, session=sess, part_bytes=64 << 20)   # warm-up
        out: dict = {"samples": None, "text_GB": text_bytes / 1e9, "parts": args.parts}
        if text_bytes < 2**31:
            t1, b1 = median_time(lambda: RB.build_records_from_vx2730_files(groups, 2, session=sess), args.reps)
            out["one_part_s"], out["one_part_text_GBps"] = t1, text_bytes / t1 / 1e9
        part_bytes = -(-text_bytes // args.parts)
        tn, bn = median_time(lambda: RB.build_records_from_vx2730_files(groups, 2, session=sess, part_bytes=part_bytes),
                             args.reps)
        out["samples"] = int(len(bn.wave_pool))
        out["n_parts_s"], out["n_parts_text_GBps"] = tn, text_bytes / tn / 1e9
        hit_cfg = {"wave_source": "records", "threshold": 15.0}

        def plugin_run():
            ctx = SimpleContext({"dt": 2, "hit_threshold": hit_cfg}, {"raw_files": groups},
                                [HipRecordsPlugin(part_bytes), HipWavePoolPlugin(part_bytes), HipThresholdHitPlugin()])
            t0 = time.perf_counter()
            rec, pool = ctx.get_data("r", "records"), ctx.get_data("r", "wave_pool")
            t1 = time.perf_counter()
            hits = ctx.get_data("r", "hit_threshold")
            t2 = time.perf_counter()
            plain = SimpleContext({"hit_threshold": hit_cfg}, {"records": rec, "wave_pool": pool.copy()},
                                  [HipThresholdHitPlugin()])
            t3 = time.perf_counter()
            hits2 = plain.get_data("r", "hit_threshold")
            t4 = time.perf_counter()
            assert hits.tobytes() == hits2.tobytes()
            return t1 - t0, t2 - t1, t4 - t3, len(hits)

        runs = [plugin_run() for _ in range(args.reps)]
        out["plugins_build_s"] = statistics.median(r[0] for r in runs)
        out["hits_resident_s"] = statistics.median(r[1] for r in runs)
        out["hits_upload_s"] = statistics.median(r[2] for r in runs)
        out["hits"] = runs[-1][3]
        out["raw_to_hits_resident_s"] = out["plugins_build_s"] + out["hits_resident_s"]
        out["raw_to_hits_text_GBps"] = text_bytes / out["raw_to_hits_resident_s"] / 1e9
    for k, v in out.items():
        print(f"  {k}: {v:.4g}" if isinstance(v, float) else f"  {k}: {v}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
