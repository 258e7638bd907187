"""st_waveforms on one GPU: the pack kernel alone, and raw VX2730 CSV files -> st_waveforms end to end.

    python tools/st_waveforms_time.py [--pool-samples 1e9] [--e2e-samples 2.5e8] [--reps 3] [--skip-e2e]

(a) pack: k_st_pack over a resident pool of --pool-samples samples cut into rows of L samples, for L = 1500
    (VX2730-like) and L = 800.  Kernel ms = sum of the k_st_pack launches (profile_report, median of --reps calls);
    algorithmic bytes = 2 * sum(min(len, L)) read + n * (76 + 2L) written + 57 B of header columns per row read.
(b) e2e: HipWaveformsPlugin through a context on synthetic files (rows of 1000 samples, header row in the first file
    of each channel list); the same build through st_builder with its phase split: host text read + sniff, decode
    (text H2D through the staging ring + CSV kernels), gather + baseline, pack (kernel + D2H through the ring), and the
    kernel times of the pass.  Times are wall seconds (median of --reps); the files are read from the page cache.
One JSON line per measurement.
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waveformanalysis_amd import st_builder as SB  # noqa: E402
from waveformanalysis_amd.device import default_pool  # noqa: E402
from waveformanalysis_amd.plugin_api import SimpleContext  # noqa: E402
from waveformanalysis_amd.plugins import HipWaveformsPlugin  # noqa: E402

HBM_BYTES_PER_S = 8e12
HEADER_COLUMN_BYTES = 8 + 4 + 8 + 8 + 8 + 8 + 4 + 4 + 2 + 2 + 1   # src_offset, src_len, the eight columns, polarity


def pack_time(sess, pool_samples: int, L: int, reps: int) -> dict:
    n = pool_samples // L
    offsets = np.arange(n, dtype=np.int64) * L
    lengths = np.full(n, L, dtype=np.int32)
    cols = {"baseline": np.full(n, 8000.5), "baseline_upstream": np.nan, "timestamp": np.arange(n, dtype=np.int64),
            "record_id": np.arange(n, dtype=np.int64), "dt": 2, "event_length": lengths, "board": 0,
            "channel": (np.arange(n) % 64).astype(np.int16)}
    codes = np.zeros(n, dtype=np.uint8)
    kernel_ms, wall = [], []
    for _ in range(reps):
        sess.profile(True)
        t0 = time.perf_counter()
        out = sess.st_pack(L, offsets, lengths, cols, codes, ["unknown"], source="pool", src_samples=pool_samples)
        wall.append(time.perf_counter() - t0)
        kernel_ms.append(sess.profile_report().get("k_st_pack", (float("nan"), 0))[0])
        del out
    sess.profile(False)
    stride = 76 + 2 * L
    alg = 2 * n * L + n * stride + n * HEADER_COLUMN_BYTES
    ms = statistics.median(kernel_ms)
    return {"what": "st_pack", "L": L, "rows": n, "samples": n * L, "out_bytes": n * stride,
            "algorithmic_bytes": alg, "kernel_ms": ms, "kernel_bytes_per_s": alg / (ms * 1e-3),
            "share_of_8TBps": alg / (ms * 1e-3) / HBM_BYTES_PER_S, "call_s": statistics.median(wall)}


def e2e_time(sess, n_samples: int, reps: int) -> list[dict]:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from records_ingest_time import make_files

    root = tempfile.mkdtemp(prefix="wfa_st_time_")
    try:
        raw = make_files(root, n_samples, 8)
        text_bytes = sum(os.path.getsize(p) for g in raw for p in g)
        walls = []
        for _ in range(reps):
            ctx = SimpleContext({"show_progress": False}, {"raw_files": raw}, [HipWaveformsPlugin()])
            t0 = time.perf_counter()
            out = ctx.get_data("r0", "st_waveforms")
            walls.append(time.perf_counter() - t0)
        rows = len(out)
        samples = int(out["event_length"].astype(np.int64).sum())
        del out
        plugin = {"what": "st_waveforms_plugin", "rows": rows, "samples": samples, "text_bytes": text_bytes,
                  "call_s": statistics.median(walls), "text_bytes_per_s": text_bytes / statistics.median(walls),
                  "samples_per_s": samples / statistics.median(walls)}
        splits = []
        for _ in range(reps):
            timings: dict = {}
            sess.profile(True)
            t0 = time.perf_counter()
            out = SB.build_st_waveforms_from_vx2730_files(raw, session=sess, timings=timings)
            timings["total"] = time.perf_counter() - t0
            timings["kernels_ms"] = {k: v[0] for k, v in sess.profile_report().items()}
            timings["h2d_GBps_last_part"] = sess.last_h2d_rate()
            splits.append(timings)
            del out
        sess.profile(False)
        best = min(splits, key=lambda t: t["total"])
        return [plugin, {"what": "st_waveforms_phases", "rows": rows, "text_bytes": text_bytes, **best}]
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool-samples", type=float, default=1e9)
    ap.add_argument("--e2e-samples", type=float, default=2.5e8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    sess = default_pool().session()
    n = int(args.pool_samples)
    pool = np.tile(np.arange(8000, 8000 + 4096, dtype=np.uint16), n // 4096 + 1)[:n]
    sess.upload_pool(pool)
    del pool
    for L in (1500, 800):
        print(json.dumps(pack_time(sess, n, L, args.reps)), flush=True)
    sess.forget_resident()
    if not args.skip_e2e:
        for line in e2e_time(sess, int(args.e2e_samples), args.reps):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
