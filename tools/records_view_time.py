"""HipRecordsView.signals on one GPU against a numpy per-record loop, and the gather kernel against k_st_pack.

    python tools/records_view_time.py [--ids 1000,10000,100000] [--reps 7] [--step-timeout 300]

For a synthetic run (synth.make_run, 800-sample records) and n ids (every record once, random order), pool and records
already resident: `signals(ids, mask=True)` as float32 and float64.
  kernel_ms           sum of the k_view_gather launches of one call (profile_report), median of --reps calls after two
                      warm-up calls, with min / max
  algorithmic bytes   per output column: 2 B read + itemsize + 1 (mask) B written
  call_s              wall time of view.signals (allocates its output), median
  reused_out_s        wall time of DeviceSession.view_gather into an output allocated and touched before: kernel + copy
                      out through the staging ring; copy_out_bytes_per_s = output bytes / (reused_out_s - kernel time)
  numpy_s             the same request through tests/records_view_util.NumpyRecordsView (one slice, one cast, one
                      subtraction and two row assignments per record), on the same box
and k_st_pack (tools/st_waveforms_time.pack_time) over the same pool cut into the same rows, for the per-byte comparison.
Every n runs in a child process of its own under --step-timeout; the first failure ends the run.  One JSON line per
measurement.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

HBM_BYTES_PER_S = 8e12
L = 800


def step(n: int, reps: int) -> None:
    from st_waveforms_time import pack_time
    from tests import records_view_util as U
    from waveformanalysis_amd import synth
    from waveformanalysis_amd.device import default_pool
    from waveformanalysis_amd.records_view import HipRecordsView

    rec, pool = synth.make_run(n, "v1725", cfg=9)
    rng = np.random.default_rng(n)
    rec["polarity"] = rng.choice(["positive", "negative", "unknown"], size=n)
    ids = rng.permutation(rec["record_id"])
    sess = default_pool().session()
    view = HipRecordsView(rec, pool, session=sess)
    rows = view._resolve_record_indices(ids)
    reference = U.NumpyRecordsView(rec, pool)
    for dtype in (np.float32, np.float64):
        itemsize = np.dtype(dtype).itemsize
        t0 = time.perf_counter()
        want = reference.signals(ids, mask=True, dtype=dtype)
        numpy_s = time.perf_counter() - t0
        for _ in range(2):  # warm-up: uploads, scratch, clocks
            got = view.signals(ids, mask=True, dtype=dtype)
        U.assert_same_bytes(got, want, f"n={n} {np.dtype(dtype)}")
        kernel_ms, call_s, reused_s = [], [], []
        out = np.zeros((n, L), dtype=dtype)
        for _ in range(reps):
            sess.profile(True)
            t0 = time.perf_counter()
            got = view.signals(ids, mask=True, dtype=dtype)
            call_s.append(time.perf_counter() - t0)
            kernel_ms.append(sess.profile_report()["k_view_gather"][0])
            del got
            t0 = time.perf_counter()
            sess.view_gather(rows, mode="signals", source="u16", out_dtype=dtype, pad_len=L, out=out)
            reused_s.append(time.perf_counter() - t0)
        sess.profile(False)
        alg = n * L * (2 + itemsize + 1)
        out_bytes = n * L * (itemsize + 1)
        ms = statistics.median(kernel_ms)
        reused = statistics.median(reused_s)
        print(json.dumps({
            "what": "signals", "ids": n, "L": L, "dtype": np.dtype(dtype).name, "algorithmic_bytes": alg,
            "kernel_ms": ms, "kernel_ms_min": min(kernel_ms), "kernel_ms_max": max(kernel_ms),
            "kernel_bytes_per_s": alg / (ms * 1e-3), "share_of_8TBps": alg / (ms * 1e-3) / HBM_BYTES_PER_S,
            "call_s": statistics.median(call_s), "call_s_min": min(call_s), "call_s_max": max(call_s),
            "reused_out_s": reused, "out_bytes": out_bytes,
            "copy_out_bytes_per_s": n * L * itemsize / max(reused - ms * 1e-3, 1e-9),
            "numpy_s": numpy_s, "numpy_over_call": numpy_s / statistics.median(call_s),
            "h2d_GBps_pool_upload": sess.last_h2d_rate()}), flush=True)
    print(json.dumps(pack_time(sess, n * L, L, reps)), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", default="1000,10000,100000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--step", type=int, default=0, help="(internal) run one n in this process")
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps)
        return
    for n in (int(x) for x in args.ids.split(",")):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(n), "--reps", str(args.reps)],
                                timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:  # nothing more is started on the device after a failed step
            print(json.dumps({"what": "signals", "ids": n, "failed": rc}), flush=True)
            sys.exit(1)


if __name__ == "__main__":
    main()
