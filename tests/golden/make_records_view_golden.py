"""Generate tests/golden/vx2730csv_records_view.npz from the reference's RecordsView
(waveform_analysis/core/data/records_view.py).  Run where the reference package is importable, as make_golden.py is:

    python tests/golden/make_records_view_golden.py

One crafted run (40 ragged records: lengths 0, 1, 7, 8, 9 and 1500 among them, even and odd pool offsets, gaps between
records, record ids neither sorted nor contiguous, the three polarities mixed, baselines no float32 holds exactly, one
baseline equal to a sample of a "positive" record so that its signal holds -0.0, samples 0 and 65535, tied timestamps)
and, for a fixed list of calls, what RecordsView returned.  A float32 pool (the same samples after a fixed float32 map)
stands for wave_pool_filtered.  Only arrays are stored; the call list travels as JSON bytes.
(The vx2730csv_ prefix keeps the file out of the per-case parity suites, which take every other fixture for a run with
recorded plugin outputs: golden_util.case_names.)
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from waveform_analysis.core.data.records_view import RecordsView  # noqa: E402
from waveform_analysis.core.processing.records_builder import RECORDS_DTYPE  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "vx2730csv_records_view.npz")

LENGTHS = [0, 1, 7, 8, 9, 1500, 16, 17, 33, 64, 100, 255, 256, 3, 5, 12, 40, 31, 0, 2,
           63, 65, 24, 15, 10, 6, 4, 11, 13, 128, 50, 9, 8, 7, 1, 20, 30, 45, 70, 90]
GAPS = [0, 3, 0, 1, 2, 0, 5, 0, 1, 0, 7, 0, 0, 1, 4, 0, 1, 1, 0, 2,
        0, 1, 0, 3, 1, 0, 0, 1, 2, 0, 1, 1, 0, 0, 6, 1, 0, 3, 0, 1]   # unused samples before each record
POLARITY = ["positive", "negative", "unknown"]
MINUS_ZERO_ROW = 9   # "positive", baseline 500.0, and its sample 5 is 500


def make_run():
    rng = np.random.default_rng(20261016)
    n = len(LENGTHS)
    rec = np.zeros(n, dtype=RECORDS_DTYPE)
    offsets, at = [], 1   # the first record starts at an odd sample
    for gap, length in zip(GAPS, LENGTHS):
        at += gap
        offsets.append(at)
        at += length
    pool = rng.integers(0, 65536, size=at + 5, dtype=np.uint16)
    rec["wave_offset"] = offsets
    rec["event_length"] = LENGTHS
    assert {o & 1 for o in offsets} == {0, 1}
    rec["record_id"] = (rng.permutation(n) * 7 + 1000).astype(np.int64)   # neither sorted nor contiguous
    rec["timestamp"] = np.sort(rng.integers(10_000, 10_400, size=n)) // 8 * 8   # sorted, with ties
    assert len(np.unique(rec["timestamp"])) < n
    rec["board"] = rng.integers(0, 2, size=n)
    rec["channel"] = rng.integers(0, 8, size=n)
    rec["dt"] = 2
    rec["polarity"] = [POLARITY[k % 3] if k % 5 else POLARITY[(k // 5) % 3] for k in range(n)]
    rec["baseline"] = rng.uniform(100.0, 16000.0, size=n) + 1.0 / 3.0
    assert np.all(rec["baseline"].astype(np.float32).astype(np.float64) != rec["baseline"])
    # extremes, and the -0.0 case
    row = int(np.flatnonzero(np.asarray(LENGTHS) >= 64)[0])
    pool[offsets[row]] = 0
    pool[offsets[row] + 1] = 65535
    rec["polarity"][MINUS_ZERO_ROW] = "positive"
    rec["baseline"][MINUS_ZERO_ROW] = 500.0
    pool[offsets[MINUS_ZERO_ROW] + 5] = 500
    pool_f32 = pool.astype(np.float32) * np.float32(0.37) + np.float32(0.125)   # the fixed float32 map
    return rec, pool, pool_f32


def make_calls(rec):
    ids = [int(i) for i in rec["record_id"]]
    by_len = {int(n): int(i) for i, n in zip(rec["record_id"], rec["event_length"])}   # last record of each length
    everything = ids[::-1]
    long_id = by_len[1500]
    rep = [long_id, ids[0], ids[3], ids[3], ids[1], ids[2], ids[4], ids[7], ids[7], ids[33], ids[12], ids[MINUS_ZERO_ROW]]
    small = [i for i in ids[::-2] if i != long_id] + [ids[2], ids[2], ids[MINUS_ZERO_ROW], ids[18]]
    calls = []

    def add(pool, method, target, **kwargs):
        calls.append({"pool": pool, "method": method, "ids": target, "kwargs": kwargs})

    windows = [(-3, None), (5, None), (2000, None), (0, 0), (2, 6), (4, 5000), (9, 3), (-1, 8), (0, -2)]
    for pool in ("u16", "f32"):
        add(pool, "waves", everything)
        add(pool, "waves", everything, mask=True, dtype="float32")
        add(pool, "waves", small, dtype="float64", pad_to=300, mask=True)
        add(pool, "waves", everything, baseline_correct=True)
        add(pool, "waves", small, baseline_correct=True, dtype="float64", mask=True)
        add(pool, "signals", everything, mask=True)
        add(pool, "signals", small, dtype="float64")
        add(pool, "signals", rep, pad_to=1600, mask=True)
        add(pool, "signals", rep[::-1], dtype="float64", sample_start=1490)
        for start, end in windows:
            add(pool, "signals", small, mask=True, sample_start=start, sample_end=end)
            add(pool, "waves", small, baseline_correct=True, dtype="float64", sample_start=start, sample_end=end)
        add(pool, "waves", small, sample_start=3, sample_end=11, pad_to=8, mask=True)
        add(pool, "signals", small, dtype="float32", sample_start=1, sample_end=2, pad_to=1)
        add(pool, "waves", [], mask=True)
        add(pool, "signals", [], dtype="float64", mask=True)
        add(pool, "signals", [], pad_to=4)
        for length in (0, 1, 7, 8, 9):
            add(pool, "waves", by_len[length])
            add(pool, "signals", by_len[length])
            add(pool, "signals", by_len[length], dtype="float64", baseline=1234.56789)
        add(pool, "waves", long_id, sample_start=3, sample_end=20)
        add(pool, "waves", long_id, dtype="float32", sample_start=1499)
        add(pool, "waves", long_id, baseline_correct=True, sample_start=-5, sample_end=9)
        add(pool, "waves", long_id, baseline_correct=True, dtype="float64", sample_start=700, sample_end=733)
        add(pool, "signals", long_id, sample_start=1400)
        add(pool, "signals", ids[MINUS_ZERO_ROW])
        add(pool, "signals", ids[MINUS_ZERO_ROW], dtype="float64")
        add(pool, "signals", ids[MINUS_ZERO_ROW], baseline=float(np.float32(0.1)), sample_start=2, sample_end=9)
        add(pool, "signals", ids[12], sample_start=300)
        add(pool, "signals", ids[12], sample_start=10, sample_end=2)
    ts = rec["timestamp"]
    tied = int(ts[np.flatnonzero(np.diff(ts) == 0)[0]])
    for t_min, t_max in [(None, None), (int(ts[7]), None), (None, int(ts[20])), (tied, tied), (tied - 1, tied + 1),
                         (int(ts[0]) - 50, int(ts[0]) - 10), (int(ts[-1]) + 1, None), (int(ts[30]), int(ts[5])),
                         (int(ts[3]) + 1, int(ts[33]) - 1)]:
        calls.append({"pool": "u16", "method": "query_time_window", "t_min": t_min, "t_max": t_max, "kwargs": {}})
    return calls


def main():
    rec, pool, pool_f32 = make_run()
    views = {"u16": RecordsView(rec, pool), "f32": RecordsView(rec, pool_f32)}
    calls = make_calls(rec)
    out = {"records": rec, "wave_pool": pool, "wave_pool_f32": pool_f32,
           "calls_json": np.frombuffer(json.dumps(calls).encode(), dtype=np.uint8)}
    minus_zero = False
    for k, call in enumerate(calls):
        view = views[call["pool"]]
        if call["method"] == "query_time_window":
            out[f"c{k}_record_id"] = np.ascontiguousarray(view.query_time_window(call["t_min"], call["t_max"])["record_id"])
            continue
        kwargs = dict(call["kwargs"])
        if "dtype" in kwargs:
            kwargs["dtype"] = np.dtype(kwargs["dtype"]).type
        got = getattr(view, call["method"])(call["ids"], **kwargs)
        values = got[0] if isinstance(got, tuple) else got
        out[f"c{k}_values"] = values
        if isinstance(got, tuple):
            out[f"c{k}_mask"] = got[1]
        if values.dtype.kind == "f":
            minus_zero |= bool(np.any((values == 0) & np.signbit(values)))
    assert minus_zero, "the -0.0 case is gone"
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(calls)} calls, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
