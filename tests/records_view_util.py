"""A small numpy restatement of the reference's RecordsView (core/data/records_view.py:16-400) and the loader of
tests/golden/vx2730csv_records_view.npz (made by tests/golden/make_records_view_golden.py from the reference itself).

NumpyRecordsView is what the GPU tests and tools/records_view_time.py compare HipRecordsView against on inputs the
fixture does not hold; tests/test_records_view_cpu.py pins it to the fixture byte for byte.  Arithmetic per sample: the
cast to the output type, one subtraction of the baseline rounded once to the output type, unary minus for records
whose polarity is exactly "positive"."""

from __future__ import annotations

import json
import os

import numpy as np

from tests import golden_util as G

FIXTURE = os.path.join(G.GOLDEN, "vx2730csv_records_view.npz")


class NumpyRecordsView:
    def __init__(self, records: np.ndarray, wave_pool: np.ndarray):
        self.records = records
        self.wave_pool = wave_pool
        self.row_of = {int(rid): i for i, rid in enumerate(records["record_id"])}
        names = records.dtype.names
        self.positive = (np.asarray(records["polarity"]).astype("U16") == "positive") if "polarity" in names \
            else np.zeros(len(records), dtype=bool)

    def __len__(self):
        return len(self.records)

    def _row(self, record_id: int) -> int:
        if int(record_id) not in self.row_of:
            raise KeyError(f"Unknown record_id: {int(record_id)}")
        return self.row_of[int(record_id)]

    def _window(self, row: int, sample_start, sample_end) -> np.ndarray:
        off, n = int(self.records["wave_offset"][row]), int(self.records["event_length"][row])
        end = n if sample_end is None else min(max(int(sample_end), 0), n)
        start = min(max(int(sample_start), 0), end)
        return self.wave_pool[off + start:off + end]

    def _values(self, row: int, mode: str, dtype: np.dtype, sample_start, sample_end, baseline=None) -> np.ndarray:
        x = self._window(row, sample_start, sample_end).astype(dtype)
        if mode == "waves":
            return x
        b = self.records["baseline"][row] if baseline is None else baseline
        x = x - np.asarray(b, dtype=dtype)
        return -x if mode == "signals" and self.positive[row] else x

    def _get(self, record_ids, mode, dtype, default, pad_to, mask, sample_start, sample_end, baseline=None):
        if np.isscalar(record_ids):
            return self._values(self._row(record_ids), mode, np.dtype(dtype or default), sample_start, sample_end, baseline)
        if baseline is not None:
            raise ValueError("baseline override is only supported for scalar signal access")
        rows = [self._row(i) for i in record_ids]
        if not rows:
            empty = np.zeros((0, 0), dtype=dtype or np.float32)
            return (empty, empty.astype(bool)) if mask else empty
        parts = [self._values(r, mode, np.dtype(dtype or default), sample_start, sample_end) for r in rows]
        longest = max(len(p) for p in parts)
        if pad_to is not None and pad_to < 0:
            raise ValueError("pad_to must be >= 0")
        if pad_to is not None and pad_to < longest:
            raise ValueError(f"pad_to ({pad_to}) < max length ({longest})")
        width = longest if pad_to is None else int(pad_to)
        values = np.zeros((len(rows), width), dtype=dtype or default)
        valid = np.zeros((len(rows), width), dtype=bool)
        for k, p in enumerate(parts):
            values[k, :len(p)] = p
            valid[k, :len(p)] = True
        return (values, valid) if mask else values

    def waves(self, record_ids, pad_to=None, mask=False, baseline_correct=False, dtype=None, sample_start=0,
              sample_end=None):
        return self._get(record_ids, "waves_baseline" if baseline_correct else "waves", dtype,
                         np.float32 if baseline_correct else self.wave_pool.dtype, pad_to, mask, sample_start, sample_end)

    def signals(self, record_ids, pad_to=None, mask=False, dtype=None, baseline=None, sample_start=0, sample_end=None):
        return self._get(record_ids, "signals", dtype, np.float32, pad_to, mask, sample_start, sample_end, baseline)

    def query_time_window(self, t_min=None, t_max=None):
        ts = self.records["timestamp"]
        lo = 0 if t_min is None else int(np.searchsorted(ts, t_min, side="left"))
        hi = len(ts) if t_max is None else int(np.searchsorted(ts, t_max, side="right"))
        return self.records[lo:hi]


def load():
    """-> (records, {"u16": pool, "f32": pool}, calls, arrays): calls is the fixture's list of
    {"pool", "method", "ids" (int or list) | "t_min"/"t_max", "kwargs"}; call k's recorded results are arrays[f"c{k}_values"]
    (+ f"c{k}_mask"), for query_time_window arrays[f"c{k}_record_id"]."""
    z = np.load(FIXTURE, allow_pickle=False)
    arrays = {k: z[k] for k in z.files}
    calls = json.loads(bytes(arrays.pop("calls_json")).decode())
    pools = {"u16": arrays.pop("wave_pool"), "f32": arrays.pop("wave_pool_f32")}
    return arrays.pop("records"), pools, calls, arrays


def call_kwargs(call) -> dict:
    kw = dict(call["kwargs"])
    if "dtype" in kw:
        kw["dtype"] = np.dtype(kw["dtype"]).type
    return kw


def run_call(view, call):
    """Apply one fixture call to a RecordsView-like object -> tuple of the arrays it returns."""
    if call["method"] == "query_time_window":
        return (np.ascontiguousarray(view.query_time_window(call["t_min"], call["t_max"])["record_id"]),)
    got = getattr(view, call["method"])(call["ids"], **call_kwargs(call))
    return got if isinstance(got, tuple) else (got,)


def expected(call, k: int, arrays) -> tuple:
    if call["method"] == "query_time_window":
        return (arrays[f"c{k}_record_id"],)
    out = (arrays[f"c{k}_values"],)
    return out + (arrays[f"c{k}_mask"],) if call["kwargs"].get("mask") else out


def assert_same_bytes(got: tuple, want: tuple, what: str) -> None:
    """Shapes, dtypes and every byte (so -0.0 differs from 0.0)."""
    assert len(got) == len(want), f"{what}: {len(got)} arrays, expected {len(want)}"
    for g, w in zip(got, want):
        assert g.shape == w.shape, f"{what}: shape {g.shape}, expected {w.shape}"
        assert g.dtype == w.dtype, f"{what}: dtype {g.dtype}, expected {w.dtype}"
        if np.ascontiguousarray(g).tobytes() != np.ascontiguousarray(w).tobytes():
            bad = np.argwhere(np.ascontiguousarray(g).view(np.uint8).reshape(g.shape + (-1,))
                              != np.ascontiguousarray(w).view(np.uint8).reshape(w.shape + (-1,)))
            first = tuple(int(i) for i in bad[0][:-1])
            raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {first}: got {g[first]!r}, expected {w[first]!r}")
