"""HipRecordsView: the reference's RecordsView (core/data/records_view.py:16-400) over a pool that stays in HBM.

`waves` / `signals` return what the reference returns, byte for byte: a scalar record_id gives the 1-D window of that
record, an iterable gives the zero-padded matrix (and its bool mask).  The reference fills the matrix with a Python loop
over the records; here one kernel gathers it from the resident pool (DeviceSession.view_gather) and the batches come
down through the pinned staging ring.  `query_time_window` and the record_id lookup are host code.

Output dtypes: float32 and float64 in every mode, and the pool's own dtype for plain `waves`.  Any other dtype raises
ValueError (the reference would cast the baseline to that dtype first, e.g. truncate it for integers; there is no CPU
fallback in this project).
"""

from __future__ import annotations

from collections.abc import Iterable
from typing import Any

import numpy as np

from .device import REQUIRED_RECORD_FIELDS, DeviceSession, default_pool

_POOL_DTYPES = (np.dtype(np.uint16), np.dtype(np.float32))
_FLOAT_DTYPES = (np.dtype(np.float32), np.dtype(np.float64))


class HipRecordsView:
    """Read-only access to records + wave_pool; drop-in for the reference's RecordsView.

    session: the DeviceSession to use; None takes the calling thread's session of `device_pool` (None: default_pool()),
    as the plugins do.  The pool is uploaded only if the session does not hold this very array object already (a
    records-route plugin or HipRecordsPlugin leaves it resident); a float32 `wave_pool` (wave_pool_filtered) goes to the
    session's float32 pool.  The records table is uploaded at the first call and again only after another caller
    replaced the session's table or pool."""

    def __init__(self, records: np.ndarray, wave_pool: np.ndarray, session: DeviceSession | None = None, *,
                 device_pool: Any = None):
        if not isinstance(records, np.ndarray) or records.dtype.names is None:
            raise ValueError("records must be a structured array")
        missing = [name for name in REQUIRED_RECORD_FIELDS if name not in records.dtype.names]
        if missing:
            raise ValueError(f"records missing required fields: {missing}")
        if not isinstance(wave_pool, np.ndarray) or wave_pool.ndim != 1:
            raise ValueError("wave_pool must be a 1-D numpy array")
        if wave_pool.dtype not in _POOL_DTYPES:
            raise ValueError(f"wave_pool dtype must be uint16 or float32, got {wave_pool.dtype}")

        self.records = records
        self.wave_pool = wave_pool
        self._session = session
        self._device_pool = device_pool
        self.batch_bytes = 256 << 20  # device batch of a matrix on its way out (two such buffers; wfa_view_gather)
        self._record_ids = records["record_id"].astype(np.int64, copy=False)
        self._wave_offsets = records["wave_offset"].astype(np.int64, copy=False)
        self._event_lengths = records["event_length"].astype(np.int64, copy=False)
        self._timestamps = records["timestamp"]
        self._validate_wave_bounds()
        # record_id -> row: one stable argsort here, one searchsorted per request
        self._id_order = np.argsort(self._record_ids, kind="stable")
        self._ids_sorted = self._record_ids[self._id_order]

    def __len__(self) -> int:
        return len(self.records)

    def _validate_wave_bounds(self) -> None:
        if len(self.records) == 0:
            return
        if np.any(self._wave_offsets < 0):
            raise ValueError("records contain negative wave_offset values")
        if np.any(self._event_lengths < 0):
            raise ValueError("records contain negative event_length values")
        if np.any(self._wave_offsets + self._event_lengths > len(self.wave_pool)):
            raise ValueError("records reference samples outside wave_pool bounds")

    # -- host side: ids, windows, dtypes ---------------------------------------------------------------------------
    def _resolve_record_indices(self, record_ids) -> np.ndarray:
        ids = np.asarray(list(record_ids) if not isinstance(record_ids, np.ndarray) else record_ids, dtype=np.int64).ravel()
        if ids.size == 0:
            return np.zeros(0, dtype=np.int64)
        n = len(self._ids_sorted)
        pos = np.searchsorted(self._ids_sorted, ids, side="left")
        found = pos < n
        found[found] = self._ids_sorted[pos[found]] == ids[found]
        if not found.all():
            raise KeyError(f"Unknown record_id: {int(ids[np.flatnonzero(~found)[0]])}")
        return self._id_order[pos]

    def _window_lengths(self, indices: np.ndarray, sample_start: int = 0, sample_end: int | None = None) -> np.ndarray:
        lengths = self._event_lengths[indices]
        ends = lengths if sample_end is None else np.clip(int(sample_end), 0, lengths)
        starts = np.minimum(np.clip(int(sample_start), 0, lengths), ends)
        return (ends - starts).astype(np.int64, copy=False)

    @staticmethod
    def _pad_len(lengths: np.ndarray, pad_to: int | None) -> int:
        max_len = int(lengths.max()) if lengths.size else 0
        if pad_to is None:
            return max_len
        if pad_to < 0:
            raise ValueError("pad_to must be >= 0")
        if pad_to < max_len:
            raise ValueError(f"pad_to ({pad_to}) < max length ({max_len})")
        return int(pad_to)

    def _out_dtype(self, dtype, default, plain_waves: bool) -> np.dtype:
        out = np.dtype(default if dtype is None else dtype)
        if out in _FLOAT_DTYPES or (plain_waves and out == self.wave_pool.dtype):
            return out
        allowed = "float32, float64" + (f" or {self.wave_pool.dtype}" if plain_waves else "")
        raise ValueError(f"unsupported dtype {out} for HipRecordsView: use {allowed}")

    # -- device side -----------------------------------------------------------------------------------------------
    def _resident_session(self) -> DeviceSession:
        """The session with this view's pool and records resident: uploads only what it does not hold (`is` tests)."""
        sess = self._session
        if sess is None:
            sess = (self._device_pool or default_pool()).session()
        pool = self.wave_pool
        if pool.dtype != np.float32 or sess.holds_pool(pool):
            uploaded = sess.ensure_pool(pool)
        elif sess.holds_filtered(pool) or sess.n_samples == pool.size:
            uploaded = sess.ensure_filtered_pool(pool)  # the float32 twin of the resident pool (wave_pool_filtered)
        else:
            uploaded = sess.ensure_pool(pool)  # a float32 pool on its own
        if uploaded or not sess.holds_records(self):
            sess.upload_records(self.records)
            sess.note_records(self)
        return sess

    def _gather(self, indices: np.ndarray, mode: str, out_dtype: np.dtype, pad_len: int, mask: bool,
                sample_start: int, sample_end: int | None, baseline_override=None):
        sess = self._resident_session()
        got = sess.view_gather(indices, mode=mode, source="f32" if self.wave_pool.dtype == np.float32 else "u16",
                               out_dtype=out_dtype, pad_len=pad_len, sample_start=sample_start, sample_end=sample_end,
                               mask=mask, baseline_override=baseline_override, batch_bytes=self.batch_bytes)
        if mask:
            return got[0], got[1].view(np.bool_)
        return got

    def _many(self, record_ids, mode: str, out_dtype: np.dtype, empty_dtype, pad_to, mask, sample_start, sample_end):
        indices = self._resolve_record_indices(record_ids)
        if indices.size == 0:
            empty = np.zeros((0, 0), dtype=empty_dtype)
            return (empty, empty.astype(bool)) if mask else empty
        lengths = self._window_lengths(indices, sample_start=sample_start, sample_end=sample_end)
        pad_len = self._pad_len(lengths, pad_to)
        return self._gather(indices, mode, out_dtype, pad_len, bool(mask), sample_start, sample_end)

    def _one(self, record_id: int, mode: str, out_dtype: np.dtype, sample_start, sample_end, baseline=None) -> np.ndarray:
        indices = self._resolve_record_indices([int(record_id)])
        n = int(self._window_lengths(indices, sample_start=sample_start, sample_end=sample_end)[0])
        override = None if baseline is None else np.asarray([baseline], dtype=np.float64)
        return self._gather(indices, mode, out_dtype, n, False, sample_start, sample_end, override)[0]

    # -- the reference's interface -----------------------------------------------------------------------------------
    def waves(self, record_ids: int | Iterable[int] | np.ndarray, pad_to: int | None = None, mask: bool = False,
              baseline_correct: bool = False, dtype: np.dtype | None = None, sample_start: int = 0,
              sample_end: int | None = None) -> np.ndarray | tuple[np.ndarray, np.ndarray]:
        """records_view.py:332-358.  dtype: None (the pool's dtype; float32 with baseline_correct), float32, float64, or
        the pool's dtype when baseline_correct is False; anything else raises ValueError."""
        mode = "waves_baseline" if baseline_correct else "waves"
        out_dtype = self._out_dtype(dtype, np.float32 if baseline_correct else self.wave_pool.dtype, not baseline_correct)
        if np.isscalar(record_ids):
            return self._one(int(record_ids), mode, out_dtype, sample_start, sample_end)
        return self._many(record_ids, mode, out_dtype, dtype or np.float32, pad_to, mask, sample_start, sample_end)

    def signals(self, record_ids: int | Iterable[int] | np.ndarray, pad_to: int | None = None, mask: bool = False,
                dtype: np.dtype | None = None, baseline: float | None = None, sample_start: int = 0,
                sample_end: int | None = None) -> np.ndarray | tuple[np.ndarray, np.ndarray]:
        """records_view.py:360-385: baseline-subtracted, negative-going pulses.  dtype: None (float32), float32 or
        float64; anything else raises ValueError."""
        out_dtype = self._out_dtype(dtype, np.float32, False)
        if np.isscalar(record_ids):
            return self._one(int(record_ids), "signals", out_dtype, sample_start, sample_end, baseline=baseline)
        if baseline is not None:
            raise ValueError("baseline override is only supported for scalar signal access")
        return self._many(record_ids, "signals", out_dtype, dtype or np.float32, pad_to, mask, sample_start, sample_end)

    def query_time_window(self, t_min: int | None = None, t_max: int | None = None) -> np.ndarray:
        timestamps = self._timestamps
        start = 0 if t_min is None else int(np.searchsorted(timestamps, t_min, side="left"))
        end = len(timestamps) if t_max is None else int(np.searchsorted(timestamps, t_max, side="right"))
        return self.records[start:end]


def hip_records_view(source: Any, run_id: str, records_name: str = "records",
                     wave_pool_name: str = "wave_pool") -> HipRecordsView:
    """HipRecordsView over the `records_name` / `wave_pool_name` outputs of a Context-like source (the reference's
    records_view factory); the view works on the calling thread's session of `source.wfa_device_pool` (else the
    default pool), where the records-route plugins leave the pool resident."""
    records = source.get_data(run_id, records_name)
    wave_pool = source.get_data(run_id, wave_pool_name)
    if not isinstance(records, np.ndarray):
        raise ValueError(f"records_view requires formal '{records_name}' plugin output")
    if not isinstance(wave_pool, np.ndarray):
        raise ValueError(f"records_view requires formal '{wave_pool_name}' plugin output")
    return HipRecordsView(records, wave_pool, device_pool=getattr(source, "wfa_device_pool", None))
