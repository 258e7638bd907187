"""Per-record plugins across several GPUs from one process: one contiguous record range per device.

Hits, basic features and width integrals depend on one record alone (the run-wide padded width of the hit pass is
passed to every shard explicitly, hit_finder.py:354-370), so a run splits into contiguous record ranges with no exchange
between devices.  Each shard's rows are the rows of its records in record order; placing the shards' tables one after
another in shard order is the reference's order (record index, then start sample) with no sort and no gather.

The plugins come here through one function, plugins/_common.py::records_route, which reads their `devices` option:
None stays on the calling thread's session, anything else takes the context's `ShardedRun` (sharded_run) and hands it
the plugin's pass.  `ShardedRun` keeps one `DeviceSession` and one long-lived worker thread per entry of `device_ids`.
Every run starts the same way (`_plan`: split, lock, and per shard its inputs, its session and its pool slice); the
three kinds of run differ in what follows:
  * run, one row per record: the caller allocates the table, every worker runs the pass into its slice of it;
  * run with `fetch`, any number of rows: every worker runs the pass, rows left on the device, and reports its count;
    the caller allocates the run's table once; every worker downloads its rows straight into its slice of it;
  * run_pool, a float32 pool (wave_pool_filtered): every worker filters its records and downloads their samples into
    the one output, and its slice stays resident for the passes that read it.
A worker's first step is always to put its shard's pool slice on its device (skipped when it is still resident) and to
take its records with wave_offset shifted to the slice.
The uploads and downloads are ctypes calls, which release the GIL: the links of different devices work at once.

The dense routes (st_waveforms / filtered_waveforms, plugins/_common.py::dense_route) are the same runs with another
answer to "what a shard puts on its device" (`_plan(rows=...)`): the rows are uniform, so shards are contiguous row
ranges balanced by row count (split_rows), cut at multiples of 8 // gcd(L, 8) rows so that r0 * L is a multiple of
POOL_ALIGN; worker k uploads `data[r0:r1]` as it is (DeviceSession.ensure_dense: a pointer offset and a row count) and
gets dense_records' rows with wave_offset shifted by r0 * L.  Residency is a per-shard tag (array, r0, r1, view) per
device buffer (_dense: uint16 rows, _dense_f32: float32 rows), under the same `is` rule as the pool slices; a pool
upload voids the dense tags of its session and a dense upload the pool tags.  filtered_waveforms is a one-row-per-record
run whose table is its output array: every shard's slice of it is noted as the content of its float32 pool.
run_hits (waveform_width, both routes) cuts a hit table by the shard the hit's record falls in (partition_hits).

This is the in-process path.  `bench.py --gpus N` keeps its multi-process route (one rank per GPU, channel shards, hit
rows gathered over RCCL) for the event-grouping chain, which needs the rows of every channel on one device.
"""

from __future__ import annotations

import math
import threading
import weakref
from concurrent.futures import ThreadPoolExecutor
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Callable, Sequence

import numpy as np

# A shard's pool slice starts on a multiple of this many samples, so every record keeps the alignment of its offset
# (the upload picks its layout routes -- span mode, padded shadow -- from it) and a shard computes what the whole run
# computes on its records.
POOL_ALIGN = 8


@dataclass(frozen=True)
class RecordShard:
    """Records [r0, r1) and the pool span [span_start, span_end) that holds their samples."""

    r0: int
    r1: int
    span_start: int
    span_end: int

    @property
    def n_records(self) -> int:
        return self.r1 - self.r0


def _columns(records: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(wave_offset, event_length), contiguous: one strided read per column (the records rows are ~100 B wide),
    everything after it on contiguous arrays."""
    if not len(records):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.ascontiguousarray(records["wave_offset"]), np.ascontiguousarray(records["event_length"])


def split_records(records: np.ndarray, n_shards: int) -> list[RecordShard]:
    """Contiguous record ranges balanced by sample count (cumulative event_length), one per shard.

    A shard's span is [min wave_offset, max(wave_offset + event_length)) over its records: exactly its slice for the
    builders' layout (offsets non-decreasing and disjoint), wider than needed for anything else (offsets out of order,
    gaps, overlaps) but always holding every sample of its records.  With fewer records than shards, or samples that
    cannot be balanced, some shards are empty (r0 == r1, span (0, 0))."""
    return _split(*_columns(records), n_shards)


def _split(offsets: np.ndarray, lengths: np.ndarray, n_shards: int) -> list[RecordShard]:
    n_shards = int(n_shards)
    if n_shards < 1:
        raise ValueError("n_shards must be >= 1")
    n = len(lengths)
    if n and int(lengths.min()) < 0:  # negative lengths hold no samples
        lengths = np.maximum(lengths, 0)
    cum = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, dtype=np.int64, out=cum[1:])
    total = int(cum[-1])
    if total > 0:
        # boundary k: the record start whose cumulative sample count is nearest to k / n_shards of the run
        target = np.arange(n_shards + 1, dtype=np.float64) * (total / n_shards)
        hi = np.clip(np.searchsorted(cum, target, side="left"), 0, n)
        lo = np.maximum(hi - 1, 0)
        bounds = np.where(np.abs(cum[lo] - target) <= np.abs(cum[hi] - target), lo, hi)
    else:  # nothing to balance: by record count
        bounds = (np.arange(n_shards + 1, dtype=np.int64) * n) // n_shards
    bounds[0], bounds[-1] = 0, n
    bounds = np.maximum.accumulate(bounds)
    shards = []
    for k in range(n_shards):
        r0, r1 = int(bounds[k]), int(bounds[k + 1])
        if r1 > r0:
            off = offsets[r0:r1].astype(np.int64, copy=False)
            s0 = int(off.min())
            s1 = int((off + lengths[r0:r1]).max())
            shards.append(RecordShard(r0, r1, s0, max(s1, s0)))
        else:
            shards.append(RecordShard(r0, r0, 0, 0))
    return shards


def dense_unit(row_length: int) -> int:
    """Rows per split unit of a dense array: the fewest rows whose samples are a multiple of POOL_ALIGN."""
    return POOL_ALIGN // math.gcd(int(row_length), POOL_ALIGN)


def split_rows(n_rows: int, row_length: int, n_shards: int) -> list[tuple[int, int]]:
    """Contiguous row ranges [r0, r1) of a dense array (uniform rows), one per shard, balanced by row count.

    Every boundary is a multiple of dense_unit(row_length) rows, so r0 * row_length is a multiple of POOL_ALIGN: row r
    of the array sits at sample (r - r0) * row_length of its shard's pool, the same offset modulo POOL_ALIGN as
    r * row_length in the whole array's, and the upload picks the same layout route for it.  The units (the last one
    may be short) are dealt floor-wise, so the shards' sizes differ by at most one unit; with fewer units than shards
    some shards are empty (r0 == r1)."""
    n_rows, n_shards = int(n_rows), int(n_shards)
    if n_shards < 1:
        raise ValueError("n_shards must be >= 1")
    unit = dense_unit(row_length)
    units = -(-n_rows // unit)
    bounds = [min((k * units) // n_shards * unit, n_rows) for k in range(n_shards + 1)]
    return list(zip(bounds[:-1], bounds[1:]))


def partition_hits(index: np.ndarray, bounds: Sequence[int]) -> list[np.ndarray]:
    """Per shard k, the positions (ascending: hit order kept) of the entries of `index` inside [bounds[k], bounds[k + 1]).
    Entries below bounds[0] or at / above bounds[-1] (a hit with no row: -1, an index out of range) go to no shard."""
    index = np.asarray(index, dtype=np.int64)
    edges = np.asarray(bounds, dtype=np.int64)
    shard = np.searchsorted(edges, index, side="right") - 1  # of equal edges (empty shards) the last one: the non-empty
    shard[(index < edges[0]) | (index >= edges[-1])] = -1
    order = np.argsort(shard, kind="stable")
    first = np.searchsorted(shard[order], np.arange(len(edges)), side="left")
    return [order[first[k]:first[k + 1]] for k in range(len(edges) - 1)]


def _copy_rows(rows: np.ndarray) -> np.ndarray:
    """A copy of a record range: one memcpy for a contiguous structured array (numpy's structured copy goes field by
    field, several times slower on the reference's records dtype)."""
    if rows.flags.c_contiguous and rows.ndim == 1 and rows.dtype.itemsize and len(rows):
        return rows.view(np.uint8).copy().view(rows.dtype)
    return rows.copy()


def _per_record(per_record: Sequence, n: int, rows) -> list:
    """`per_record` with every 1-d array of n entries cut to `rows` (a slice or a mask); scalars, 0-d arrays and None go
    through as they are."""
    return [a[rows] if isinstance(a, np.ndarray) and a.ndim == 1 and len(a) == n else a for a in per_record]


def _shard_inputs(records: np.ndarray | None, sh: RecordShard, per_record: Sequence) -> tuple:
    """(slice start, records of the shard with wave_offset shifted to the slice, its per-record arguments).  A run that
    reads no records table (waveform_width on dense rows) passes None and gets None."""
    lo = sh.span_start - sh.span_start % POOL_ALIGN
    if records is None:
        return lo, None, list(per_record)
    rec = _copy_rows(records[sh.r0:sh.r1])
    if lo:
        rec["wave_offset"] -= lo
    return lo, rec, _per_record(per_record, len(records), slice(sh.r0, sh.r1))


def _own_samples(records: np.ndarray, shards: Sequence[RecordShard]) -> tuple[list, tuple, bool]:
    """([(starts, ends)] per shard: the samples of its records as sorted disjoint runs [start, end), adjacent records
    joined; (starts, ends) of every shard's runs merged and sorted by start; whether a sample belongs to records of two
    shards -- if none does the merged runs are disjoint, so sorted by end as well)."""
    off, ln = (c.astype(np.int64, copy=False) for c in _columns(records))
    runs = []
    for sh in shards:
        o, n_k = off[sh.r0:sh.r1], ln[sh.r0:sh.r1]
        has = n_k > 0
        if not has.all():
            o, n_k = o[has], n_k[has]
        if len(o) > 1 and np.any(o[1:] < o[:-1]):
            order = np.argsort(o, kind="stable")
            o, n_k = o[order], n_k[order]
        e = o + n_k
        if len(o) == 0:
            runs.append((o, e))
            continue
        reach = np.maximum.accumulate(e)
        first = np.flatnonzero(np.concatenate(([True], o[1:] > reach[:-1])))  # a run starts after a gap
        runs.append((o[first], np.maximum.reduceat(e, first)))
    starts = np.concatenate([r[0] for r in runs]) if runs else np.zeros(0, np.int64)
    ends = np.concatenate([r[1] for r in runs]) if runs else np.zeros(0, np.int64)
    order = np.argsort(starts, kind="stable")
    starts, ends = starts[order], ends[order]
    shared = len(starts) > 1 and bool(np.any(starts[1:] < np.maximum.accumulate(ends)[:-1]))
    return runs, (starts, ends), shared


class ShardError(RuntimeError):
    """A shard's worker raised; `device_id` and `shard` name where, `__cause__` is the worker's exception."""

    def __init__(self, message: str, device_id: int, shard: int):
        super().__init__(message)
        self.device_id = device_id
        self.shard = shard


def _default_factory(device_id: int):
    from .device import DeviceSession

    return DeviceSession(device_id)


class ShardedRun:
    """One session and one worker thread per entry of `device_ids` (an id may repeat: several sessions on one GPU).

    Every call to a session happens on its worker thread.  Residency follows `DeviceSession.ensure_pool`: a shard's
    upload is skipped while its session still holds the slice of the very same pool array OBJECT (strong reference,
    compared with `is`) with the same bounds."""

    def __init__(self, device_ids: Sequence[int], session_factory: Callable | None = None):
        ids = [int(d) for d in device_ids]
        if not ids:
            raise ValueError("ShardedRun needs at least one device id")
        self.device_ids = ids
        self._factory = session_factory or _default_factory
        self.sessions: list = []
        self._workers = [ThreadPoolExecutor(max_workers=1, thread_name_prefix=f"wfa-shard{k}") for k in range(len(ids))]
        self._resident: list[tuple | None] = [None] * len(ids)  # (pool, lo, hi, view) the session holds
        self._filtered: list[tuple | None] = [None] * len(ids)  # (output, lo, hi, view) its filters wrote (run_pool)
        # (dense array, r0, r1, view) whose `wave` rows the session holds, one tag per device buffer as in DeviceSession
        self._dense: list[tuple | None] = [None] * len(ids)      # int16 / uint16 rows: the device uint16 pool
        self._dense_f32: list[tuple | None] = [None] * len(ids)  # float32 rows: the device float32 pool
        self._lock = threading.Lock()  # one run at a time: the sessions hold one run's rows
        self.closed = False
        futures = [w.submit(self._factory, d) for w, d in zip(self._workers, ids)]
        made, error = [], None
        for fut in futures:
            try:
                made.append(fut.result())
            except BaseException as exc:  # noqa: BLE001  (re-raised below once every worker is done)
                made.append(None)
                error = error or exc
        self.sessions = made
        if error is not None:
            self.close()
            raise error

    @property
    def n_shards(self) -> int:
        return len(self.device_ids)

    # -- workers ---------------------------------------------------------------------------------------------------
    def _on_all(self, fn: Callable[[int], object], shards: Sequence[int] | None = None) -> list:
        """fn(k) on worker k for every k; every worker finishes before a failure is reported.  A failed shard's session
        is closed and replaced (its device state is not trusted, as DevicePool.drop_session), then the first failure
        (in shard order) is raised with its device id."""
        ks = range(self.n_shards) if shards is None else shards
        futures = {k: self._workers[k].submit(fn, k) for k in ks}
        results, failed = [None] * self.n_shards, []
        for k, fut in futures.items():
            try:
                results[k] = fut.result()
            except BaseException as exc:  # noqa: BLE001  (re-raised below once every worker is done)
                failed.append((k, exc))
        if not failed:
            return results
        for k, _exc in failed:
            self._replace_session(k)
        k, exc = failed[0]
        raise ShardError(f"shard {k} on device {self.device_ids[k]} failed: {type(exc).__name__}: {exc}",
                         self.device_ids[k], k) from exc

    def _drop_tags(self, k: int) -> None:
        """Session k holds nothing this run knows of (replaced, closed, or an upload has just replaced its pools)."""
        self._resident[k] = self._filtered[k] = self._dense[k] = self._dense_f32[k] = None

    def _replace_session(self, k: int) -> None:
        self._drop_tags(k)
        old = self.sessions[k]
        negative_row = getattr(old, "first_negative_row", -1)

        def swap():
            try:
                old.close()
            except Exception:  # noqa: BLE001  (a broken context may not close cleanly; the new one is what counts)
                pass
            return self._factory(self.device_ids[k])

        try:
            self.sessions[k] = self._workers[k].submit(swap).result()
        except BaseException:  # noqa: BLE001  (no new context on that device: this run is done, the next call starts anew)
            self.sessions[k] = None
            self.close()
            return
        if negative_row >= 0:  # the dense upload that failed: what it found stays readable where the caller looks for it
            self.sessions[k].first_negative_row = negative_row

    def _ensure_slice(self, k: int, sess, pool: np.ndarray, lo: int, hi: int, cacheable: bool) -> None:
        f32 = self._filtered[k]
        if cacheable and f32 is not None and f32[0] is pool and f32[1] == lo and f32[2] == hi \
                and sess.holds_filtered(f32[3]):
            return  # the slice of a run_pool output its own filters left on the device: the float32 source reads it
        tag = self._resident[k]
        if cacheable and tag is not None and tag[0] is pool and tag[1] == lo and tag[2] == hi:
            view = tag[3]  # the object the session remembers: its own `is` test decides
        else:
            view = pool[lo:hi]
        if sess.ensure_pool(view, cacheable=cacheable):
            self._drop_tags(k)  # a pool upload replaces whatever else was resident, dense rows included
        self._resident[k] = (pool, lo, hi, view) if cacheable else None

    def _ensure_rows(self, k: int, sess, data: np.ndarray, r0: int, r1: int, what: str) -> None:
        """Rows [r0, r1) of the dense array `data` on session k: `data[r0:r1]` goes up as it is
        (DeviceSession.ensure_dense) unless the session still holds that very view of that very array."""
        tags = self._dense_f32 if data.dtype["wave"].base == np.float32 else self._dense
        tag = tags[k]
        if tag is not None and tag[0] is data and tag[1] == r0 and tag[2] == r1:
            view = tag[3]  # the object the session remembers: its own `is` test decides
        else:
            view = data[r0:r1]
        try:
            uploaded = sess.ensure_dense(view, what=what)
        except ValueError:
            if getattr(sess, "first_negative_row", -1) >= 0:
                sess.first_negative_row += r0  # the row of the whole array; the lowest failing shard's is its first
            raise
        if uploaded:
            self._drop_tags(k)  # a dense upload replaces whatever else was resident
        tags[k] = (data, r0, r1, view)

    # -- a run -----------------------------------------------------------------------------------------------------
    @contextmanager
    def _plan(self, records: np.ndarray | None, pool: np.ndarray, per_record: Sequence, cacheable: bool,
              rows: tuple[str, int, int] | None = None):
        """What every run starts with, the run's lock held inside: (shards, the shards that have records, ready, the
        run's longest event_length).  ready(k), on worker k, puts the shard's samples on its device and returns
        (session, shard, slice start, records_k, per-record arguments of shard k).

        rows=None: `pool` is the flat pool the records point into; shards are record ranges balanced by sample count and
        a shard's samples are its pool slice.  rows=(name, row length L, row count): a dense run, record r is row r;
        shards are row ranges (split_rows) and a shard's samples are the rows `pool[r0:r1]` of the dense structured array
        itself (resident under _ensure_rows), or, when `pool` is the flat row-major copy of an array that cannot go up
        as it is, the slice [r0 L, r1 L) of that copy, uploaded every time.  The run's width is then L."""
        if self.closed:
            raise RuntimeError("ShardedRun is closed")
        if rows is None:
            offsets, lengths = _columns(records)
            shards = _split(offsets, lengths, self.n_shards)
            width = int(lengths.max(initial=0))

            def put(k, sess, sh, lo):
                self._ensure_slice(k, sess, pool, lo, sh.span_end, cacheable)
        else:
            what, width, n_rows = rows
            shards = [RecordShard(r0, r1, r0 * width, r1 * width) if r1 > r0 else RecordShard(r0, r0, 0, 0)
                      for r0, r1 in split_rows(n_rows, width, self.n_shards)]

            def put(k, sess, sh, lo):
                if pool.dtype.names is not None:
                    self._ensure_rows(k, sess, pool, sh.r0, sh.r1, what)
                else:
                    self._ensure_slice(k, sess, pool, lo, sh.span_end, False)

        def ready(k):
            sh, sess = shards[k], self.sessions[k]
            lo, rec, extra = _shard_inputs(records, sh, per_record)
            put(k, sess, sh, lo)
            return sess, sh, lo, rec, extra

        with self._lock:
            yield shards, [k for k, sh in enumerate(shards) if sh.n_records > 0], ready, width

    def run(self, records: np.ndarray, pool: np.ndarray, row_dtype, task: Callable, *, fetch: Callable | None = None,
            per_record: Sequence = (), cacheable: bool = True, record_index_field: str | None = None,
            width_arg: str | None = None, rows: tuple[str, int, int] | None = None, out: np.ndarray | None = None,
            note_out: bool | None = None) -> np.ndarray:
        """The run's table, shards placed one after another in shard order.

        task(sess, records_k, *per_record_k, out=...) runs on worker k after the shard's pool slice is resident, with
        records_k = records[r0:r1] (wave_offset shifted to the slice) and every per-record array of `per_record` sliced
        the same way (scalars, 0-d arrays and None go through as they are).
          * fetch=None: one row per record.  `out` is the shard's slice of the table; task writes it.
            record_index_field: a field that holds the record index; the shard's r0 is added to it.
            out: the table to write into instead of a new zeroed one (filtered_waveforms: the rows it has filled but for
            `wave`).  note_out (filtered_waveforms): the pass leaves the `wave` rows it wrote into its slice of `out` in
            the session's float32 pool; True tags that slice as resident (note_dense on the view, keyed on `out`, r0,
            r1), False (a layout that could not be uploaded as it is) forgets what the session held.
          * fetch given: task(..., out=None) runs the pass and returns the shard's row count, rows left on the device;
            then fetch(sess, out_k) downloads them into the shard's slice of the table.
            width_arg: a keyword under which task also gets the run's longest event_length (the hit pass pads every
            shard to the run's width, hit_finder.py:354-370, not to the shard's own).
        rows: a dense run (see _plan); `pool` is then the dense array, or the flat copy of its rows.
        A failure raises ShardError and returns no table."""
        row_dtype = np.dtype(row_dtype)
        with self._plan(records, pool, per_record, cacheable, rows) as (_shards, busy, ready, width):
            if fetch is None:
                if out is None:
                    out = np.zeros(len(records), dtype=row_dtype)

                def one_pass(k):
                    sess, sh, _lo, rec, extra = ready(k)
                    part = out[sh.r0:sh.r1]
                    task(sess, rec, *extra, out=part)
                    if record_index_field is not None and sh.r0:
                        part[record_index_field] += sh.r0
                    if note_out:
                        sess.note_dense(part)
                        self._filtered[k] = None  # (the filters overwrote the device float32 pool)
                        self._dense_f32[k] = (out, sh.r0, sh.r1, part)
                    elif note_out is not None:
                        sess.forget_resident()
                        self._drop_tags(k)

                self._on_all(one_pass, busy)
                return out

            run_width = {width_arg: width} if width_arg else {}

            def count(k):
                sess, _sh, _lo, rec, extra = ready(k)
                return int(task(sess, rec, *extra, out=None, **run_width))

            counts = self._on_all(count, busy)
            rows = np.array([c or 0 for c in counts], dtype=np.int64)
            first = np.zeros(self.n_shards + 1, dtype=np.int64)
            np.cumsum(rows, out=first[1:])
            out = np.empty(int(first[-1]), dtype=row_dtype)
            self._on_all(lambda k: fetch(self.sessions[k], out[first[k]:first[k + 1]]),
                         [k for k in busy if rows[k] > 0])
            return out

    def run_hits(self, index: np.ndarray, task: Callable, records: np.ndarray | None, pool: np.ndarray, *,
                 cacheable: bool = True, rows: tuple[str, int, int] | None = None) -> list[tuple[np.ndarray, object]]:
        """Per-hit work on the shard that holds the hit's record (waveform_width): [(positions in the hit table, what
        task returned)] for every shard that has hits.

        index: per hit, the record (row) it points at.  The hit table is cut by the shard that record falls in
        (partition_hits over the shards of _plan: a hit with a negative or out-of-range index goes to no shard, the
        caller marks it invalid).  task(sess, records_k, positions, index - r0, r1 - r0) runs on worker k after the
        shard's samples are resident; positions are ascending, so a shard sees its hits in hit order.  A shard with no hits
        uploads nothing.  records=None with `rows`: the pass reads rows, no records table (the dense route)."""
        with self._plan(records, pool, (), cacheable, rows) as (shards, _busy, ready, _width):
            index = np.asarray(index, dtype=np.int64)
            picks = partition_hits(index, [sh.r0 for sh in shards] + [shards[-1].r1])
            busy = [k for k, mine in enumerate(picks) if len(mine)]

            def one(k):
                sess, sh, _lo, rec, _extra = ready(k)
                return task(sess, rec, picks[k], index[picks[k]] - sh.r0, sh.n_records)

            results = self._on_all(one, busy)
            return [(picks[k], results[k]) for k in busy]

    def run_pool(self, records: np.ndarray, pool: np.ndarray, task: Callable, *, per_record: Sequence = (),
                 cacheable: bool = True) -> np.ndarray:
        """A float32 array of len(pool) samples (wave_pool_filtered): 0.0 except the samples of the records, each written
        by the shard that holds its record.

        task(sess, records_k, *per_record_k) runs on worker k after the shard's pool slice is resident (records and
        per-record arrays sliced and shifted as in run()) and leaves the shard's float32 pool on the device, 0.0 outside
        its records.  The worker then downloads the samples of its OWN records into the output: its whole span in one
        copy when no other shard's record lies inside it (the builders' layout), else one copy per run of its records'
        samples.  A sample two shards' records share (hand-made layouts: overlapping records) has one value for the
        order the writes happen in, so when any sample is shared the whole call runs on the first shard alone, pool
        and records as they are -- what one device computes.  Records that hold no sample and point outside the pool
        are left out of the run: they write nothing, and their offsets would widen a shard's span.

        With cacheable, each shard's float32 slice stays tagged as resident, keyed on the returned array object and the
        slice bounds: a later run() on that array with the same records (same split) uploads nothing.  Of that slice the
        device holds the samples of the shard's own records (0.0 elsewhere); a per-record pass reads no others.
        A failure raises ShardError and returns no table."""
        off, ln = _columns(records)
        idle = (ln <= 0) & ((off < 0) | (off > len(pool)))
        if np.any(idle):
            records, per_record = records[~idle], _per_record(per_record, len(records), ~idle)
        out = np.zeros(len(pool), dtype=np.float32)
        with self._plan(records, pool, per_record, cacheable) as (shards, busy, ready, _width):
            runs, (starts, ends), shared = _own_samples(records, shards)
            self._filtered = [None] * self.n_shards

            def keep(k, sess, lo, hi):
                if cacheable:
                    view = out[lo:hi]
                    sess.note_filtered(view)
                    self._filtered[k] = (out, lo, hi, view)
                self._dense_f32[k] = None  # (the filters overwrote the device float32 pool)

            def alone(k):
                sess = self.sessions[k]
                self._ensure_slice(k, sess, pool, 0, len(pool), cacheable)
                task(sess, records, *per_record)
                sess.download_filtered(out)
                keep(k, sess, 0, len(pool))

            def one(k):
                sess, sh, lo, rec, extra = ready(k)
                task(sess, rec, *extra)
                own0, own1 = runs[k]
                inside = int(np.searchsorted(starts, sh.span_end, "left") - np.searchsorted(ends, sh.span_start, "right"))
                if inside == len(own0):  # nothing of another shard in the span: its gaps are 0.0 on the device too
                    sess.download_filtered(out[sh.span_start:sh.span_end], start=sh.span_start - lo)
                else:
                    for a, b in zip(own0.tolist(), own1.tolist()):
                        sess.download_filtered(out[a:b], start=a - lo)
                keep(k, sess, lo, sh.span_end)

            if shared:
                self._on_all(alone, [0])
            else:
                self._on_all(one, busy)
            return out

    # -- lifetime --------------------------------------------------------------------------------------------------
    def release_scratch(self) -> None:
        """DeviceSession.release_scratch on every session (the plugins' cleanup hook)."""
        self._on_all(lambda k: self.sessions[k].release_scratch())

    def close(self) -> None:
        """Close every session and stop the workers."""
        if self.closed:
            return
        self.closed = True
        for k in range(self.n_shards):
            self._drop_tags(k)
        for k, w in enumerate(self._workers):
            s = self.sessions[k] if k < len(self.sessions) else None
            try:
                if s is not None:
                    w.submit(s.close).result()
            finally:
                w.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def resolve_devices(devices) -> tuple[int, ...] | None:
    """The `devices` plugin option: None (single-device route), "all" (every visible device) or a list of ids."""
    if devices is None:
        return None
    if isinstance(devices, str):
        if devices.strip().lower() != "all":
            raise ValueError(f"devices must be None, 'all' or a list of device ids, got {devices!r}")
        from .device import device_count

        n = device_count()
        if n < 1:
            raise RuntimeError("devices='all': no HIP device visible")
        return tuple(range(n))
    ids = tuple(int(d) for d in devices)
    if not ids:
        raise ValueError("devices must name at least one device")
    return ids


_runs: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()  # context -> {device tuple: ShardedRun}
_shared: dict = {}  # the same for contexts that take no weak reference
_runs_lock = threading.Lock()


def _cache(context, create: bool) -> dict | None:
    try:
        cache = _runs.get(context)
        if cache is None and create:
            cache = _runs[context] = {}
        return cache
    except TypeError:
        return _shared


def sharded_run(context, devices) -> ShardedRun:
    """The ShardedRun of (context, device tuple), created on first use.  A context may name the session factory its
    sessions come from (`context.wfa_session_factory`, as `context.wfa_device_pool` names the single-device pool)."""
    ids = resolve_devices(devices)
    with _runs_lock:
        cache = _cache(context, create=True)
        run = cache.get(ids)
        if run is None or run.closed:
            run = cache[ids] = ShardedRun(ids, session_factory=getattr(context, "wfa_session_factory", None))
    return run


def peek_sharded_runs(context) -> list[ShardedRun]:
    """Every live ShardedRun of `context` (never creates one)."""
    with _runs_lock:
        cache = _cache(context, create=False) or {}
        return [r for r in cache.values() if not r.closed]


def close_sharded_runs(context) -> None:
    """Close and forget every ShardedRun of `context`."""
    with _runs_lock:
        cache = _cache(context, create=False) or {}
        runs = list(cache.values())
        cache.clear()
    for r in runs:
        r.close()


__all__ = ["POOL_ALIGN", "RecordShard", "ShardError", "ShardedRun", "split_records", "dense_unit", "split_rows",
           "partition_hits", "resolve_devices", "sharded_run", "peek_sharded_runs", "close_sharded_runs"]
