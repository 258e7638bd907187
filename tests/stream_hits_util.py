"""Inputs and expectations for the streaming hit pipeline (waveformanalysis_amd/streaming.py: HipThresholdHitStream).

The reference evaluates hit windows on a matrix padded to the longest record of the RUN (hit_finder.py:364,370); the
padding of a short record carries signal = +-baseline, so a hit that ends within `right_extension` of a short record's
end takes its position, height, integral, rise / fall time and timestamp from the padding.  The expectation throughout
is therefore the oracle over the whole run (`want`), never over a chunk.  Runs:

  ragged    600 records of 40..120 samples back to back, one of 200 samples every 150 records, a few of 0, 1 and 7
            samples; dips on the last samples of every third record.  Chunks of 50 or 100 records that hold no
            200-sample record are narrower than the run, chunks of 150 never are.
  mixed     four time segments (uniform 64, uniform 88, ragged 40..64, uniform 24) in one pool: every layout route of
            the fused pass among the chunks of one run, the run's width 88 above most chunks' own.
  shuffled  the ragged records, their samples packed per channel with 5 garbage samples between records: offsets are
            not monotone in time and a chunk's slice of the pool holds other chunks' samples and gaps.
  sparse    blocks of records without any hit between blocks with two hits per record.

`OracleSession` is a device double that answers a queued pass with the oracle's rows for what was uploaded, at the width
that reached `hits_enqueue`: the driver's host logic runs end to end without a GPU, its mistakes included."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

from oracle import wfa_oracle as O
from tests import hit_rows_util as H
from tests.bench_stub import Session
from waveformanalysis_amd import _lib
from waveformanalysis_amd.chunk import Chunk
from waveformanalysis_amd.dtypes import RECORDS_DTYPE, THRESHOLD_HIT_DTYPE
from waveformanalysis_amd.streaming import records_to_chunks

THRESHOLD, LE, RE = 10.0, 2, 2
SG = (11, 2)
BASELINE = 8000
DIP = 300
GARBAGE = 12345
SEGMENT_GAP_PS = 2 * 10**13
RUN_NAMES = ("ragged", "mixed", "shuffled", "sparse")


@dataclasses.dataclass(eq=False)
class Run:
    name: str
    records: np.ndarray
    pool: np.ndarray
    chunk_sizes: tuple          # the chunk_size values compute() is driven with

    @functools.cached_property
    def width(self) -> int:
        return int(self.records["event_length"].max())

    @functools.cached_property
    def filtered(self) -> np.ndarray:
        out = O.filter_wave_pool(self.records, self.pool, sg_window_size=SG[0], sg_poly_order=SG[1])
        out.setflags(write=False)
        return out

    def source(self, use_filtered: bool) -> np.ndarray:
        return self.filtered if use_filtered else self.pool

    @functools.cache
    def want(self, use_filtered: bool) -> np.ndarray:
        """The run-wide oracle: every window on the matrix padded to the run's longest record."""
        rows = O.threshold_hits(self.records, self.source(use_filtered), threshold=THRESHOLD, left_extension=LE,
                                right_extension=RE)
        rows.setflags(write=False)
        return rows

    @functools.cache
    def length_of(self) -> dict:
        return dict(zip(self.records["record_id"].tolist(), self.records["event_length"].tolist()))

    def row_lengths(self, rows: np.ndarray) -> np.ndarray:
        """event_length of the record of every hit row."""
        lut = self.length_of()
        return np.array([lut[int(r)] for r in rows["record_id"]], dtype=np.int64)

    def in_padding(self, rows: np.ndarray) -> np.ndarray:
        return rows["position"] >= self.row_lengths(rows)

    def segments(self) -> list:
        """The records of every time segment (breaks of more than 10^13 ps), as the driver cuts them."""
        ts = self.records["timestamp"].astype(np.int64)
        cuts = np.flatnonzero(np.diff(ts) > 10**13) + 1
        return np.split(self.records, cuts)

    def chunks(self, chunk_size: int) -> list:
        """Ready-made chunks: what HipThresholdHitStream._data_to_chunks yields for this chunk_size."""
        out = []
        for seg_id, seg in enumerate(self.segments()):
            for ch in records_to_chunks(seg, chunk_size, "run"):
                ch.metadata["segment_id"] = seg_id
                out.append(ch)
        return out

    def per_chunk_oracle(self, chunk_size: int, use_filtered: bool = False) -> np.ndarray:
        """What a driver gives that pads every chunk to its own longest record."""
        parts = [O.threshold_hits(ch.data, self.source(use_filtered), threshold=THRESHOLD, left_extension=LE,
                                  right_extension=RE) for ch in self.chunks(chunk_size)]
        return np.concatenate(parts)


def differing_rows(a: np.ndarray, b: np.ndarray) -> dict:
    """{field: indices of the rows that differ} of two tables of equal length."""
    assert len(a) == len(b), (len(a), len(b))
    out = {}
    for name in a.dtype.names:
        bad = np.flatnonzero(a[name] != b[name])
        if len(bad):
            out[name] = bad
    return out


def empty_chunk_between(before: Chunk, after: Chunk) -> Chunk:
    """A Chunk of zero records that covers the time between two chunks."""
    start = min(before.end, after.start)
    return Chunk(before.data[:0], start, max(start, after.start), run_id="run", data_type="records",
                 data_kind="records", time_field="timestamp", length_field="event_length", metadata={"first_record": -1})


def expected_end(chunk: Chunk) -> int:
    """The end of a result: the input chunk's, raised to the end of its last record (HipThresholdHitStream._collect)."""
    rec = chunk.data
    if len(rec) == 0:
        return int(chunk.end)
    endtime = rec["timestamp"].astype(np.int64) + rec["dt"].astype(np.int64) * 1000 * rec["event_length"].astype(np.int64)
    return max(int(chunk.end), int(endtime.max()) + 1)


def _outside(run: Run, chunks: list, tables: list) -> list:
    """(record_id, position) of the rows whose timestamp lies outside [start, expected end) of their chunk."""
    out = []
    for c, rows in zip(chunks, tables):
        ts = rows["timestamp"]
        bad = (ts < c.start) | (ts >= expected_end(c))
        out += list(zip(rows["record_id"][bad].tolist(), rows["position"][bad].tolist()))
    return out


def check_bookkeeping(run: Run, chunks: list, outs: list, want: np.ndarray, what: str = "") -> np.ndarray:
    """Results in input order with the input chunks' bounds; every hit inside its chunk's time range, but for the rows in
    the padding that the oracle predicts outside it; record_id non-decreasing.  -> the concatenated rows."""
    assert len(outs) == len(chunks), (what, len(outs), len(chunks))
    for k, (c, o) in enumerate(zip(chunks, outs)):
        assert o.data.dtype == THRESHOLD_HIT_DTYPE, (what, k)
        assert (o.start, o.end) == (c.start, expected_end(c)), (what, k, o.start, o.end, c.start, c.end)
        assert np.isin(o.data["record_id"], c.data["record_id"]).all(), (what, k, "rows of another chunk's records")
    got = np.concatenate([o.data for o in outs]) if outs else np.zeros(0, dtype=THRESHOLD_HIT_DTYPE)
    assert np.all(np.diff(got["record_id"]) >= 0), (what, "record_id decreases")
    outside = _outside(run, chunks, [o.data for o in outs])
    chunk_of = {int(r): k for k, c in enumerate(chunks) for r in c.data["record_id"]}
    k_of_row = np.array([chunk_of[int(r)] for r in want["record_id"]], dtype=np.int64)
    predicted = _outside(run, chunks, [want[k_of_row == k] for k in range(len(chunks))])
    lut = run.length_of()
    assert all(pos >= lut[rid] for rid, pos in outside), (what, "a hit inside its record lies outside its chunk")
    assert outside == predicted, (what, outside[:5], predicted[:5])
    return got


# ---- builders -----------------------------------------------------------------------------------------------------
def _records(lengths, offsets, timestamps, positive=None) -> np.ndarray:
    n = len(lengths)
    rec = np.zeros(n, dtype=RECORDS_DTYPE)
    rec["event_length"], rec["wave_offset"] = lengths, offsets
    rec["timestamp"] = rec["time"] = timestamps
    rec["dt"] = 2
    rec["record_id"] = 1000 + np.arange(n)
    rec["board"], rec["channel"] = 0, np.arange(n) % 4
    rec["baseline"] = BASELINE + (np.arange(n) % 5) * 0.25
    rec["polarity"] = "negative"
    if positive is not None:
        rec["polarity"][positive] = "positive"
    return rec


def _wave(L, kind, rng, sign=-1):
    """Pedestal with noise of -2..2 and dips (bumps for sign=+1) of DIP counts: kind 0 on the last 4 samples, 1 on the
    first 3, 2 in the middle and on the last sample, 3 none, 4 on the first 3 and the last 4."""
    w = BASELINE + rng.integers(-2, 3, L)
    if kind in (0, 4):
        w[max(L - 4, 0):] += sign * DIP
    if kind in (1, 4):
        w[:min(3, L)] += sign * DIP
    if kind == 2 and L >= 20:
        w[L // 2 : L // 2 + 5] += sign * (DIP + 40)
        w[L - 1] += sign * DIP
    return w.astype(np.uint16)


def _freeze(run: Run) -> Run:
    run.records.setflags(write=False)
    run.pool.setflags(write=False)
    return run


N_RAGGED = 600
SHORT = {13: 0, 222: 0, 431: 0, 27: 1, 333: 1, 576: 1, 42: 7, 267: 7, 498: 7}   # record -> length (0, 1, 7 samples)


def _ragged_parts():
    rng = np.random.default_rng(20)
    n = N_RAGGED
    lengths = rng.integers(40, 121, n)
    lengths[::150] = 200
    positive = np.arange(n) % 7 == 3
    for r, L in SHORT.items():
        lengths[r] = L
    # one record per block of 50 without a 200-sample record: as long as the block's longest, its dip on the last samples
    for b in range(0, n, 50):
        if b % 150 == 0:
            continue
        r = next(r for r in range(b + 3, b + 50) if r % 3 == 0 and not positive[r] and r not in SHORT)
        lengths[r] = 120
    if int(lengths.sum()) % 8 == 0:
        lengths[n - 1] += 3
    waves = [_wave(int(L), r % 3 if r % 3 < 2 else (2 if r % 2 else 3), rng, +1 if positive[r] else -1)
             for r, L in enumerate(lengths)]
    timestamps = 10**12 + np.arange(n, dtype=np.int64) * 500_000
    return lengths, waves, timestamps, positive


@functools.cache
def ragged() -> Run:
    lengths, waves, timestamps, positive = _ragged_parts()
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1])])
    pool = np.concatenate(waves)
    assert pool.size % 8 and set((offsets % 8).tolist()) == set(range(8))
    return _freeze(Run("ragged", _records(lengths, offsets, timestamps, positive), pool, (50, 100, 150)))


@functools.cache
def shuffled() -> Run:
    lengths, waves, timestamps, positive = _ragged_parts()
    n = len(lengths)
    channel = np.arange(n) % 4
    order = np.lexsort((np.arange(n), (channel * 3) % 4))     # channels 0, 3, 2, 1; by time inside a channel
    offsets = np.zeros(n, dtype=np.int64)
    parts, at = [], 0
    for r in order:
        gap = np.full(5, GARBAGE, dtype=np.uint16)
        parts += [gap, waves[r]]
        offsets[r] = at + 5
        at += 5 + int(lengths[r])
    pool = np.concatenate(parts)
    assert np.any(np.diff(offsets) < 0)
    return _freeze(Run("shuffled", _records(lengths, offsets, timestamps, positive), pool, (50,)))


MIXED_SEGMENTS = (("L64", 150), ("L88", 130), ("ragged", 170), ("L24", 120))   # names as in test_hip_layout_routes.ROUTES


@functools.cache
def mixed() -> Run:
    rng = np.random.default_rng(21)
    lengths, waves, timestamps = [], [], []
    for k, (name, n) in enumerate(MIXED_SEGMENTS):
        seg_len = rng.integers(40, 65, n) if name == "ragged" else np.full(n, int(name[1:]))
        if name == "ragged":
            seg_len[::17] = 64
        for i, L in enumerate(seg_len):
            waves.append(_wave(int(L), (0, 1, 2, 4)[i % 4], rng))
        lengths.append(seg_len)
        timestamps.append(10**12 + k * SEGMENT_GAP_PS + np.arange(n, dtype=np.int64) * 300_000)
    lengths = np.concatenate(lengths)
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1])])
    return _freeze(Run("mixed", _records(lengths, offsets, np.concatenate(timestamps)), np.concatenate(waves), (100,)))


SPARSE_BLOCK = 60
SPARSE_PATTERN = (True, False, True, True, False, False, True, False, True)    # blocks with hits / without


@functools.cache
def sparse() -> Run:
    rng = np.random.default_rng(22)
    n = SPARSE_BLOCK * len(SPARSE_PATTERN)
    # uniform 64 (the streaming kernel, whose row launch is sized by the previous pass) up to the last three blocks
    lengths = np.where((np.arange(n) >= 6 * SPARSE_BLOCK) & (np.arange(n) % 9 == 4), 48, 64)
    waves = [_wave(int(L), 4 if SPARSE_PATTERN[r // SPARSE_BLOCK] else 3, rng) for r, L in enumerate(lengths)]
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1])])
    timestamps = 10**12 + np.arange(n, dtype=np.int64) * 300_000
    return _freeze(Run("sparse", _records(lengths, offsets, timestamps), np.concatenate(waves), (SPARSE_BLOCK,)))


def run(name: str) -> Run:
    return {"ragged": ragged, "mixed": mixed, "shuffled": shuffled, "sparse": sparse}[name]()


def sparse_chunks_with_empty() -> tuple:
    """(chunks, index of the zero-record Chunk): the sparse run's chunks with a Chunk of no records in the middle."""
    chunks = sparse().chunks(SPARSE_BLOCK)
    k = 4
    return chunks[:k] + [empty_chunk_between(chunks[k - 1], chunks[k])] + chunks[k:], k


# ---- a device double that computes -----------------------------------------------------------------------------------
class OracleSession(Session):
    """tests/bench_stub.Session whose queued pass returns the oracle's rows of the uploaded chunk at the width given to
    hits_enqueue (0: the chunk's longest record; below it: refused, as wfa_hits_enqueue does).  `log` (shared by the
    sessions of one factory) receives one dict per staged chunk."""

    def __init__(self, device_id: int = 0, log: list | None = None, uploads: list | None = None):
        super().__init__(device_id)
        self.log = [] if log is None else log
        self.uploads = [] if uploads is None else uploads      # sample count of every pool upload
        self._pool = self._rec = self._rows = None
        self._thr, self._sg = THRESHOLD, None

    def upload_pool(self, pool):
        super().upload_pool(pool)
        self.uploads.append(int(pool.size))
        self._pool = np.array(pool, copy=True)
        self._rec = None

    def upload_records(self, rec, thr):
        super().upload_records(rec, thr)
        self._rec, self._thr = rec.copy(), float(thr)

    def set_sg_plan(self, w, p):
        self._sg = (int(w), int(p))

    def hits_enqueue(self, source=_lib.SRC_SG_FUSED, baseline_window=(0, 0), left_extension=2, right_extension=2,
                     max_len=0):
        rec, pool = self._rec, self._pool
        assert rec is not None and pool is not None, "hits_enqueue before the uploads"
        longest = int(rec["event_length"].max())
        if 0 < max_len < longest:
            raise _lib.WfaError(_lib.WFA_E_INVALID, f"max_len ({max_len}) < longest uploaded record ({longest})")
        self.log.append({"device": self.device_id, "session": self, "max_len": int(max_len), "source": int(source),
                         "n_records": len(rec), "pool": pool, "records": rec})
        src = pool
        if source == _lib.SRC_SG_FUSED:
            src = O.filter_wave_pool(rec, pool, sg_window_size=self._sg[0], sg_poly_order=self._sg[1])
        thr = np.full(len(rec), self._thr)
        self._rows = H.oracle_rows(rec, src, thr, left_extension, right_extension, int(max_len))

    def hits_wait(self):
        return len(self._rows)

    def _fill_hits(self, n):
        assert n == len(self._rows)
        return self._rows


def oracle_pool(device_ids=(0,), **kw):
    """A DevicePool of OracleSessions that share one log (`pool.log`) and one list of uploads (`pool.uploads`)."""
    from waveformanalysis_amd.device import DevicePool

    log, uploads = [], []
    pool = DevicePool(device_ids=list(device_ids), session_factory=lambda dev: OracleSession(dev, log, uploads), **kw)
    pool.log, pool.uploads = log, uploads
    return pool


__all__ = ["Run", "run", "RUN_NAMES", "OracleSession", "oracle_pool", "differing_rows", "sparse_chunks_with_empty",
           "THRESHOLD", "LE", "RE", "SG", "MIXED_SEGMENTS", "SPARSE_BLOCK", "SPARSE_PATTERN", "THRESHOLD_HIT_DTYPE"]
