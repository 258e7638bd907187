"""HipRecordsStream -- `records` and `wave_pool` from CAEN V1725 DAW_DEMO files, block by block: the head of the
streaming chain.

The static route (records_builder.build_records_from_v1725_files) reads every file whole, sorts the whole run and packs
the whole pool.  Its table is the stable sort of the concatenated per-file waves by (timestamp, pid = 0, board, channel):
spelled out, by (timestamp, board, channel, file index, wave index in file).  The stream delivers the same rows and the
same samples in the same order, chunk after chunk, and keeps on the GPU only the waves that a later block could still
precede.

The promise.  V1725 files are not time-sorted -- the waves of one event header differ by a few ticks -- so the caller
promises a bound: inside one file, a wave's timestamp is never more than `reorder_window_ns` below the greatest timestamp
before it in that file.  Timestamps are in ps as in `records` (ticks * dt_ns * 1000) and the window goes down as
reorder_window_ns * 1000, all in int64.  A wave that breaks the promise is a ValueError raised on the host before its block
is uploaded; the chunks delivered before it are then not, in general, a prefix of the static table (a wave that came too
late may belong in front of rows already released).

The schedule (ReadSchedule, pure Python: no device, no file).  Per file f: hi_f = the greatest timestamp read so far,
low_f = hi_f - window, saturating at the smallest int64, which it also is while nothing of f has been read.  The next block
comes from the unfinished file with the smallest low_f (ties: the lowest file index); a block is whole events from the
file's position while (end of event - block start) <= block_bytes, at least one event; only at the end of a file does a
short header or payload end the walk, the complete waves of the cut event kept.  One push follows every block with the
horizon H = min low_f over the unfinished files, final when none is left.  A push releases, in the static order, every
held wave with timestamp < H, strictly (a later wave may tie at H with a smaller board / channel); a final push releases
everything.  H never decreases.

The device part is wfa_records_stream_* (DeviceSession.records_stream_begin / _push / _end): order, offsets, ONE sample
pass from the block's bytes and the old sample carry to the output pool and the new sample carry, rows written on the
device.
"""

from __future__ import annotations

import os
import time
from typing import Any

import numpy as np

from . import records_builder as RB
from .chunk import Chunk
from .device import DevicePool
from .dtypes import RECORDS_DTYPE
from .plugin_api import Option
from .streaming import HipStreamingPlugin, given_options, option_resolver

INT64_MIN = int(np.iinfo(np.int64).min)
INT64_MAX = int(np.iinfo(np.int64).max)
HORIZON_END = INT64_MAX            # the horizon of the final push: nothing follows
DEFAULT_BLOCK_BYTES = 64 << 20
SEQ_FILE_SHIFT = 40                # seq = file index << 40 | wave index in file


def window_ps(reorder_window_ns) -> int:
    """reorder_window_ns (int >= 0) in ps; refused when the product leaves int64."""
    if isinstance(reorder_window_ns, bool) or not isinstance(reorder_window_ns, (int, np.integer)):
        raise ValueError(f"reorder_window_ns must be an int >= 0, got {reorder_window_ns!r}")
    w = int(reorder_window_ns)
    if w < 0:
        raise ValueError(f"reorder_window_ns must be >= 0, got {w}")
    if w * 1000 > INT64_MAX:
        raise ValueError(f"reorder_window_ns = {w}: the window in ps does not fit int64")
    return w * 1000


class ReadSchedule:
    """Read order and horizon rule of the records stream.  Fed the timestamps (ps) of every block in file order, it says
    which file to read next and what (H, final) the push behind a block carries.  No device, no file access."""

    def __init__(self, names, reorder_window_ns: int = 0):
        self.names = [str(n) for n in names]
        self.window = window_ps(reorder_window_ns)
        n = len(self.names)
        self.hi: list = [None] * n          # greatest timestamp read so far (None: nothing read)
        self.done = [False] * n
        self.waves = [0] * n                # waves read so far = index in its file of the next one
        self.horizon = INT64_MIN

    def low(self, f: int) -> int:
        return INT64_MIN if self.hi[f] is None else max(self.hi[f] - self.window, INT64_MIN)

    def next_file(self):
        """The unfinished file with the smallest low_f, ties to the lowest index; None when no file is left."""
        best = None
        for f in range(len(self.names)):
            if not self.done[f] and (best is None or self.low(f) < self.low(best)):
                best = f
        return best

    def feed(self, f: int, timestamps_ps, at_end: bool) -> tuple[int, bool]:
        """The block just read from file f (its waves' timestamps in file order; at_end: the file is finished) ->
        (H, final).  A wave below (greatest timestamp before it in f) - window is a ValueError, and nothing is taken."""
        if self.done[f]:
            raise RuntimeError(f"file {self.names[f]} is finished")
        ts = np.asarray(timestamps_ps, dtype=np.int64)
        hi = self.hi[f]
        if len(ts):
            before = np.maximum.accumulate(np.concatenate(([INT64_MIN if hi is None else hi], ts)))[:-1]
            # before - window, saturating at the smallest int64 (the wrapped differences are the ones not taken)
            low = np.where(before < INT64_MIN + self.window, INT64_MIN, before - np.int64(self.window))
            bad = np.flatnonzero(ts < low)
            if len(bad):
                k = int(bad[0])
                need = -((int(ts[k]) - int(before[k])) // 1000)
                raise ValueError(f"{self.names[f]}: wave {self.waves[f] + k} lies {int(before[k]) - int(ts[k])} ps below the "
                                 f"greatest timestamp before it in the file; reorder_window_ns = {self.window // 1000} "
                                 f"promises less, {need} would have been needed")
            self.hi[f] = max(int(ts.max()), INT64_MIN if hi is None else hi)
            self.waves[f] += len(ts)
        if at_end:
            self.done[f] = True
        left = [self.low(g) for g in range(len(self.names)) if not self.done[g]]
        if not left:
            self.horizon = HORIZON_END
            return HORIZON_END, True
        self.horizon = max(self.horizon, min(left))   # (min low_f never decreases; the max only says so)
        return self.horizon, False


class BlockFile:
    """One V1725 file read block by block: whole events from the current position while (end of event - block start) <=
    block_bytes, at least one event; at the end of the file the walk ends as wfa_v1725_index ends it."""

    def __init__(self, path: str, block_bytes: int):
        self.path = path
        self.block_bytes = int(block_bytes)
        self.fh = open(path, "rb")
        self.buf = np.zeros(0, dtype=np.uint8)   # bytes read and not yet handed out
        self.eof = False
        self.bytes_read = 0

    def close(self) -> None:
        self.fh.close()

    def _fill(self, want: int) -> None:
        """Hold want + 1 bytes, or the rest of the file (the extra byte tells a window that ends with the file)."""
        while len(self.buf) <= want and not self.eof:
            ask = want + 1 - len(self.buf)
            got = np.fromfile(self.fh, dtype=np.uint8, count=ask)
            self.bytes_read += len(got)
            if len(got) < ask:
                self.eof = True
            if len(got):
                self.buf = got if len(self.buf) == 0 else np.concatenate([self.buf, got])

    def _window(self, size: int):
        self._fill(size)
        at_end = self.eof and len(self.buf) <= size
        return self.buf[: min(len(self.buf), size)], at_end

    def next_block(self):
        """-> (the block's bytes, index columns with payload_offset into the block, at_end)."""
        size = self.block_bytes
        view, at_end = self._window(size)
        idx, used = RB.v1725_index_block(view, at_end)
        if used == 0 and not at_end:
            # the first event is longer than block_bytes: it is read whole, alone.  `used` is 0 below its end and positive
            # from there on: grow the window until it holds the event, then bisect for the event's end
            short = len(view)
            while used == 0 and not at_end:
                short = len(view)
                size *= 2
                view, at_end = self._window(size)
                idx, used = RB.v1725_index_block(view, False)
            if used == 0:      # the file ends inside its last event
                idx, used = RB.v1725_index_block(view, True)
            else:
                at_end = False
                long = len(view)
                while long - short > 1:
                    mid = (short + long) // 2
                    if RB.v1725_index_block(view[:mid], False)[1] > 0:
                        long = mid
                    else:
                        short = mid
                idx, used = RB.v1725_index_block(view[:long], False)
                at_end = self.eof and used == len(self.buf)
        block = self.buf[:used]
        self.buf = self.buf[used:]
        return block, idx, at_end


class HipRecordsStream(HipStreamingPlugin):
    """compute() = the records of a run's V1725 files with their samples, delivered in the static table's order as the
    horizon passes them.

    Options: `daq_adapter` (anything but "v1725" is a ValueError before a file is opened: the VX2730 CSV route stays
    static), `dt` (ns per sample, resolved like the records plugin's: resolve_dt_ns), `block_bytes` (default 64 MiB, >= 1;
    an event longer than that is read whole), `reorder_window_ns` (int >= 0, default 0: the promise of the module
    docstring).  A value given to the constructor wins over the Context, the Context over the option's default.

    `compute(context, run_id)` takes the paths from `raw_files` (the groups flattened, a path once, in order) and
    `stream_files(paths, dt_ns, ...)` takes them as given: order and duplicates are the caller's, a missing file is
    skipped, as in the static builder.  Both yield one Chunk per push that releases at least one record: `data` is the
    RECORDS_DTYPE rows (apply_records_polarity applied per chunk when a Context is at hand; wave_offset and record_id count
    through the run), `metadata` holds `wave_pool` (this chunk's samples, a host uint16 array), `pool_base` (the run offset
    of its first sample), `horizon`, `n_carry` and `first_record`.  All chunks concatenated are the static bundle of the
    same paths, byte for byte.  If a file breaks the promise the ValueError names the file, the wave and the window that
    would have been needed; the chunks delivered before it are not, in general, a prefix of the static table.

    `stats` after (or during) a run: pushes, rows_in, rows_out, max_carry, max_carry_samples, bytes_read, and
    samples_moved (what the sample passes wrote: released + carried samples, summed over the pushes).

    Stateful: the carry lives on one session borrowed for the whole run."""

    provides = "records_stream"
    depends_on = ["raw_files"]
    description = "records and wave_pool from V1725 files, block by block (HIP, gfx950)."
    version = "0.1.0+hip1"
    output_dtype = RECORDS_DTYPE
    output_data_kind = "records"
    save_when = "never"
    length_field = "event_length"
    is_stateful = True
    reset_on_break = False
    profile_pushes = False   # measurement: kernel timers on the borrowed session, their report in stats["profile"]

    options = {
        "daq_adapter": Option(default="v1725", type=str, help="DAQ adapter; the records stream reads v1725 only"),
        "dt": Option(default=None, type=int, help="Sample interval in ns (defaults to the adapter's rate)"),
        "block_bytes": Option(default=DEFAULT_BLOCK_BYTES, type=int, help="bytes read per block (whole events), >= 1"),
        "reorder_window_ns": Option(default=0, type=int,
                                    help="inside one file no wave lies more than this below the greatest timestamp before it"),
    }

    def __init__(self, device_pool: DevicePool | None = None, **given):
        super().__init__()
        self._given = given_options(self, given)
        self.device_pool = device_pool
        self.stats: dict = {}
        self._configure(None)

    def _configure(self, context: Any) -> dict:
        """Constructor argument > Context configuration > option default; refusals before a file is opened."""
        value = option_resolver(self, context)
        cfg = {name: value(name) for name in self.options}
        adapter = cfg["daq_adapter"]
        if not isinstance(adapter, str) or adapter.lower() != "v1725":
            raise ValueError(f"records_stream reads v1725 binary files, not {adapter!r} (the VX2730 CSV route is static)")
        cfg["daq_adapter"] = "v1725"
        cfg["block_bytes"] = self._block_bytes(cfg["block_bytes"])
        window_ps(cfg["reorder_window_ns"])
        cfg["reorder_window_ns"] = int(cfg["reorder_window_ns"])
        self.cfg = cfg
        return cfg

    @staticmethod
    def _block_bytes(value) -> int:
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) < 1:
            raise ValueError(f"block_bytes must be an int >= 1, got {value!r}")
        return int(value)

    def compute_chunk(self, chunk: Chunk, context: Any, run_id: str, **_kw):
        raise NotImplementedError("records_stream reads files, not chunks: drive it through compute() / stream_files()")

    def compute(self, context: Any, run_id: str, **kwargs):
        from .plugins.records import resolve_dt_ns

        cfg = self._configure(context)
        dt_ns = resolve_dt_ns(context, self, adapter_name="v1725")
        raw_files = context.get_data(run_id, "raw_files")
        seen, paths = set(), []
        for group in raw_files or ():
            for path in ([group] if isinstance(group, (str, os.PathLike)) else group or ()):
                if path not in seen:
                    seen.add(path)
                    paths.append(path)
        yield from self.stream_files(paths, dt_ns, block_bytes=cfg["block_bytes"], reorder_window_ns=cfg["reorder_window_ns"],
                                     context=context, run_id=run_id)

    def stream_files(self, paths, dt_ns: int, block_bytes: int | None = None, reorder_window_ns: int | None = None,
                     context: Any = None, run_id: str = "", first_chunk_time: list | None = None):
        """Generator over the chunks of `paths` (see the class docstring).  `first_chunk_time` (optional list) receives
        time.perf_counter() when the first chunk is delivered."""
        block_bytes = self.cfg["block_bytes"] if block_bytes is None else self._block_bytes(block_bytes)
        window_ns = self.cfg["reorder_window_ns"] if reorder_window_ns is None else reorder_window_ns
        window_ps(window_ns)
        dt_ns = int(dt_ns)
        if dt_ns <= 0 or dt_ns > np.iinfo(np.int32).max:
            raise ValueError(f"dt_ns must be in 1 .. 2^31 - 1, got {dt_ns}")
        paths = [str(p) for p in paths if os.path.exists(p)]   # the reference's reader logs a warning and goes on
        stats = self.stats = dict.fromkeys(("pushes", "rows_in", "rows_out", "max_carry", "max_carry_samples", "bytes_read",
                                            "samples_moved"), 0)
        if not paths:
            return
        schedule = ReadSchedule(paths, window_ns)
        boards = [RB._board_from_path(p) for p in paths]
        scale = np.int64(dt_ns * 1000)
        files: list = [None] * len(paths)
        with self._pool(context).borrow() as sess:
            if self.profile_pushes:
                sess.profile(True)
            sess.records_stream_begin(dt_ns)
            try:
                while True:
                    f = schedule.next_file()
                    if f is None:
                        break
                    if files[f] is None:
                        files[f] = BlockFile(paths[f], block_bytes)
                    before = files[f].bytes_read
                    block, idx, at_end = files[f].next_block()
                    stats["bytes_read"] += files[f].bytes_read - before
                    n = len(idx["channel"])
                    first_wave = schedule.waves[f]
                    waves = {
                        "timestamp_ps": idx["timestamp"] * scale,     # SAMPLE_INDEX mode (formats/base.py:177-185)
                        "seq": (np.int64(f) << SEQ_FILE_SHIFT) + first_wave + np.arange(n, dtype=np.int64),
                        "payload_offset": idx["payload_offset"], "n_samples": idx["n_samples"],
                        "board": np.full(n, boards[f], dtype=np.int16), "channel": idx["channel"],
                        "baseline": idx["baseline"], "trunc": idx["trunc"],
                    }
                    horizon, final = schedule.feed(f, waves["timestamp_ps"], at_end)   # (refuses before the upload)
                    if at_end:
                        files[f].close()
                    rows, pool, n_carry, n_carry_samples = sess.records_stream_push(block, waves, horizon, final)
                    stats["pushes"] += 1
                    stats["rows_in"] += n
                    stats["rows_out"] += len(rows)
                    stats["max_carry"] = max(stats["max_carry"], n_carry)
                    stats["max_carry_samples"] = max(stats["max_carry_samples"], n_carry_samples)
                    stats["samples_moved"] += len(pool) + n_carry_samples
                    if len(rows) == 0:
                        continue
                    if context is not None:
                        from .plugins.records import apply_records_polarity

                        apply_records_polarity(context, run_id, rows)
                    if first_chunk_time is not None and not first_chunk_time:
                        first_chunk_time.append(time.perf_counter())
                    yield self._chunk(rows, pool, horizon, n_carry, run_id)
            finally:
                for bf in files:
                    if bf is not None:
                        bf.close()
                if self.profile_pushes:
                    stats["profile"] = sess.profile_report()
                    sess.profile(False)
                sess.records_stream_end()

    def _chunk(self, rows: np.ndarray, pool: np.ndarray, horizon: int, n_carry: int, run_id: str) -> Chunk:
        endtime = rows["timestamp"].astype(np.int64) + rows["dt"].astype(np.int64) * 1000 * rows["event_length"]
        return Chunk(rows, int(rows["timestamp"][0]), int(endtime.max()) + 1, run_id=run_id, data_type="records",
                     data_kind="records", time_field="timestamp", length_field="event_length",
                     metadata={"first_record": int(rows["record_id"][0]), "wave_pool": pool,
                               "pool_base": int(rows["wave_offset"][0]), "horizon": int(horizon), "n_carry": int(n_carry)})


__all__ = ["HipRecordsStream", "ReadSchedule", "BlockFile", "window_ps", "HORIZON_END", "DEFAULT_BLOCK_BYTES"]
