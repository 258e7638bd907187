"""PushStream -- what the carry streams share on the host (hit_grouped_stream, hit_merged_stream,
hit_merged_grouped_stream, df_events_stream).  Each chunks the static `records` array, lets an inner per-chunk stream
compute every chunk's rows, and pushes them in chunk order to ONE more session borrowed for the whole run, with a horizon
below which nothing later lies; the device keeps what is still open (the carry) between pushes."""

from __future__ import annotations

import time
from typing import Any

import numpy as np

from .chunk import Chunk
from .device import DevicePool
from .streaming import HipStreamingPlugin, _RecordsChunking, given_options, option_resolver


def later_minima(chunks: list) -> list:
    """Per records chunk the minimum record timestamp over all records of LATER chunks (a suffix minimum, taken once per
    run; correct for unsorted runs as well); None where no record follows."""
    out: list = [None] * len(chunks)
    later = None
    for k in range(len(chunks) - 1, -1, -1):
        out[k] = later
        if len(chunks[k].data):
            first = int(chunks[k].data["timestamp"].min())
            later = first if later is None else min(later, first)
    return out


class PushStream(_RecordsChunking, HipStreamingPlugin):
    """Base of the carry streams.  A subclass builds its inner stream (`_inner`), cuts the run into pushes
    (`run_chunks`, which ends in `_push_loop`), opens and closes the device stream (`_begin` / `_end`), turns one push
    into a result chunk or None (`_push`) and names its counters (`counters`).

    Stateful (the carry lives on the device between chunks) and not reset at a time break: what is open may span one.
    A value given to the constructor wins over the Context, the Context over the option's default."""

    depends_on = ["records", "wave_pool"]
    version = "0.1.0+hip1"
    save_when = "never"
    chunk_size = 50_000
    length_field = "event_length"
    is_stateful = True
    reset_on_break = False
    profile_pushes = False   # measurement: kernel timers on the borrowed session, their report in stats["profile"]
    role = "push"            # what the third session does, for the pool refusal (`_sessions`: what all three do)
    counters: tuple = ()     # the stream's own counters, between rows_out and max_carry in `stats`

    def __init__(self, device_pool: DevicePool | None = None, **given):
        super().__init__()
        self._given = given_options(self, given)
        self.device_pool = device_pool
        self.stats: dict = {}
        self._configure(None)

    def _configure(self, context: Any) -> dict:
        """Constructor argument > Context configuration > option default."""
        value = option_resolver(self, context)
        cfg = {name: value(name) for name in self.options}
        self._check_cfg(cfg)
        self.cfg = cfg
        return cfg

    def _check_cfg(self, cfg: dict) -> None:
        """Convert and refuse the subclass's own options, in place."""

    def _check_scope(self, context: Any) -> None:
        """Refuse a Context the stream does not cover (before any upload)."""

    def _check_pool(self, pool: DevicePool) -> None:
        if int(pool.max_sessions) < 3:
            raise ValueError(f"{self.provides} needs a device pool with max_sessions >= 3 ({self._sessions()}), "
                             f"got {pool.max_sessions}")

    def compute_chunk(self, chunk: Chunk, context: Any, run_id: str, **_kw):
        raise NotImplementedError(f"{self.provides} is stateful across chunks: drive it through compute() / run_chunks()")

    def compute(self, context: Any, run_id: str, **kwargs):
        self._apply_streaming_config(kwargs.pop("streaming_config", None))
        records = context.get_data(run_id, "records")
        if not isinstance(records, np.ndarray) or records.dtype.names is None:
            raise TypeError(f"{self.provides} chunks the structured `records` array")
        # (refusals first: the chunk list is only cut once the run is known to start)
        self._configure(context)
        self._check_scope(context)
        self._check_pool(self._pool(context))
        workers = (kwargs.get("executor_config") or {}).get("max_workers") or self.max_workers
        yield from self.run_chunks(list(self._data_to_chunks(records, run_id)), context, run_id, max_workers=workers)

    def _push_loop(self, pool: DevicePool, cfg: dict, results, n_chunks: int, push_args, flush_args, run_id: str,
                   stats: dict, first_event_time: list | None = None):
        """The push loop: one session borrowed for the whole run, `_begin`, one `_push(sess, *push_args(k, chunk, raw),
        run_id, stats)` per (chunk, raw result) of `results` in order, then one with `flush_args` (None: the last chunk's
        push has closed everything), `_end`.  Yields what the pushes return, Nones dropped."""
        def deliver(out):
            if first_event_time is not None and not first_event_time:
                first_event_time.append(time.perf_counter())
            return out

        with pool.borrow() as sess:
            if self.profile_pushes:
                sess.profile(True)
            self._begin(sess, cfg)
            try:
                k = -1
                for k, (chunk, raw) in enumerate(results):
                    out = self._push(sess, *push_args(k, chunk, raw), run_id, stats)
                    if out is not None:
                        yield deliver(out)
                if k + 1 != n_chunks:
                    raise RuntimeError(f"{self.provides}: {k + 1} results for {n_chunks} chunks")
                if flush_args is not None:
                    out = self._push(sess, *flush_args, run_id, stats)
                    if out is not None:
                        yield deliver(out)
            finally:
                if hasattr(results, "close"):
                    results.close()   # (gives the inner stream's sessions back before ours)
                if self.profile_pushes:
                    stats["profile"] = sess.profile_report()
                    sess.profile(False)
                self._end(sess)

    def _new_stats(self) -> dict:
        return dict.fromkeys(("pushes", "rows_in", "rows_out", *self.counters, "max_carry"), 0)

    @staticmethod
    def _count_push(stats: dict, rows, n_out: int, n_carry: int) -> None:
        stats["pushes"] += 1
        stats["rows_in"] += 0 if rows is None else len(rows)
        stats["rows_out"] += int(n_out)
        stats["max_carry"] = max(stats["max_carry"], int(n_carry))

    def _events_chunk(self, out: np.ndarray, run_id: str, stats: dict, **metadata) -> Chunk | None:
        """The result chunk of the event rows one push closed (None for none): bounds [min t_min, max t_max + 1),
        `first_event` in front of the caller's metadata, stats["events"] = events delivered so far."""
        if len(out) == 0:
            return None
        stats["events"] = int(out["event_id"][-1]) + 1
        result = Chunk(out, int(out["t_min"].min()), int(out["t_max"].max()) + 1, run_id, self.provides,
                       data_kind=self.output_data_kind, time_field="t_min", endtime_field="t_max",
                       metadata={"first_event": int(out["event_id"][0]), **metadata})
        self._validate_chunk(result)
        return result


__all__ = ["PushStream", "later_minima"]
