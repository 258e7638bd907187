"""HipBasicFeaturesStream -- `basic_features` of the records route as a chunk stream.

The reference computes basic_features for a whole run at once (cpu/basic_features.py:43-278) and has no streaming form of
it.  The features of a record depend on that record alone, so one chunk of records goes through the static plugin's device
pass on one DeviceSession: the chunk's slice of the pool and its records go up, wfa_basic_features runs, and the
BASIC_FEATURES_DTYPE rows come back.  All chunks together are the rows of the static plugin on the records route, byte for
byte, whatever the chunk size.
"""

from __future__ import annotations

from typing import Any

import numpy as np

from .chunk import Chunk
from .device import DevicePool
from .dtypes import BASIC_FEATURES_DTYPE
from .plugin_api import Option
from .plugins import _common as K
from .plugins.basic_features import PEAK_RANGE
from .streaming import HipStreamingPlugin, _RecordsChunking, given_options, option_resolver


class HipBasicFeaturesStream(_RecordsChunking, HipStreamingPlugin):
    """compute_chunk() = the basic_features rows of one chunk of records.

    `compute(context, run_id)` streams over the static `records` array, chunked like hit_threshold_stream: `chunk_size`
    consecutive records of a time segment, nothing widened, nothing clipped.  Per chunk a session is borrowed from the
    device pool (serial, or the worker threads of `_compute_parallel`, one session each) and runs
      upload_pool(the chunk's slice, cut as HipThresholdHitStream._stage cuts it) + upload_records(wave_offset rebased)
      -> basic_features(fixed_baseline = K.fixed_baseline_per_record of the chunk's records).
    `event_index` is the row's index in the Context's `records`: a chunk's metadata["first_record"] counts inside its
    time segment, so the chunk rule here numbers the chunks through the run (metadata["record_base"]).

    Options carry the static plugin's names and defaults (height_range, area_range, channel_config); a value given to
    the constructor wins over the Context, the Context over the default.  Refused with a ValueError before any upload:
    use_filtered=True (no filtered pool is built per chunk here), the deprecated fixed_baseline option, and a
    wave_source other than "records" (the dense route is outside the stream; unlike the static plugin's, the stream's
    default is "records")."""

    provides = "basic_features_stream"
    depends_on = ["records", "wave_pool"]
    description = "basic_features of the records stream, chunk by chunk (HIP, gfx950)."
    version = "0.1.0+hip1"
    output_dtype = BASIC_FEATURES_DTYPE
    save_when = "never"
    chunk_size = 50_000
    length_field = "event_length"
    output_data_kind = "features"

    options = {
        "height_range": Option(default=PEAK_RANGE, type=tuple, help="(start, end) for height/amp"),
        "area_range": Option(default=(0, None), type=tuple, help="(start, end) for area; None = to the end"),
        "channel_config": Option(default=None, type=dict, help="per (board, channel) fixed_baseline"),
        "use_filtered": Option(default=False, type=bool, help="refused when set: the stream reads wave_pool"),
        "wave_source": Option(default=K.WAVE_SOURCE_RECORDS, type=str, help="records (anything else is refused)"),
        "fixed_baseline": Option(default=None, type=dict, help="deprecated and refused; use channel_config"),
    }

    def __init__(self, device_pool: DevicePool | None = None, **given):
        super().__init__()
        self._given = given_options(self, given)
        self.device_pool = device_pool
        self._configure(None)

    def _configure(self, context: Any) -> dict:
        """Constructor argument > Context configuration > option default; the refusals.  Worker threads share the
        plugin: a chunk works on the dict it was handed."""
        value = option_resolver(self, context)
        if bool(value("use_filtered")):
            raise ValueError(f"{self.provides}: use_filtered=True is outside the stream (no filtered pool is built per chunk)")
        if value("fixed_baseline"):
            raise ValueError(f"{self.provides}: the deprecated fixed_baseline option is outside the stream; use channel_config")
        source = K.normalize_wave_source(value("wave_source"))
        if source != K.WAVE_SOURCE_RECORDS:
            raise ValueError(f"{self.provides} reads records + wave_pool; wave_source must be 'records' (got {source!r})")
        cfg = {"height_range": tuple(value("height_range")), "area_range": tuple(value("area_range")),
               "channel_config": value("channel_config") or None}
        self.cfg = cfg
        return cfg

    def _data_to_chunks(self, data: Any, run_id: str):
        base = 0
        for ch in super()._data_to_chunks(data, run_id):
            ch.metadata["record_base"] = base   # index of the chunk's first record in the run's `records`
            base += len(ch.data)
            yield ch

    def _get_input_chunks(self, context: Any, run_id: str, **kwargs):
        self._configure(context)   # (refusals before anything is cut or uploaded)
        return super()._get_input_chunks(context, run_id, **kwargs)

    def _result(self, chunk: Chunk, rows: np.ndarray, run_id: str) -> Chunk:
        end = int(chunk.end)
        if len(chunk.data):
            end = max(end, int(self._endtime_of(chunk.data, "timestamp").max()) + 1)
        return Chunk(rows, chunk.start, end, run_id, self.provides, data_kind=self.output_data_kind,
                     time_field="timestamp", metadata=dict(chunk.metadata))

    def compute_chunk(self, chunk: Chunk, context: Any, run_id: str, **_kw) -> Chunk:
        return self._compute_one(chunk, context, run_id, self._configure(context))

    def _compute_one(self, chunk: Chunk, context: Any, run_id: str, cfg: dict) -> Chunk:
        recs = chunk.data
        if len(recs) == 0:
            return self._result(chunk, np.zeros(0, dtype=BASIC_FEATURES_DTYPE), run_id)
        fixed = K.fixed_baseline_per_record(recs, cfg["channel_config"], run_id)
        wave_pool = context.get_data(run_id, "wave_pool")
        K.pool_source(wave_pool, raw_only=True)
        # the slice of the pool from the chunk's first sample to its last (see HipThresholdHitStream._stage)
        lo = int(recs["wave_offset"].min())
        hi = int((recs["wave_offset"].astype(np.int64) + recs["event_length"]).max())
        sub = recs.copy()
        sub["wave_offset"] -= lo
        # worker threads come and go with every compute(): the session is borrowed for this chunk only
        samples = wave_pool[lo:hi] if hi > lo else np.zeros(1, dtype=np.uint16)   # (records without samples read none)
        with self._pool(context).borrow() as sess:
            sess.upload_pool(np.ascontiguousarray(samples))
            sess.upload_records(sub)
            rows = sess.basic_features(K.SRC_RAW, cfg["height_range"], cfg["area_range"], fixed)
        meta = chunk.metadata
        rows["event_index"] += int(meta.get("record_base", meta.get("first_record", 0)))
        return self._result(chunk, rows, run_id)


__all__ = ["HipBasicFeaturesStream"]
