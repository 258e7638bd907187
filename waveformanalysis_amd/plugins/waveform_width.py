"""HipWaveformWidthPlugin -- drop-in for WaveformWidthPlugin
(reference: waveform_analysis/core/plugins/builtin/cpu/waveform_width.py:39-374).

Per `hit` row: baseline = mean of the first 50 samples of the waveform row the hit points at, first
crossings of the rise/fall fractions either side of the peak with linear interpolation, divided by the
sampling rate.  One GPU lane per hit (k_waveform_width); the row lookup and the id columns are table
work done here with numpy.

wave_source="records" (no counterpart in the reference, whose plugin reads dense rows only): the same arithmetic on
waveform = pool[wave_offset[r] : wave_offset[r] + event_length[r]] of the resident records + wave_pool /
wave_pool_filtered, r = the hit's record_id taken as an index into `records` -- the way the `hit` records branch
fetched the waveform the hit was found on (peak_finding.py:401-407).  No dense copy of the samples is built, and the
pool the other records plugins left on the device is used as it is.
"""

from __future__ import annotations

from typing import Any

import numpy as np

from ..dtypes import WAVEFORM_WIDTH_DTYPE
from ..plugin_api import Option, Plugin
from . import _common as K


def first_row_of_record_id(row_record_ids: np.ndarray, wanted: np.ndarray) -> np.ndarray:
    """Index of the FIRST row whose record_id equals each wanted id, -1 if none
    (waveform_width.py:163-167: np.flatnonzero(record_id == wanted)[0])."""
    ids, first = np.unique(np.asarray(row_record_ids, dtype=np.int64), return_index=True)
    wanted = np.asarray(wanted, dtype=np.int64)
    pos = np.searchsorted(ids, wanted)
    pos_c = np.minimum(pos, max(len(ids) - 1, 0))
    found = (pos < len(ids)) & (ids[pos_c] == wanted) if len(ids) else np.zeros(len(wanted), dtype=bool)
    return np.where(found, first[pos_c] if len(ids) else -1, -1).astype(np.int64)


class HipWaveformWidthPlugin(K.HipPlugin):
    """Rise / fall / total width per detected peak, computed on the GPU."""

    provides = "waveform_width"
    algorithmic_bytes = (0, 0, 56)  # device pass: bytes per sample, per record, per output row
    depends_on = []  # dynamic, see resolve_depends_on
    description = "Calculate rise/fall time based on peak detection results (HIP, gfx950)."
    version = "3.0.0+hip1"
    save_when = "always"
    output_dtype = WAVEFORM_WIDTH_DTYPE

    options = {
        "use_filtered": Option(default=False, type=bool, help="read filtered_waveforms instead of st_waveforms"),
        "wave_source": Option(default=K.WAVE_SOURCE_AUTO, type=str,
                              help="auto|records|st_waveforms|filtered_waveforms"),
        "sampling_rate": Option(default=None, type=float, help="sampling rate (GHz); 0.5 when unset"),
        "rise_low": Option(default=0.1, type=float, help="low fraction of the rise time"),
        "rise_high": Option(default=0.9, type=float, help="high fraction of the rise time"),
        "fall_high": Option(default=0.9, type=float, help="high fraction of the fall time"),
        "fall_low": Option(default=0.1, type=float, help="low fraction of the fall time"),
        "interpolation": Option(default=True, type=bool, help="linear interpolation of the crossings"),
        "devices": Option(default=None, track=False, help=K.DEVICES_HELP),
    }

    def resolve_depends_on(self, context: Any, run_id: str | None = None) -> list[str]:
        _kind, deps, _name = K.resolve_wave_input(context, self)
        return ["hit"] + deps

    def compute(self, context: Any, run_id: str, **_kwargs) -> np.ndarray:
        kind, _deps, data_name = K.resolve_wave_input(context, self)
        sampling_rate = context.get_config(self, "sampling_rate")
        if sampling_rate is None:
            sampling_rate = 0.5
        # python floats, as Option(type=float) delivers them: numpy then keeps float32 rows in float32
        rise_low = float(context.get_config(self, "rise_low"))
        rise_high = float(context.get_config(self, "rise_high"))
        fall_high = float(context.get_config(self, "fall_high"))
        fall_low = float(context.get_config(self, "fall_low"))
        interpolation = bool(context.get_config(self, "interpolation"))

        hits = context.get_data(run_id, "hit")
        if kind == "records":
            return self._compute_records(context, run_id, data_name, hits, rise_low, rise_high, fall_high, fall_low,
                                         float(sampling_rate), interpolation)
        waveform_data = context.get_data(run_id, data_name)
        if not isinstance(hits, np.ndarray):
            raise ValueError("waveform_width expects hit as a single structured array")
        if not isinstance(waveform_data, np.ndarray):
            raise ValueError("waveform_width expects st_waveforms as a single structured array")
        if len(hits) == 0 or len(waveform_data) == 0:
            return np.zeros(0, dtype=WAVEFORM_WIDTH_DTYPE)

        record_id, position = _hit_columns(hits)
        if "record_id" in (waveform_data.dtype.names or ()):
            row = first_row_of_record_id(waveform_data["record_id"], record_id)
        else:
            row = np.where((record_id >= 0) & (record_id < len(waveform_data)), record_id, -1)

        dense_in = K.dense_input(waveform_data, data_name)

        def widths(sess, _records, mine, row_k, n_rows):
            return sess.waveform_width(dense_in.source, position[mine], row_k, n_rows, dense_in.L, rise_low, rise_high,
                                       fall_high, fall_low, float(sampling_rate), interpolation)

        # devices: the hit table is cut by the shard its row falls in, rows and valid scattered back into hit order
        rows, valid = K.dense_hit_route(context, self, dense_in, row, widths)
        return _kept_rows(rows, valid, hits, record_id)

    def _compute_records(self, context, run_id, pool_name, hits, rise_low, rise_high, fall_high, fall_low, sampling_rate,
                         interpolation) -> np.ndarray:
        """The hit's record_id is an index into `records` (range-checked on the device); the session is the calling
        thread's, its pool uploaded only if another array has taken its place since `hit` / `basic_features` ran."""
        if not isinstance(hits, np.ndarray):
            raise ValueError("waveform_width expects hit as a single structured array")
        records, pool = K.load_records_input(context, self, run_id, pool_name)
        if len(hits) == 0 or len(records) == 0:
            return np.zeros(0, dtype=WAVEFORM_WIDTH_DTYPE)
        record_id, position = _hit_columns(hits)
        cacheable = True
        if pool_name == "wave_pool_filtered":
            pool, cacheable = K.float32_pool(pool)
            source = K.SRC_F32
        else:
            source = K.pool_source(pool, raw_only=True)

        def widths(sess, rec_k, mine, record_k, _n_records):
            if not sess.holds_records(rec_k):  # (a pool upload has dropped the note; a shard's records are new every run)
                sess.upload_records(rec_k)
                sess.note_records(rec_k)
            return sess.waveform_width_records(source, position[mine], record_k, rise_low, rise_high, fall_high,
                                               fall_low, sampling_rate, interpolation)

        # devices: the hit table is cut by the shard that holds record `record_id`; a shard with no hits uploads nothing
        rows, valid = K.records_hit_route(context, self, records, pool, record_id, widths, cacheable=cacheable)
        return _kept_rows(rows, valid, hits, record_id)


def _hit_columns(hits: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(record_id, position) of a hit table as int64 columns (waveform_width.py:154-159)."""
    hit_names = hits.dtype.names or ()
    record_id = np.asarray(hits["record_id"] if "record_id" in hit_names else hits["event_index"], dtype=np.int64)
    position = np.asarray(hits["position"], dtype=np.int64)
    if np.any(position < 0):
        raise ValueError("waveform_width (HIP backend) requires hit positions >= 0")
    return record_id, position


def _kept_rows(rows: np.ndarray, valid: np.ndarray, hits: np.ndarray, record_id: np.ndarray) -> np.ndarray:
    """The rows of the hits the reference keeps, in hit order, id fields from the hit table."""
    out = rows[valid]
    sel = hits[valid]
    out["timestamp"] = sel["timestamp"]
    out["board"] = sel["board"] if "board" in (hits.dtype.names or ()) else 0
    out["channel"] = sel["channel"]
    out["record_id"] = record_id[valid]
    return out
