"""HipThresholdHitPlugin -- drop-in for ThresholdHitPlugin
(reference: waveform_analysis/core/plugins/builtin/cpu/hit_finder.py:82-413)."""

from __future__ import annotations

from functools import partial
from typing import Any

import numpy as np

from .. import _lib, dense
from ..dtypes import THRESHOLD_HIT_DTYPE
from ..plugin_api import Option, Plugin
from ..records_builder import _baseline_window
from ..filter_engine import design_bw, plan_fused_groups, stage_fused_groups
from ..sg_plan import normalize_window
from . import _common as K


def fuse_baseline_window(value) -> tuple[int, int] | None:
    """The fuse_baseline option as (start, end), validated like the (start, end) form of the records builder's
    baseline_samples (same messages): None, or two non-negative ints with start < end.  An empty window is refused
    because the two routes of the plugin would read it differently: the fused entry point of the library skips the
    estimate for end <= start and keeps the uploaded baselines, baseline_mean gives NaN and with it no hits."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (tuple, list)):
        raise TypeError(f"fuse_baseline must be None or a tuple (start, end), got {type(value).__name__}")
    return _baseline_window(value, 0, 0, 1)


def _valid_fuse_baseline(value) -> bool:
    try:
        fuse_baseline_window(value)
    except (TypeError, ValueError):
        return False
    return True


class HipThresholdHitPlugin(K.HipPlugin):
    """Threshold-only hit detector with THRESHOLD_HIT_DTYPE output, computed on the GPU."""

    provides = "hit_threshold"
    algorithmic_bytes = (2, 29, 60)  # device pass: bytes per sample, per record, per output row
    depends_on = []  # dynamic, see resolve_depends_on
    description = "Threshold-only hit detector with THRESHOLD_HIT_DTYPE output (HIP, gfx950)."
    version = "0.11.0+hip1"
    output_dtype = THRESHOLD_HIT_DTYPE
    save_when = "always"

    options = {
        "threshold": Option(default=10.0, type=float, help="hit threshold"),
        "use_filtered": Option(default=False, type=bool, help="threshold the filtered waveform"),
        "fuse_filter": Option(
            default=False, type=bool,
            help="with use_filtered: evaluate the filter inside the hit kernel from wave_pool instead of reading a "
                 "materialised wave_pool_filtered (same result).  The filter settings are those of the registered "
                 "wave_pool_filtered plugin, resolved per record (filter_type, channel_config): one Savitzky-Golay "
                 "setting for the run is one pass; several settings (at most 8; fuse_filter=False takes any number) "
                 "run one pass each over the resident pool, their rows merged on the device; a Butterworth group is "
                 "filtered on the device first (never downloaded)"),
        "fuse_baseline": Option(
            default=None, validate=_valid_fuse_baseline,
            help="None, or (start, end) with 0 <= start < end: re-estimate records.baseline as the mean of samples "
                 "[start, min(end, event_length)) inside the hit kernel (the records-builder rule; NaN and no "
                 "hits for a record that ends at or before start)"),
        "wave_source": Option(default=K.WAVE_SOURCE_AUTO, type=str,
                              help="auto|records|st_waveforms|filtered_waveforms"),
        "left_extension": Option(default=2, type=int, help="samples added left of a hit"),
        "right_extension": Option(default=2, type=int, help="samples added right of a hit"),
        "dt": Option(default=None, type=int, help="sample interval (ns) when records lack dt"),
        "channel_config": Option(default=None, type=dict, help="per (board, channel) threshold"),
        "devices": Option(default=None, track=False, help=K.DEVICES_HELP),
    }

    def resolve_depends_on(self, context: Any, run_id: str | None = None) -> list[str]:
        kind, deps, _name = K.resolve_wave_input(context, self)
        if kind == "dense":
            return deps
        deps, _pool = K.records_dependencies(context, self)
        return deps

    def compute(self, context: Any, run_id: str, **_kwargs) -> np.ndarray:
        threshold = float(context.get_config(self, "threshold"))
        le = max(0, int(context.get_config(self, "left_extension")))
        re = max(0, int(context.get_config(self, "right_extension")))
        explicit_dt = K.resolve_dt_config(context, self, deprecated_keys=("sampling_interval_ns", "dt_ns"))
        channel_config = context.get_config(self, "channel_config")
        use_filtered = bool(context.get_config(self, "use_filtered"))
        fused = use_filtered and bool(context.get_config(self, "fuse_filter"))
        fuse_baseline = fuse_baseline_window(context.get_config(self, "fuse_baseline"))
        kind, _deps, data_name = K.resolve_wave_input(context, self)
        if kind == "dense":
            return self._compute_dense(context, run_id, data_name, threshold, le, re, explicit_dt, channel_config)
        _deps, pool_name = K.records_dependencies(context, self)
        records, pool = K.load_records_input(context, self, run_id, pool_name)
        if len(records) == 0:
            return np.zeros(0, dtype=THRESHOLD_HIT_DTYPE)

        dt_values = K.require_dt_array(records, explicit_dt=explicit_dt, plugin_name=self.provides,
                                       data_name="records")
        thresholds = K.per_record_channel_option(records, channel_config, run_id, "threshold",
                                                 threshold, threshold)
        rec = records
        if "dt" not in (records.dtype.names or ()):
            rec = K.records_with_dt(records, dt_values)

        cacheable = True
        if use_filtered and not fused:
            pool, cacheable = K.float32_pool(pool)
            source = K.SRC_F32
        else:
            source = K.pool_source(pool, raw_only=True)
            if fused:
                source = K.SRC_SG_FUSED
        sg, groups, group_of_record = None, None, ()
        if fused:
            # the filter settings per record, exactly as wave_pool_filtered resolves them (filtering.py:339-374)
            fplugin = context.get_plugin("wave_pool_filtered") if "wave_pool_filtered" in getattr(context, "_plugins", {}) else None
            plan = plan_fused_groups(context, fplugin, run_id, rec)
            if len(plan) == 1 and plan[0][0][0] == "SG":  # the common case: one Savitzky-Golay pair for the run
                sg = normalize_window(*plan[0][0][1:])
            else:  # one pass per group, the rows merged on the device (records_pass)
                groups = [key for key, _mask in plan]
                if len(groups) > _lib.MAX_HIT_GROUPS:
                    raise ValueError(f"hit_threshold: the run resolves to {len(groups)} distinct filter settings, the "
                                     f"grouped pass takes at most {_lib.MAX_HIT_GROUPS} (fuse_filter=False takes any "
                                     "number of settings)")
                column = np.zeros(len(rec), dtype=np.int32)
                for g, (_key, mask) in enumerate(plan):
                    if mask is not None:
                        column[mask] = g
                group_of_record = (column,)
        return K.records_route(context, self, rec, pool, THRESHOLD_HIT_DTYPE,
                               partial(records_pass, source=source, sg=sg, fuse_baseline=fuse_baseline, le=le, re=re,
                                       groups=groups),
                               (thresholds,) + group_of_record, cacheable=cacheable,
                               download=lambda sess, out: sess.download_hits(out))

    def _compute_dense(self, context, run_id, data_name, threshold, le, re, explicit_dt, channel_config) -> np.ndarray:
        """hit_finder.py:179-255: the whole row is searched; the records/wave_pool length of the same record_id
        (hit_finder.py:257-286) only clamps the reported edges."""
        data = K.load_dense_input(context, self, run_id, data_name)
        if len(data) == 0:
            return np.zeros(0, dtype=THRESHOLD_HIT_DTYPE)
        names = data.dtype.names or ()
        rows = K.dense_input(data, data_name)
        source, L = rows.source, rows.L
        rec = dense.dense_records(data, L, keep_record_id=True)
        rec["dt"] = K.require_dt_array(data, explicit_dt=explicit_dt, plugin_name=self.provides, data_name=data_name)
        if "event_length" in names:
            source_lengths = np.asarray(data["event_length"], dtype=np.int64)
        else:
            source_lengths = np.full(len(data), L, dtype=np.int64)
        record_lengths = _lengths_from_records(context, run_id, rec["record_id"], source_lengths)
        thresholds = K.per_record_channel_option(rec, channel_config, run_id, "threshold", threshold, threshold)
        if "baseline" not in names and source != K.SRC_RAW:
            raise ValueError(f"hit_threshold (HIP backend) needs a 'baseline' field on float32 {data_name}")

        def whole_rows(sess, rec_k, thresholds_k, max_len=0, download=True):
            sess.upload_records(rec_k, thresholds_k)
            if "baseline" not in names:
                sess.baseline_mean(0, L, update_records=True)  # waves.mean(axis=1): exact integer sum / L
            return sess.threshold_hits(source, le, re, max_len=max_len, download=download)

        # the rows above and the clamp below concern the whole run and stay on the whole table; the pass is per shard
        hits = K.dense_route(context, self, rows, rec, THRESHOLD_HIT_DTYPE, whole_rows, (thresholds,),
                             download=lambda sess, out: sess.download_hits(out))
        if len(hits) and np.any(record_lengths < L):
            order = np.argsort(rec["record_id"], kind="stable")
            row = order[np.searchsorted(rec["record_id"][order], hits["record_id"])]
            limit = np.maximum(record_lengths[row], 0).astype(np.int32)
            edge_start = np.minimum(hits["edge_start"], limit)
            edge_end = np.maximum(np.minimum(hits["edge_end"], limit), edge_start)
            hits["edge_start"], hits["edge_end"] = edge_start, edge_end
            hits["width"] = (edge_end - edge_start).astype(np.float32)
        return hits


def records_pass(sess, records: np.ndarray, thresholds, group_of_record=None, *, source: int, sg: tuple[int, int] | None,
                 fuse_baseline, le: int, re: int, groups=None, max_len: int = 0, download: bool = True):
    """The pass K.records_route runs, on a session whose pool is resident: records in, hit pass run ->
    THRESHOLD_HIT_DTYPE rows, or their count with download=False (rows left on the device).  sg: the Savitzky-Golay
    (window, order) of the fused filter, None for the raw / materialised sources.  max_len: the padded width (0 = the
    longest uploaded record; a shard gets the run's width, hit_finder.py:354-370, not its own).

    groups: None, or the filter keys of a fused pass over records with several resolved filter settings
    (filter_engine.plan_fused_groups), `group_of_record` then holding one int32 per record: the index of its key."""
    if groups is not None:
        return _grouped_pass(sess, records, thresholds, group_of_record, groups=groups, fuse_baseline=fuse_baseline, le=le,
                             re=re, max_len=max_len, download=download)
    sess.upload_records(records, thresholds)
    if sg is not None:
        sess.set_sg_plan(*sg)
    if sg is not None and fuse_baseline is not None:
        return sess.fused_baseline_filter_hits(tuple(fuse_baseline), le, re, max_len=max_len, download=download)
    if fuse_baseline is not None:
        sess.baseline_mean(int(fuse_baseline[0]), int(fuse_baseline[1]), update_records=True)
    return sess.threshold_hits(source, le, re, max_len=max_len, download=download)


def _grouped_pass(sess, records: np.ndarray, thresholds, group_of_record, *, groups, fuse_baseline, le: int, re: int,
                  max_len: int, download: bool):
    """Fused pass over records whose channels resolve to several filter settings: the one queued grouped pass of the
    library (filter_engine.stage_fused_groups), one device pass per group over ALL uploaded records -- the uniform
    layout, and with it the streaming / span routes and the padded shadow, stays -- the rows merged on the device into
    the reference's order (record index, start), resident like the rows of one pass.

    `groups` are the run's keys and a key's index is its plan slot on every shard; the groups without a record among
    `records` (a shard) are dropped and group_of_record is renumbered to the positions that are left.  With one
    Savitzky-Golay group left the single pass runs.  A Butterworth group is filtered over the uploaded table into the
    device float32 twin (never downloaded, nobody's wave_pool_filtered afterwards); with fuse_baseline its pass reads
    the baselines one baseline_mean wrote, the Savitzky-Golay groups estimate theirs inside their pass."""
    column = np.asarray(group_of_record, dtype=np.int32)
    slots = [int(g) for g in np.unique(column)] or [0]
    keys = [groups[g] for g in slots]
    if len(keys) == 1 and keys[0][0] == "SG":
        return records_pass(sess, records, thresholds, source=K.SRC_SG_FUSED, sg=keys[0][1:], fuse_baseline=fuse_baseline,
                            le=le, re=re, max_len=max_len, download=download)
    sess.upload_records(records, thresholds)
    if fuse_baseline is not None and any(key[0] == "BW" for key in keys):
        sess.baseline_mean(int(fuse_baseline[0]), int(fuse_baseline[1]), update_records=True)
    window = {} if fuse_baseline is None else {"baseline_window": tuple(fuse_baseline)}
    stage_fused_groups(sess, keys, slots, lambda g: design_bw(*keys[g][1:]), np.searchsorted(slots, column).astype(np.int32),
                       le, re, max_len, **window)
    n = sess.hits_wait()
    return sess._fill_hits(n) if download else n


def _lengths_from_records(context: Any, run_id: str, record_ids: np.ndarray, source_lengths: np.ndarray) -> np.ndarray:
    """hit_finder.py:257-286 (`_resolve_wave_pool_metadata`): every dense row must exist in records with the same
    length; returns the records-side event_length per row."""
    records = context.get_data(run_id, "records")
    if not isinstance(records, np.ndarray) or records.dtype.names is None:
        raise ValueError("hit_threshold needs the 'records' table to resolve record_id into records/wave_pool")
    rid = np.asarray(records["record_id"], dtype=np.int64)
    order = np.argsort(rid, kind="stable")
    # duplicates: the reference's dict keeps the LAST row of an id
    pos = np.searchsorted(rid[order], record_ids, side="right") - 1
    found = (pos >= 0) & (rid[order][np.maximum(pos, 0)] == record_ids) if len(rid) else np.zeros(len(record_ids), bool)
    if not np.all(found):
        bad = int(record_ids[np.flatnonzero(~found)[0]])
        raise ValueError(f"hit_threshold could not resolve record_id={bad} into records/wave_pool")
    lengths = np.asarray(records["event_length"], dtype=np.int64)[order][pos]
    diff = np.flatnonzero(lengths != source_lengths)
    if len(diff):
        i = int(diff[0])
        raise ValueError("hit_threshold waveform source length does not match records/wave_pool length for "
                         f"record_id={int(record_ids[i])}: source={int(source_lengths[i])}, records={int(lengths[i])}")
    return lengths
