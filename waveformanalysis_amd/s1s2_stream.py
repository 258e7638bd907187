"""HipS1S2Stream -- the S1/S2 chain of the records route as a chunk stream.

The reference has no streaming form of `records + wave_pool -> wave_pool_filtered -> hit -> waveform_width -> s1_s2`
(basic_features on the side); its profiles.py names `streaming_default()` as not available yet.  Here one chunk of
records goes through that chain on one DeviceSession: the chunk's samples and records go up, the filter, the find_peaks
pass and the peak chain (wfa_peak_chain_count: features, widths, range cuts, compaction) run on the device, and only
the labelled S1_S2_CLASSIFIER_DTYPE rows come back.
"""

from __future__ import annotations

import weakref
from types import SimpleNamespace
from typing import Any

import numpy as np

from . import _lib
from .chunk import Chunk
from .device import DevicePool
from .dtypes import S1_S2_CLASSIFIER_DTYPE
from .filter_engine import FILTER_OPTION_NAMES, design_bw, plan_fused_groups, resolve_filter_key
from .plugin_api import Option
from .plugins import _common as K
from .plugins.basic_features import PEAK_RANGE, HipBasicFeaturesPlugin
from .plugins.hit_finder import _dt_values
from .plugins.s1_s2 import HipS1S2ClassifierPlugin, class_ranges
from .plugins.wave_pool_filtered import HipWavePoolFilteredPlugin
from .streaming import (HipStreamingPlugin, _RecordsChunking, _channel_keys, _filter_signature, given_options,
                        option_resolver)

HIT_OPTION_NAMES = ("use_derivative", "height", "distance", "prominence", "width", "threshold", "height_method",
                    "height_window_extension")
WIDTH_OPTION_NAMES = ("rise_low", "rise_high", "fall_high", "fall_low")
CLASS_OPTION_NAMES = tuple(HipS1S2ClassifierPlugin.options)
# (static plugin, option) the stream does not implement by default; filter_source="wave_pool_filtered" takes the first,
# baseline_source="basic_features" the second, the deprecated third stays outside
OUT_OF_SCOPE = (("wave_pool_filtered", "channel_config"), ("basic_features", "channel_config"),
                ("basic_features", "fixed_baseline"))
FILTER_SOURCES = ("own", "wave_pool_filtered")
BASELINE_SOURCES = ("records", "basic_features")


class _ChannelPlan:
    """The per-channel settings of one run: the sorted (board, channel) keys of its records, the filter group of each
    with the filter key of every group (`keys`; None: the stream's own filter), and the fixed baseline of each
    (`fixed_of_key`; None: no record of the run has one).  Immutable once resolved; worker threads share it."""

    def __init__(self, channel_key, group_of_key, keys, fixed_of_key):
        self.channel_key, self.group_of_key, self.keys, self.fixed_of_key = channel_key, group_of_key, keys, fixed_of_key
        self._designs: dict = {}

    @classmethod
    def resolve(cls, context: Any, run_id: str, fplugin: Any, channel_config: Any, tables: list) -> "_ChannelPlan":
        """fplugin: the wave_pool_filtered plugin whose settings the run takes (None: not asked for); channel_config:
        basic_features' (None: not asked for).  Groups are numbered in plan_filter_groups' order over the run's
        channels."""
        uniq = np.unique(np.concatenate([_channel_keys(t) for t in tables])) if tables else np.zeros(0, dtype=np.int64)
        channels = np.zeros(len(uniq), dtype=[("board", np.int16), ("channel", np.int16)])
        channels["board"] = uniq >> 16
        channels["channel"] = (uniq & 0xFFFF).astype(np.uint16).astype(np.int16)
        group, keys = np.zeros(len(uniq), dtype=np.int32), None
        if fplugin is not None:
            keys = []
            for g, (key, mask) in enumerate(plan_fused_groups(context, fplugin, run_id, channels)):
                keys.append(tuple(key))
                if mask is not None:
                    group[np.asarray(mask, dtype=bool)] = g
            if len(keys) > _lib.MAX_HIT_GROUPS:
                raise ValueError(f"s1_s2_stream: the run resolves to {len(keys)} distinct filter settings, the grouped "
                                 f"filter takes at most {_lib.MAX_HIT_GROUPS}")
        fixed = K.fixed_baseline_per_record(channels, channel_config, run_id) if len(uniq) else None
        return cls(uniq, group, keys, fixed)

    def lookup(self, records: np.ndarray):
        """(group_of_record int32, basic_features' fixed baseline per record: float64 with NaN = none, or None when the
        run has none) of a chunk's records, by one vectorised lookup."""
        key = _channel_keys(records)
        at = np.searchsorted(self.channel_key, key)
        at[at >= len(self.channel_key)] = 0
        if len(self.channel_key) == 0 or np.any(self.channel_key[at] != key):
            raise ValueError("s1_s2_stream: a chunk holds a (board, channel) the run's records do not")
        return self.group_of_key[at], None if self.fixed_of_key is None else self.fixed_of_key[at]

    def design(self, g: int):
        """("SG", window, order) or ("BW", sos, zi, padlen) of group g, a Butterworth group designed once."""
        key = self.keys[g]
        if key[0] == "SG":
            return key
        if g not in self._designs:
            self._designs[g] = ("BW",) + tuple(design_bw(*key[1:]))
        return self._designs[g]


class HipS1S2Stream(_RecordsChunking, HipStreamingPlugin):
    """compute_chunk() = the s1_s2 rows of one chunk of records.

    `compute(context, run_id)` streams over the static `records` array, chunked like hit_threshold_stream: `chunk_size`
    consecutive records of a time segment, nothing widened, nothing clipped (every stage of the chain depends on a
    peak's own record only).  Per chunk a session is borrowed from the device pool (the worker threads of
    `_compute_parallel` give the overlap of one chunk's upload with another's kernels) and runs
      upload_pool(slice) + upload_records(wave_offset and record_id rebased to the chunk)
      -> savgol / sosfiltfilt (use_filtered, nothing downloaded) -> find_peaks(download=False)
      -> peak_chain(record_id_base = the chunk's first id),
    so the rows of all chunks together are the rows of the static plugin chain under the same configuration, byte for
    byte, whatever the chunk size.  Options carry the static plugins' names and defaults (hit, wave_pool_filtered,
    waveform_width with `width_use_filtered` for its use_filtered, basic_features' ranges with `features_use_filtered`,
    s1_s2), read from the Context like theirs; a value given to the constructor wins.

    record_id.  The static chain reads the waveform of row record_id[i] (peak_finding.py:401-407), a chunk holds only
    its own rows: a `records` table whose record_id is not arange(len(records)) (or that has no such column) is refused
    with a ValueError before anything is uploaded, like records without `dt` when no `dt` option is given and a
    height_method outside minmax / diff.  The `dt` option is resolved before the records are cut into chunks.

    Per-channel settings.  `filter_source="wave_pool_filtered"` takes the filter settings the registered
    wave_pool_filtered plugin would apply per record (filter_type, SG / Butterworth parameters, its channel_config:
    filtering.py:339-374; a fresh HipWavePoolFilteredPlugin stands in when none is registered), resolved once per run
    with plan_filter_groups' rules and messages and cached on the records array and the configuration, as the hit
    stream's `_run_plan`.  Groups are numbered over the whole run; group g of a Savitzky-Golay setting uses the resident
    plan slot g of its session.  A chunk then runs, behind its two uploads and for every group that has a record in it,
    savgol_group(slot g) or sosfiltfilt_group(g) over the uploaded table (the find_peaks pass and the peak chain need the
    whole chunk's table resident), then find_peaks and peak_chain as before; a run that resolves to one setting takes the
    set_sg_plan + savgol / sosfiltfilt calls of the default path.  More than WFA_MAX_HIT_GROUPS settings, or a filter
    option given to the constructor beside this value, is a ValueError before anything is uploaded.
    `baseline_source="basic_features"` hands peak_chain the fixed baseline per record that the registered
    basic_features plugin's channel_config gives (K.fixed_baseline_per_record, cut to the chunk; nothing when no record
    of the run has one).  A pool upload drops the session's float32 twin, so a reused session never shows the filtered
    samples of an earlier chunk: the first group call of a chunk zeroes the twin.

    Out of scope: the deprecated basic_features.fixed_baseline option, the dense (st_waveforms) route, and a queued
    (non-blocking) form of the chain.  With both options at their defaults ("own", "records") a Context whose
    configuration sets wave_pool_filtered's channel_config or basic_features' channel_config / fixed_baseline is refused
    with a ValueError: the static chain would apply them, the stream as configured would not.  Each option lifts the
    refusal of the setting it implements."""

    provides = "s1_s2_stream"
    depends_on = ["records", "wave_pool"]
    description = "S1/S2 labelled peaks of the records stream, chunk by chunk (HIP, gfx950)."
    version = "0.1.0+hip1"
    output_dtype = S1_S2_CLASSIFIER_DTYPE
    save_when = "never"
    chunk_size = 50_000
    length_field = "event_length"
    output_data_kind = "peaks"

    options = {
        # hit
        "use_filtered": Option(default=True, type=bool, help="detect on the filtered samples"),
        "use_derivative": Option(default=True, type=bool, help="detect on the first difference"),
        "height": Option(default=30.0, type=float, help="minimum peak height"),
        "distance": Option(default=2, type=int, help="minimum distance between peaks (samples)"),
        "prominence": Option(default=0.7, type=float, help="minimum prominence"),
        "width": Option(default=4, type=int, help="minimum width at half prominence (samples)"),
        "threshold": Option(default=None, help="minimum vertical distance to the neighbours (optional)"),
        "height_method": Option(default="minmax", type=str, help="'diff' or 'minmax'"),
        "height_window_extension": Option(default=4, type=int, help="samples added either side of the peak window"),
        "dt": Option(default=None, type=int, help="sample interval (ns) when records lack dt"),
        # wave_pool_filtered, one setting per run
        "filter_type": Option(default="SG", type=str, help="'SG' (Savitzky-Golay) or 'BW' (Butterworth sosfiltfilt)"),
        "lowcut": Option(default=0.1, type=float, help="BW low cut"),
        "highcut": Option(default=0.5, type=float, help="BW high cut"),
        "fs": Option(default=0.5, type=float, help="BW sampling rate (GHz)"),
        "filter_order": Option(default=4, type=int, help="BW order"),
        "sg_window_size": Option(default=11, type=int, help="SG window (odd)"),
        "sg_poly_order": Option(default=2, type=int, help="SG polynomial order"),
        # waveform_width
        "width_use_filtered": Option(default=False, type=bool, help="measure widths on the filtered samples"),
        "sampling_rate": Option(default=None, type=float, help="sampling rate (GHz); 0.5 when unset"),
        "rise_low": Option(default=0.1, type=float, help="low fraction of the rise time"),
        "rise_high": Option(default=0.9, type=float, help="high fraction of the rise time"),
        "fall_high": Option(default=0.9, type=float, help="high fraction of the fall time"),
        "fall_low": Option(default=0.1, type=float, help="low fraction of the fall time"),
        "interpolation": Option(default=True, type=bool, help="linear interpolation of the crossings"),
        "filter_source": Option(default="own", type=str,
                                help="own (the filter options above, one setting per run) | wave_pool_filtered (the "
                                     "registered wave_pool_filtered plugin's settings per record)"),
        # basic_features
        "baseline_source": Option(default="records", type=str,
                                  help="records (every record's own baseline) | basic_features (the fixed_baseline of "
                                       "the registered basic_features plugin's channel_config)"),
        "height_range": Option(default=PEAK_RANGE, type=tuple, help="(start, end) for height"),
        "area_range": Option(default=(0, None), type=tuple, help="(start, end) for area; None = to the end"),
        "features_use_filtered": Option(default=False, type=bool, help="features of the filtered samples"),
        # s1_s2
        **HipS1S2ClassifierPlugin.options,
    }

    def __init__(self, device_pool: DevicePool | None = None, **given):
        super().__init__()
        self._given = given_options(self, given)
        self.device_pool = device_pool
        self._ids_of = None  # weak reference to the records array whose record_id column was checked last
        self._plan_of = None  # (weak reference to a records array, config signature, _ChannelPlan): _run_plan's last run
        self._configure(None)

    def _configure(self, context: Any) -> dict:
        """Constructor argument > Context configuration > option default; returns (and keeps) the resolved settings.
        Worker threads share the plugin: a chunk works on the dict it was handed, never on `self.cfg` again."""
        value = option_resolver(self, context)
        threshold = value("threshold")
        if threshold is not None and not np.isscalar(threshold):
            raise ValueError("s1_s2_stream takes a scalar threshold (a lower bound), or None")
        filter_source, baseline_source = str(value("filter_source")), str(value("baseline_source"))
        if filter_source not in FILTER_SOURCES:
            raise ValueError(f"s1_s2_stream: filter_source must be one of {FILTER_SOURCES}, got {filter_source!r}")
        if baseline_source not in BASELINE_SOURCES:
            raise ValueError(f"s1_s2_stream: baseline_source must be one of {BASELINE_SOURCES}, got {baseline_source!r}")
        contradicted = sorted(set(FILTER_OPTION_NAMES) & set(self._given))
        if filter_source == "wave_pool_filtered" and contradicted:
            raise ValueError(f"s1_s2_stream: {contradicted} given to the constructor contradict "
                             "filter_source='wave_pool_filtered' (the filter settings are that plugin's)")
        cfg = {
            "filter_source": filter_source,
            "baseline_source": baseline_source,
            "use_filtered": bool(value("use_filtered")),
            "peaks": dict(use_derivative=bool(value("use_derivative")), height=float(value("height")),
                          distance=int(value("distance")), prominence=float(value("prominence")),
                          width=int(value("width")),  # peak_finding.py:200 truncates to int
                          threshold=None if threshold is None else float(threshold),
                          height_method=str(value("height_method")),
                          height_window_extension=int(value("height_window_extension"))),
            "filter": {name: value(name) for name in FILTER_OPTION_NAMES},
            "width_source": _lib.SRC_F32 if bool(value("width_use_filtered")) else _lib.SRC_RAW,
            "feature_source": _lib.SRC_F32 if bool(value("features_use_filtered")) else _lib.SRC_RAW,
            "chain": dict(sampling_rate=0.5 if value("sampling_rate") is None else float(value("sampling_rate")),
                          interpolation=bool(value("interpolation")), height_range=tuple(value("height_range")),
                          area_range=tuple(value("area_range")),
                          **{name: float(value(name)) for name in WIDTH_OPTION_NAMES},
                          **{name: value(name) for name in CLASS_OPTION_NAMES}),
        }
        dt = self._given.get("dt")
        if dt is None and context is not None and hasattr(context, "config"):
            dt = K.resolve_dt_config(context, self, deprecated_keys=("sampling_interval_ns", "dt_ns"))
        cfg["dt"] = dt
        self.cfg = cfg
        return cfg

    # -- host-side refusals: before any upload ---------------------------------------------------------------
    def _check_run(self, cfg: dict, context: Any, run_id: str) -> None:
        if cfg["peaks"]["height_method"] not in ("minmax", "diff"):
            raise ValueError(f"不支持的峰高计算方法: {cfg['peaks']['height_method']}")  # peak_finding.py:612
        chain = cfg["chain"]
        class_ranges(strict=chain["strict"], **{k: chain[k] for k in CLASS_OPTION_NAMES if k.endswith("_range")})
        self._check_scope(context, cfg)
        records = context.get_data(run_id, "records") if hasattr(context, "get_data") else None
        if isinstance(records, np.ndarray) and records.dtype.names:
            seen = self._ids_of  # (one read: worker threads share the plugin)
            if seen is None or seen() is not records:
                self._check_ids(records, 0)
                self._ids_of = weakref.ref(records)

    @staticmethod
    def _check_scope(context: Any, cfg: dict | None = None) -> None:
        """What the static chain would read from this Context and the stream, as configured, does not apply: refused, so
        that one configuration never gives two tables."""
        if not isinstance(getattr(context, "config", None), dict):
            return
        taken = set()
        if cfg is not None and cfg["filter_source"] == "wave_pool_filtered":
            taken.add(OUT_OF_SCOPE[0])
        if cfg is not None and cfg["baseline_source"] == "basic_features":
            taken.add(OUT_OF_SCOPE[1])
        for provides, name in OUT_OF_SCOPE:
            if (provides, name) in taken:
                continue
            if K.raw_config(context, SimpleNamespace(provides=provides), name):
                raise ValueError(f"s1_s2_stream: the configuration sets {name!r} for {provides}; per-channel filter "
                                 "settings and fixed baselines of basic_features are outside the stream (the static "
                                 "chain would apply them)")

    @staticmethod
    def _check_ids(records: np.ndarray, first: int) -> None:
        if "record_id" not in (records.dtype.names or ()):
            raise ValueError("s1_s2_stream: records need a 'record_id' column equal to arange(len(records))")
        if not np.array_equal(records["record_id"], first + np.arange(len(records), dtype=np.int64)):
            raise ValueError("s1_s2_stream: records['record_id'] must be arange(len(records)): the static chain reads "
                             "the waveform of row record_id[i], a chunk holds only its own rows")

    @staticmethod
    def _filtered(cfg: dict) -> bool:
        """The filtered samples exist where a stage reads them: detection (use_filtered), widths, features."""
        return cfg["use_filtered"] or _lib.SRC_F32 in (cfg["width_source"], cfg["feature_source"])

    def _run_plan(self, cfg: dict, context: Any, run_id: str, chunk_records: np.ndarray | None = None):
        """None with both options at their defaults: nothing per record happens on the host.  Otherwise the run's
        _ChannelPlan, resolved once per run from the Context's `records` (cached on that array and the resolved
        configuration), else from the chunk at hand.  Raises what plan_filter_groups raises for a bad setting, and a
        ValueError for more than WFA_MAX_HIT_GROUPS distinct ones: before anything is uploaded."""
        grouped = cfg["filter_source"] == "wave_pool_filtered" and self._filtered(cfg)
        fixed = cfg["baseline_source"] == "basic_features"
        if not grouped and not fixed:
            return None
        plugins = getattr(context, "_plugins", {})
        fplugin = channel_config = None
        if grouped:
            fplugin = context.get_plugin("wave_pool_filtered") if "wave_pool_filtered" in plugins else HipWavePoolFilteredPlugin()
        if fixed:
            bplugin = context.get_plugin("basic_features") if "basic_features" in plugins else HipBasicFeaturesPlugin()
            channel_config = context.get_config(bplugin, "channel_config")
        signature = (run_id, _filter_signature(context, fplugin), repr(channel_config))
        records = context.get_data(run_id, "records") if hasattr(context, "get_data") else None
        if isinstance(records, np.ndarray) and records.dtype.names:
            seen = self._plan_of  # (one read: worker threads share the plugin)
            if seen is None or seen[0]() is not records or seen[1] != signature:
                seen = (weakref.ref(records), signature,
                        _ChannelPlan.resolve(context, run_id, fplugin, channel_config, [records]))
                self._plan_of = seen
            return seen[2]
        tables = [chunk_records] if chunk_records is not None and len(chunk_records) else []
        return _ChannelPlan.resolve(context, run_id, fplugin, channel_config, tables)

    def _get_input_chunks(self, context: Any, run_id: str, **kwargs):
        """The chunks of the Context's `records`, after the host-side refusals and with the `dt` option standing in for
        a missing `dt` column: the chunk rule reads dt (a record's end), so it is resolved before anything is cut."""
        records = context.get_data(run_id, "records")
        if not isinstance(records, np.ndarray):
            return super()._get_input_chunks(context, run_id, **kwargs)
        if records.dtype.names is None:
            raise TypeError(f"{self.provides} chunks the structured `records` array")
        cfg = self._configure(context)
        self._check_run(cfg, context, run_id)
        self._run_plan(cfg, context, run_id)
        if "dt" not in records.dtype.names:
            records = K.records_with_dt(records, _dt_values(records, cfg["dt"], "records"))
        return self._data_to_chunks(records, run_id)

    def _filter_design(self, cfg: dict):
        """("SG", window, order) or ("BW", sos, zi, padlen) of the run's one filter setting, with the reference's
        messages for a bad one (filtering.py:76-124)."""
        key = resolve_filter_key(cfg["filter"])
        return key if key[0] == "SG" else ("BW",) + tuple(design_bw(*key[1:]))

    def _empty(self, chunk: Chunk, run_id: str) -> Chunk:
        return Chunk(np.zeros(0, dtype=S1_S2_CLASSIFIER_DTYPE), chunk.start, chunk.end, run_id, self.provides,
                     data_kind=self.output_data_kind, time_field="timestamp", metadata=dict(chunk.metadata))

    def compute_chunk(self, chunk: Chunk, context: Any, run_id: str, **_kw) -> Chunk:
        recs = chunk.data
        if len(recs) == 0:
            return self._empty(chunk, run_id)
        cfg = self._configure(context)
        self._check_run(cfg, context, run_id)
        names = recs.dtype.names or ()
        first = int(recs["record_id"][0]) if "record_id" in names else 0
        self._check_ids(recs, first)
        dt_values = _dt_values(recs, cfg["dt"], "records")
        filtered = self._filtered(cfg)
        plan = self._run_plan(cfg, context, run_id, recs)
        design = groups = extra = None
        if filtered and (plan is None or plan.keys is None):
            design = self._filter_design(cfg)
        elif filtered and len(plan.keys) == 1:  # one setting for the run: the calls of the stream's own filter
            design = plan.design(0)
        if plan is not None:
            group_of_record, fixed = plan.lookup(recs)
            if filtered and design is None:  # several settings: one call per group
                groups = group_of_record
            if fixed is not None:
                extra = {"fixed_baseline": fixed}
        wave_pool = context.get_data(run_id, "wave_pool")
        K.pool_source(wave_pool, raw_only=True)
        # the slice of the pool from the chunk's first sample to its last (see HipThresholdHitStream._stage)
        lo = int(recs["wave_offset"].min())
        hi = int((recs["wave_offset"].astype(np.int64) + recs["event_length"]).max())
        sub = recs.copy() if "dt" in names else K.records_with_dt(recs, dt_values)
        sub["wave_offset"] -= lo
        sub["record_id"] -= first
        # a record that overlaps the chunk's end has peaks behind it: the result spans every record it came from
        end = max(int(chunk.end), int(self._endtime_of(sub, "timestamp").max()) + 1)
        if hi <= lo:  # records without samples have no peaks
            rows = np.zeros(0, dtype=S1_S2_CLASSIFIER_DTYPE)
        else:
            # worker threads come and go with every compute(): the session is borrowed for this chunk only
            with self._pool(context).borrow() as sess:
                sess.upload_pool(np.ascontiguousarray(wave_pool[lo:hi]))
                sess.upload_records(sub, 0.0)
                if design is not None and design[0] == "SG":
                    sess.set_sg_plan(design[1], design[2])
                    sess.savgol(download=False)
                elif design is not None:
                    sess.sosfiltfilt(*design[1:], download=False)
                elif groups is not None:
                    # every group with a record here, over the uploaded table: the chunk's table stays resident
                    for g in np.unique(groups):
                        d = plan.design(int(g))
                        if d[0] == "SG":
                            sess.store_sg_plan(int(g), d[1], d[2])  # (a slot that holds the pair is left alone)
                            sess.savgol_group(int(g), groups, int(g))
                        else:
                            sess.sosfiltfilt_group(*d[1:], groups, int(g))
                sess.find_peaks(_lib.SRC_F32 if cfg["use_filtered"] else _lib.SRC_RAW, download=False, **cfg["peaks"])
                rows = sess.peak_chain(cfg["width_source"], cfg["feature_source"], record_id_base=first, **cfg["chain"],
                                       **(extra or {}))
        return Chunk(rows, chunk.start, end, run_id, self.provides, data_kind=self.output_data_kind,
                     time_field="timestamp", metadata=dict(chunk.metadata))


__all__ = ["HipS1S2Stream"]
