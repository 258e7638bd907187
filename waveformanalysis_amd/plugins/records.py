"""HipRecordsPlugin / HipWavePoolPlugin -- drop-ins for RecordsPlugin / WavePoolPlugin
(reference: waveform_analysis/core/plugins/builtin/cpu/records.py:204-332; bundle assembly :119-201, shared bundle
`get_records_bundle` :441).

Both products come from one bundle per run, built from `raw_files` on the context's device session:
  vx2730: CSV text decoded on the GPU part by part into the session's sample arena, one device sort over all rows,
          one gather into the packed wave_pool (records_builder.build_records_from_vx2730_files with part_bytes);
  v1725:  host header walk, then the payloads gathered on the GPU straight from the file bytes
          (records_builder.build_records_from_v1725_files).
The gathered pool stays on the device as the session's resident wave_pool, so the records-route plugins that follow
on the same thread (hit_threshold, basic_features, ...) find it there and skip their upload.
"""

from __future__ import annotations

import os
from typing import Any

import numpy as np

from .. import records_builder as RB
from ..channel_config import channel_metadata_layers, polarity_lookup
from ..dtypes import RECORDS_DTYPE
from ..plugin_api import Option
from . import _common as K

_BUNDLE_CACHE_NAME = "_records_bundle"
DEFAULT_PART_BYTES = 1 << 30   # CSV text per device decode call
# adapter sampling rates (utils/formats/vx2730.py:101, v1725.py:220) -> dt in ns
ADAPTER_DT_NS = {"vx2730": 2, "v1725": 4}


def get_records_bundle_cache_key(context: Any, run_id: str) -> str:
    """records.py:30-38."""
    data_name = "records"
    plugins = getattr(context, "_plugins", {})
    if data_name not in plugins and "wave_pool" in plugins:
        data_name = "wave_pool"
    return f"{_BUNDLE_CACHE_NAME}-{context.key_for(run_id, data_name)}"


def _cleanup_stale_bundles(context: Any, run_id: str, keep_key: str) -> None:
    """records.py:102-116."""
    stale = [(rid, name) for (rid, name), value in context._results.items()
             if rid == run_id and name != keep_key and isinstance(value, RB.RecordsBundle)
             and name.startswith(_BUNDLE_CACHE_NAME)]
    for key in stale:
        del context._results[key]


def resolve_dt_ns(context: Any, plugin: Any, adapter_name: str | None = None) -> int:
    """records.py:66-88: the `dt` option, the deprecated keys, the adapter's sampling rate, else 1."""
    dt_ns = K.resolve_dt_config(context, plugin, deprecated_keys=("records_dt_ns", "dt_ns", "sampling_interval_ns"))
    if dt_ns is None:
        daq_adapter = adapter_name or context.config.get("daq_adapter")
        if isinstance(daq_adapter, str):
            dt_ns = ADAPTER_DT_NS.get(daq_adapter.lower())
    if dt_ns is None:
        dt_ns = 1
    if dt_ns > np.iinfo(np.int32).max or dt_ns < 0:
        raise ValueError(f"records_dt_ns out of int32 range: {dt_ns}")
    return int(dt_ns)


def resolve_adapter_name(context: Any, plugin: Any) -> str | None:
    """records.py:91-99."""
    adapter = None
    if plugin is not None and "daq_adapter" in plugin.options:
        adapter = context.get_config(plugin, "daq_adapter")
    if adapter is None:
        adapter = context.config.get("daq_adapter")
    return adapter.lower() if isinstance(adapter, str) else None


def file_epoch_ns(path: str) -> int:
    """DAQAdapter.get_file_epoch (utils/formats/adapter.py:312-329)."""
    stat = os.stat(path)
    return int(getattr(stat, "st_birthtime", stat.st_mtime) * 1e9)


def apply_records_polarity(context: Any, run_id: str, records: np.ndarray) -> np.ndarray:
    """records.py:40-63: every record "unknown", then the channel_metadata polarity of its (board, channel)."""
    if len(records) == 0:
        return records
    records["polarity"] = "unknown"
    lookup = polarity_lookup(channel_metadata_layers(context, run_id), records["board"], records["channel"])
    for (board, channel), polarity in lookup.items():
        if polarity != "unknown":
            records["polarity"][(records["board"] == board) & (records["channel"] == channel)] = polarity
    return records


def _session(context: Any):
    """The session resident_session() of the records-route plugins uses on this thread."""
    return K.note_session(K._device_pool(context).session())


def _build_bundle(context: Any, run_id: str, plugin: Any, adapter_name: str | None, dt_ns: int) -> RB.RecordsBundle:
    """records.py:119-201, on the context's device session."""
    cache_key = get_records_bundle_cache_key(context, run_id)
    cached = context._results.get((run_id, cache_key))
    if isinstance(cached, RB.RecordsBundle):
        _cleanup_stale_bundles(context, run_id, cache_key)
        return cached

    raw_files = context.get_data(run_id, "raw_files")
    if adapter_name == "v1725":
        seen, paths = set(), []
        for group in raw_files:
            for path in group or ():
                if path not in seen:
                    seen.add(path)
                    paths.append(path)
        bundle = RB.build_records_from_v1725_files(paths, dt_ns=dt_ns, session=_session(context))
    else:
        if not isinstance(raw_files, list):
            raise ValueError("records expects raw_files as a list of per-channel file groups")
        if adapter_name not in (None, "vx2730"):
            raise ValueError(f"records (HIP backend) reads vx2730 CSV or v1725 binary files, not {adapter_name!r}")
        baseline_samples = context.get_config(plugin, "baseline_samples")
        RB._baseline_window(baseline_samples, 0, 0, 1)   # the reference's _validate_baseline_samples messages
        epoch_ns = None
        if adapter_name:
            first_file = next((group[0] for group in raw_files if group), None)
            if first_file is not None:
                try:
                    epoch_ns = file_epoch_ns(first_file)
                except (FileNotFoundError, OSError):
                    epoch_ns = None
        part_bytes = getattr(plugin, "part_bytes", None) or DEFAULT_PART_BYTES
        bundle = RB.build_records_from_vx2730_files(raw_files, default_dt_ns=dt_ns, baseline_samples=baseline_samples,
                                                    epoch_ns=epoch_ns, session=_session(context),
                                                    part_bytes=part_bytes)
    apply_records_polarity(context, run_id, bundle.records)
    context._set_data(run_id, cache_key, bundle)
    _cleanup_stale_bundles(context, run_id, cache_key)
    return bundle


def get_records_bundle(context: Any, run_id: str) -> RB.RecordsBundle:
    """records.py:441-470."""
    try:
        plugin = context.get_plugin("records")
    except Exception:
        plugin = context.get_plugin("wave_pool")
    adapter_name = resolve_adapter_name(context, plugin)
    dt_ns = resolve_dt_ns(context, plugin, adapter_name=adapter_name)
    return _build_bundle(context, run_id, plugin, adapter_name, dt_ns)


def _valid_baseline_samples(v) -> bool:
    return (v is None or isinstance(v, int)
            or (isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(x, int) for x in v)))


class _HipRecordsBundlePluginBase(K.HipPlugin):
    """Options, dependencies and lineage of _RecordsBundlePluginBase (records.py:209-305).

    part_bytes (instance attribute, not an option: it does not change the output): CSV text per device decode
    call, DEFAULT_PART_BYTES when None."""

    uses_run_config = True
    save_when = "always"
    part_bytes: int | None = None
    options = {
        "daq_adapter": Option(default="vx2730", type=str,
                              help="DAQ adapter name for records bundle (e.g., 'vx2730', 'v1725')."),
        "channel_workers": Option(default=None, help="Workers for channel-level waveform loading (None=auto).",
                                  track=False),
        "channel_executor": Option(default="thread", type=str,
                                   help="Channel-level executor type: 'thread' or 'process'.", track=False),
        "n_jobs": Option(default=None, type=int, help="Workers per channel for file-level parsing (None=auto).",
                         track=False),
        "use_process_pool": Option(default=False, type=bool,
                                   help="Use a process pool for file-level parsing (False=thread pool).", track=False),
        "chunksize": Option(default=None, type=int,
                            help="CSV read chunk size; None reads full file (PyArrow if available).", track=False),
        "parse_engine": Option(default="auto", type=str, help="CSV engine: auto | polars | pyarrow | pandas",
                               track=False),
        "records_part_size": Option(default=250_000, type=int, help="Max events per records shard; <=0 disables sharding."),
        "dt": Option(default=None, type=int,
                     help="Sample interval in ns for records.dt (defaults to adapter rate or 1ns)."),
        "baseline_samples": Option(
            default=None, type=None, validate=_valid_baseline_samples,
            help="Baseline range: int (sample count from adapter start) or tuple (start, end) "
                 "relative to samples_start. JSON lists like [0, 800] are also accepted. None=adapter default."),
    }
    version = "0.10.0+hip1"
    depends_on = ["raw_files"]

    def __init__(self, part_bytes: int | None = None):
        super().__init__()
        if part_bytes is not None:
            self.part_bytes = int(part_bytes)

    def resolve_depends_on(self, context: Any, run_id: str | None = None) -> list[str]:
        return ["raw_files"]

    def get_lineage(self, context: Any) -> dict:
        adapter_name = resolve_adapter_name(context, self)
        config = {}
        for key in self.config_keys:
            option = self.options.get(key)
            if option and getattr(option, "track", True):
                config[key] = context.get_config(self, key)
        if adapter_name:
            config["daq_adapter"] = adapter_name
        return {
            "plugin_class": self.__class__.__name__,
            "plugin_version": getattr(self, "version", "0.0.0"),
            "description": getattr(self, "description", ""),
            "config": config,
            "depends_on": {dep: context.get_lineage(dep) for dep in self.resolve_depends_on(context)},
            "dtype": np.dtype(self.output_dtype).descr,
        }


class HipRecordsPlugin(_HipRecordsBundlePluginBase):
    """records (event index table) from the shared bundle, built on the GPU."""

    provides = "records"
    description = "Build records (event index table) from the shared internal records bundle (HIP, gfx950)."
    output_dtype = RECORDS_DTYPE

    def compute(self, context: Any, run_id: str, **kwargs) -> np.ndarray:
        return get_records_bundle(context, run_id).records


class HipWavePoolPlugin(_HipRecordsBundlePluginBase):
    """wave_pool from the shared bundle; it stays resident on the device session after the build."""

    provides = "wave_pool"
    description = "Build wave_pool from the shared internal records bundle (HIP, gfx950)."
    output_dtype = np.dtype(np.uint16)

    def compute(self, context: Any, run_id: str, **kwargs) -> np.ndarray:
        return get_records_bundle(context, run_id).wave_pool


__all__ = ["HipRecordsPlugin", "HipWavePoolPlugin", "get_records_bundle", "get_records_bundle_cache_key",
           "resolve_dt_ns", "apply_records_polarity"]
