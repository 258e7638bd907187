"""HipWaveformsPlugin -- drop-in for WaveformsPlugin (reference: waveform_analysis/core/plugins/builtin/cpu/waveforms.py
:971-1476): st_waveforms built from `raw_files` on the context's device session.

  vx2730: every file's delimiter and header rows sniffed on the host, the texts decoded on the GPU part by part into
          the session's sample arena, the baselines taken over the untruncated rows (k_baseline_mean), the packed rows
          written by k_st_pack (st_builder.build_st_waveforms_from_vx2730_files);
  v1725:  host header walk, the rows packed on the GPU straight from the file bytes
          (st_builder.build_st_waveforms_from_v1725_files).
Rows are in raw-file order (no sort) and come down in bounded batches through the pinned staging ring.
"""

from __future__ import annotations

from typing import Any

import numpy as np

from .. import st_builder as SB
from ..channel_config import channel_metadata_layers, polarity_lookup
from ..dtypes import create_record_dtype
from ..plugin_api import Option
from . import _common as K
from .records import _session

# FormatSpec.sampling_rate_hz of the adapters (utils/formats/vx2730.py, v1725.py) -> dt in ns
ADAPTER_RATE_HZ = {"vx2730": 500e6, "v1725": 250e6}


def _valid_baseline_samples(v) -> bool:
    return (v is None or isinstance(v, int)
            or (isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(x, int) for x in v)))


def resolve_st_dt_ns(context: Any, plugin: Any, adapter: str | None) -> int:
    """The `dt` option, then the deprecated keys, then the adapter's rate (WaveformStructConfig.get_dt_ns :563-579)."""
    dt_ns = K.resolve_dt_config(context, plugin, deprecated_keys=("dt_ns", "sampling_interval_ns"))
    if dt_ns is not None:
        dt_ns = int(dt_ns)
    else:
        rate = ADAPTER_RATE_HZ.get(adapter or "vx2730")
        dt_ns = int(round(1e9 / float(rate))) if rate else 1
    if dt_ns <= 0:
        dt_ns = 1
    if dt_ns > np.iinfo(np.int32).max:
        raise ValueError(f"dt_ns out of int32 range: {dt_ns}")
    return dt_ns


def _polarity_of(context: Any, run_id: str):
    """Per-row polarity from channel_metadata (`_apply_polarity_metadata` :317-349)."""
    layers = channel_metadata_layers(context, run_id)

    def of(boards: np.ndarray, channels: np.ndarray) -> np.ndarray:
        out = np.full(len(boards), "unknown", dtype="U8")
        for (board, channel), polarity in polarity_lookup(layers, boards, channels).items():
            if polarity != "unknown":
                out[(boards == board) & (channels == channel)] = polarity
        return out

    return of


class HipWaveformsPlugin(K.HipPlugin):
    """st_waveforms from raw files on the GPU.

    Instance attributes (not options: they do not change the output): part_bytes = CSV text per device decode call,
    pack_batch_bytes = bytes of packed rows per device batch."""

    provides = "st_waveforms"
    version = "0.10.0+hip1"
    depends_on: list = []
    uses_run_config = True
    save_when = "always"
    description = ("Extract waveforms from raw CSV files and structure them into NumPy structured arrays "
                   "(HIP, gfx950).")
    output_dtype = np.dtype(create_record_dtype(SB.DEFAULT_WAVE_LENGTH))
    part_bytes: int = 1 << 30
    pack_batch_bytes: int = SB.DEFAULT_PACK_BATCH_BYTES
    options = {
        "daq_adapter": Option(default="vx2730", type=str, help="DAQ adapter name (e.g., 'vx2730')"),
        "wave_length": Option(default=None, type=int,
                              help="Waveform length (number of sampling points). Automatically detect from the data "
                                   "when None。"),
        "dt": Option(default=None, type=int, help="Sampling interval in ns for st_waveforms.dt (None=auto from adapter)."),
        "n_jobs": Option(default=None, type=int, help="Accepted for compatibility; the HIP build does not use it.",
                         track=False),
        "use_process_pool": Option(default=False, type=bool,
                                   help="Accepted for compatibility; the HIP build does not use it.", track=False),
        "chunksize": Option(default=None, type=int, help="Accepted for compatibility; the HIP build does not use it.",
                            track=False),
        "parse_engine": Option(default="auto", type=str,
                               help="Accepted for compatibility; the CSV text is decoded on the GPU.", track=False),
        "use_upstream_baseline": Option(default=False, type=bool,
                                        help="Whether to use baseline from upstream plugin (requires 'baseline' data)."),
        "baseline_samples": Option(
            default=None, type=None, validate=_valid_baseline_samples,
            help="Baseline range: int (sample count from adapter start) or tuple (start, end) relative to "
                 "samples_start. JSON lists like [0, 800] are also accepted. None=adapter default."),
        "streaming_mode": Option(default=False, type=bool,
                                 help="Reference streaming branch: polarity left empty, baseline_upstream NaN "
                                      "(no memmap here).", track=False),
    }

    def __init__(self, part_bytes: int | None = None, pack_batch_bytes: int | None = None):
        super().__init__()
        if part_bytes is not None:
            self.part_bytes = int(part_bytes)
        if pack_batch_bytes is not None:
            self.pack_batch_bytes = int(pack_batch_bytes)

    def resolve_depends_on(self, context: Any, run_id: str | None = None) -> list[str]:
        """:1054-1075: raw_files, plus baseline with use_upstream_baseline."""
        deps = ["raw_files"]
        if context.get_config(self, "use_upstream_baseline"):
            deps.append("baseline")
        return deps

    def get_lineage(self, context: Any) -> dict:
        """:1088-1109: the dtype is that of the configured wave_length (DEFAULT_WAVE_LENGTH when None)."""
        config = {}
        for key in self.config_keys:
            option = self.options.get(key)
            if option and getattr(option, "track", True):
                config[key] = context.get_config(self, key)
        wave_length = config.get("wave_length")
        lineage = {
            "plugin_class": self.__class__.__name__,
            "plugin_version": getattr(self, "version", "0.0.0"),
            "description": getattr(self, "description", ""),
            "config": config,
            "depends_on": {dep: context.get_lineage(dep) for dep in self.resolve_depends_on(context)},
        }
        wl = SB.DEFAULT_WAVE_LENGTH if wave_length is None else int(wave_length)
        lineage["dtype"] = np.dtype(create_record_dtype(wl)).descr
        return lineage

    def compute(self, context: Any, run_id: str, **kwargs) -> np.ndarray:
        raw_files = context.get_data(run_id, "raw_files")
        adapter = context.get_config(self, "daq_adapter")
        adapter = adapter.lower() if isinstance(adapter, str) else None
        wave_length = context.get_config(self, "wave_length")
        dt_ns = resolve_st_dt_ns(context, self, adapter)
        use_upstream = context.get_config(self, "use_upstream_baseline")
        baseline_samples = context.get_config(self, "baseline_samples")
        streaming = bool(context.get_config(self, "streaming_mode"))
        if adapter not in (None, "vx2730", "v1725"):
            raise ValueError(f"st_waveforms (HIP backend) reads vx2730 CSV or v1725 binary files, not {adapter!r}")
        if not raw_files:
            self.output_dtype = create_record_dtype(SB.DEFAULT_WAVE_LENGTH if wave_length is None else int(wave_length))
            return np.zeros(0, dtype=self.output_dtype)
        polarity_of = _polarity_of(context, run_id)
        if adapter == "v1725":
            seen, paths = set(), []
            for group in raw_files:
                for path in group or ():
                    if path not in seen:
                        seen.add(path)
                        paths.append(path)
            out = SB.build_st_waveforms_from_v1725_files(paths, wave_length=wave_length, dt_ns=dt_ns,
                                                         polarity_of=polarity_of, session=_session(context),
                                                         pack_batch_bytes=self.pack_batch_bytes)
            self.output_dtype = out.dtype
            return out
        upstream = None
        if use_upstream and not streaming:
            try:
                upstream = context.get_data(run_id, "baseline")
            except Exception:   # the reference logs a warning and fills NaN
                upstream = None
        out = SB.build_st_waveforms_from_vx2730_files(
            raw_files, wave_length=wave_length, dt_ns=dt_ns, baseline_samples=baseline_samples,
            polarity_of=polarity_of, streaming=streaming, upstream_baselines=upstream, session=_session(context),
            part_bytes=self.part_bytes, pack_batch_bytes=self.pack_batch_bytes)
        self.output_dtype = out.dtype
        return out


__all__ = ["HipWaveformsPlugin", "resolve_st_dt_ns"]
