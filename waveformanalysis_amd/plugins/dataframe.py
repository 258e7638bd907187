"""HipDataFramePlugin -- drop-in for DataFramePlugin
(reference: waveform_analysis/core/plugins/builtin/cpu/dataframe.py:31-311).

One row per record (records branch) or per st_waveforms / filtered_waveforms row (dense branch), joined with the
basic_features row of the same index.  No waveform samples are read, so this stage is host table work with no kernel:
the columns are copied into a DataFrame, the per-channel gains are looked up once per distinct (board, channel) and
scattered with one `np.unique` inverse (the reference loops over every row in Python), and the table is sorted by
timestamp.
"""

from __future__ import annotations

import logging
import warnings
from collections.abc import Mapping
from typing import Any

import numpy as np

from ..channel_config import parse_channel_key
from ..plugin_api import Option, Plugin
from . import _common as K

logger = logging.getLogger(__name__)


def _channel_key_error(key: Any) -> ValueError:
    return ValueError(f"Invalid channel key {key!r}; expected HardwareChannel, (board, channel), "
                      'or "board:channel".')


def _normalize_gain_map(gain_adc_per_pe: Any) -> dict:
    """dataframe.py:78-104: warn about entries that are not positive numbers, keep the map as it is."""
    if not isinstance(gain_adc_per_pe, dict):
        return {}
    for channel, gain in gain_adc_per_pe.items():
        try:
            gain_float = float(gain)
        except (TypeError, ValueError):
            logger.warning("df.gain_adc_per_pe has invalid entry: channel=%r, gain=%r", channel, gain)
            continue
        if gain_float <= 0:
            logger.warning("df.gain_adc_per_pe[%s]=%s is non-positive; calibrated columns will be NaN for this channel",
                           channel, gain_float)
    return dict(gain_adc_per_pe)


def _extract_gain_from_run_config(run_config: Any) -> Any:
    """dataframe.py:106-120: calibration.gain_adc_per_pe, then the top-level gain_adc_per_pe."""
    if not isinstance(run_config, dict):
        return None
    calibration = run_config.get("calibration")
    if isinstance(calibration, dict) and isinstance(calibration.get("gain_adc_per_pe"), dict):
        return calibration.get("gain_adc_per_pe")
    if isinstance(run_config.get("gain_adc_per_pe"), dict):
        return run_config.get("gain_adc_per_pe")
    return None


def resolve_gain_map(channel_config: Any, run_id: str, have_channels: bool, plugin_name: str = "df",
                     value_name: str = "gain_adc_per_pe") -> dict[tuple[int, int], float]:
    """{(board, channel): gain} of a "board:channel"-keyed map, optionally wrapped as {run_id: {...}} and / or
    {"channels": {...}} (reference core/hardware/channel.py:571-619).  Entries that are not positive numbers are
    dropped with one warning; a key that is not a channel reference raises."""
    if not have_channels or channel_config is None:
        return {}
    if not isinstance(channel_config, Mapping):
        warnings.warn(f"Plugin '{plugin_name}' run '{run_id}': channel config must be dict-like, "
                      f"cannot resolve '{value_name}'.", UserWarning, stacklevel=3)
        return {}
    selected = channel_config
    run_block = selected.get(run_id)
    if isinstance(run_block, Mapping):
        selected = run_block
    if isinstance(selected.get("channels"), Mapping):
        selected = selected["channels"]
    values: dict[tuple[int, int], float] = {}
    invalid: list[str] = []
    for key, raw_value in selected.items():
        hw = parse_channel_key(key)
        if hw is None:
            raise _channel_key_error(key)
        if isinstance(raw_value, Mapping):
            raw_value = raw_value.get(value_name)
        try:
            value = float(raw_value)
        except (TypeError, ValueError):
            if raw_value is not None:
                invalid.append(f"board{hw[0]}:ch{hw[1]}")
            continue
        if value_name == "gain_adc_per_pe" and value <= 0:
            invalid.append(f"board{hw[0]}:ch{hw[1]}")
            continue
        values[hw] = value
    if invalid:
        warnings.warn(f"Plugin '{plugin_name}' run '{run_id}': invalid '{value_name}' entries -> "
                      + ", ".join(sorted(invalid)), UserWarning, stacklevel=3)
    return values


def gains_per_row(gain_map: dict[tuple[int, int], float], boards: np.ndarray, channels: np.ndarray) -> np.ndarray:
    """float64 gain of every row, NaN where (board, channel) has no entry: one lookup per distinct pair."""
    n = len(channels)
    if n == 0 or not gain_map:
        return np.full(n, np.nan, dtype=np.float64)
    key = np.asarray(boards, dtype=np.int64) * 65536 + (np.asarray(channels, dtype=np.int64) & 0xFFFF)
    uniq, inverse = np.unique(key, return_inverse=True)
    per_key = np.full(len(uniq), np.nan, dtype=np.float64)
    for k, kv in enumerate(uniq.tolist()):
        hw = (kv >> 16, int(np.int16(np.uint16(kv & 0xFFFF))))
        if hw in gain_map:
            per_key[k] = gain_map[hw]
    return per_key[inverse.reshape(-1)]


class HipDataFramePlugin(Plugin):
    """Build the single-channel events DataFrame (timestamp, record_id, area, height, amp, max_abs_diff, board,
    channel, and area_pe / height_pe when a gain map is configured).

    Gain map precedence: the explicit `gain_adc_per_pe` option, then the run config's
    `calibration.gain_adc_per_pe`, then its top-level `gain_adc_per_pe`, then none (no calibrated columns).
    The final sort by timestamp is stable here; the reference's `sort_values("timestamp")` is not, so rows with
    equal timestamps may come out in another order there.
    """

    provides = "df"
    depends_on = []  # dynamic, see resolve_depends_on
    description = "Build the initial single-channel events DataFrame."
    version = "1.7.0+hip1"
    save_when = "always"
    uses_run_config = True
    options = {
        "use_filtered": Option(default=False, type=bool, help="use filtered_waveforms"),
        "wave_source": Option(default=K.WAVE_SOURCE_AUTO, type=str,
                              help="auto|records|st_waveforms|filtered_waveforms"),
        "gain_adc_per_pe": Option(default=None, type=dict,
                                  help='ADC/PE gain per hardware channel, keys "board:channel", e.g. '
                                       '{"0:0": 12.5, "0:1": 13.2}; adds the area_pe / height_pe columns'),
    }

    def resolve_depends_on(self, context: Any, run_id: str | None = None) -> list[str]:
        kind, deps, _ = K.resolve_wave_input(context, self)
        deps = [K.WAVE_SOURCE_RECORDS] if kind == "records" else list(deps)  # no samples are read
        return deps + ["basic_features"]

    @staticmethod
    def _basic_features_is_records(context: Any) -> tuple[bool, str]:
        from .basic_features import HipBasicFeaturesPlugin

        bf = HipBasicFeaturesPlugin()
        kind, _, _ = K.resolve_wave_input(context, bf)
        return kind == "records", K.normalize_wave_source(K._cfg(context, bf, "wave_source"))

    def _resolve_gain_map(self, context: Any, run_id: str, have_channels: bool) -> tuple[dict, bool]:
        """dataframe.py:122-195: (gain map, emit calibrated columns)."""
        gain = context.get_config(self, "gain_adc_per_pe")
        explicit = False
        has_explicit = getattr(context, "has_explicit_config", None)
        if callable(has_explicit):
            try:
                explicit = bool(has_explicit(self, "gain_adc_per_pe"))
            except Exception:
                explicit = False
        if explicit:
            if isinstance(gain, dict):
                return resolve_gain_map(_normalize_gain_map(gain), run_id, have_channels), bool(gain)
            return {}, False
        if isinstance(gain, dict) and gain:
            return resolve_gain_map(_normalize_gain_map(gain), run_id, have_channels), True
        getter = getattr(context, "get_run_config", None)
        if callable(getter):
            try:
                run_gain = _extract_gain_from_run_config(getter(run_id))
                if isinstance(run_gain, dict):
                    return resolve_gain_map(_normalize_gain_map(run_gain), run_id, have_channels), bool(run_gain)
            except Exception as exc:
                logger.warning("Failed to resolve gain from run config for run '%s': %s", run_id, exc)
        return {}, False

    def compute(self, context: Any, run_id: str, **kwargs) -> Any:
        import pandas as pd

        basic_features = context.get_data(run_id, "basic_features")
        kind, _, data_name = K.resolve_wave_input(context, self)
        if kind == "records":  # the records table alone: no samples, no pool
            plugins = getattr(context, "_plugins", None)
            if isinstance(plugins, dict) and plugins and "records" not in plugins and \
                    "records" not in getattr(context, "_data", {}):
                raise KeyError("df requires 'records' but it is not registered. Register RecordsPlugin to provide "
                               "'records'.")
            table = context.get_data(run_id, "records")
            if not isinstance(table, np.ndarray):
                raise ValueError("df expects records as a single structured array")
        else:
            table = K.load_dense_input(context, self, run_id, data_name)
        if not isinstance(basic_features, np.ndarray):
            raise ValueError("df expects basic_features as a single structured array")

        names = table.dtype.names or ()
        n = len(table)
        if kind == "records":
            bf_records, bf_source = self._basic_features_is_records(context)
            if not bf_records:
                raise ValueError("df.wave_source=records requires basic_features.wave_source=records "
                                 f"(resolved as {bf_source!r}).")
            if n != len(basic_features):
                raise ValueError(f"basic_features length ({len(basic_features)}) != records length ({n})")
            channel = np.asarray(table["channel"]) if "channel" in names else np.zeros(n, dtype=np.int16)
        else:
            if n != len(basic_features):
                raise ValueError(f"basic_features length ({len(basic_features)}) != {data_name} length ({n})")
            channel = np.asarray(table["channel"])
        board = np.asarray(table["board"]) if "board" in names else np.zeros(n, dtype=np.int16)
        df = pd.DataFrame({
            "timestamp": np.asarray(table["timestamp"]),
            "record_id": (np.asarray(table["record_id"], dtype=np.int64) if "record_id" in names
                          else np.arange(n, dtype=np.int64)),
            "area": np.asarray(basic_features["area"]),
            "height": np.asarray(basic_features["height"]),
            "amp": np.asarray(basic_features["amp"]),
            "max_abs_diff": np.asarray(basic_features["max_abs_diff"]),
            "board": board,
            "channel": channel,
        })
        gain_map, calibrated = self._resolve_gain_map(context, run_id, n > 0)
        if calibrated:
            gains = gains_per_row(gain_map, board, channel)
            df["area_pe"] = np.asarray(df["area"], dtype=np.float64) / gains
            df["height_pe"] = np.asarray(df["height"], dtype=np.float64) / gains
        return df.sort_values("timestamp", kind="stable")


__all__ = ["HipDataFramePlugin", "resolve_gain_map", "gains_per_row"]
