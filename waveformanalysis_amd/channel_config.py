"""Per-hardware-channel option overrides, resolved on the host into per-record SoA arrays.

Semantics follow the reference's layered plugin channel config
(waveform_analysis/core/hardware/channel.py:268-313,379-431):

    channel_config = {                       # optionally wrapped as {run_id: {...}}
        "defaults": {opt: value, ...},       # applies to every channel
        "groups":   [{"name":..., "channels": ["0:1", (0, 2)], "config": {...}}, ...]
                    or {name: {"channels": [...], "config": {...}}},
        "channels": {"0:3": {...}, (0, 4): {...}},   # or the same keys at top level
    }

Precedence: base option values < defaults < matching groups (in order) < the channel entry.
Channel keys are "board:channel" strings or (board, channel) pairs; anything else raises
ValueError("Invalid channel key ...") like the reference (channel.py:229-233).

The kernels never see this structure: plugins call `per_record_option` once per distinct
(board, channel) and scatter the result into a per-record array that is uploaded with the
records SoA.
"""

from __future__ import annotations

from collections.abc import Mapping, Sequence
from typing import Any

import numpy as np

_RESERVED = ("defaults", "groups", "channels")


def parse_channel_key(key: Any):
    """Return (board, channel) or None if `key` is not a channel reference."""
    if isinstance(key, (tuple, list)) and len(key) == 2:
        try:
            return int(key[0]), int(key[1])
        except (TypeError, ValueError):
            return None
    if hasattr(key, "board") and hasattr(key, "channel"):
        return int(key.board), int(key.channel)
    if isinstance(key, str) and ":" in key:
        left, right = key.strip().split(":", 1)
        try:
            return int(left.strip()), int(right.strip())
        except (TypeError, ValueError):
            return None
    return None


def _bad_key(key: Any) -> ValueError:
    return ValueError(
        f"Invalid channel key {key!r}; expected HardwareChannel, (board, channel), "
        'or "board:channel".'
    )


def _groups(block: Mapping) -> list[Mapping]:
    groups = block.get("groups")
    if isinstance(groups, Mapping):
        out = []
        for name, grp in groups.items():
            if isinstance(grp, Mapping):
                out.append(grp if "name" in grp else {"name": str(name), **grp})
        return out
    if isinstance(groups, Sequence) and not isinstance(groups, (str, bytes)):
        return [g for g in groups if isinstance(g, Mapping)]
    return []


def _selects(selectors: Any, hw: tuple[int, int]) -> bool:
    if not isinstance(selectors, Sequence) or isinstance(selectors, (str, bytes)):
        return False
    return any(parse_channel_key(item) == hw for item in selectors)


def resolve_channel_values(
    channel_config: Any,
    run_id: str,
    board: int,
    channel: int,
    base_values: Mapping[str, Any] | None = None,
) -> dict[str, Any]:
    """Effective option values for one hardware channel (channel.py:412-431)."""
    resolved: dict[str, Any] = dict(base_values or {})
    if not isinstance(channel_config, Mapping):
        return resolved
    block = channel_config
    if isinstance(block.get(run_id), Mapping):  # {run_id: {...}} wrapper
        block = block[run_id]
    resolved.update(_layer_values(block, (int(board), int(channel)), "config"))
    return resolved


def _layer_values(block: Mapping, hw: tuple[int, int], group_key: str) -> dict[str, Any]:
    """defaults < matching groups < the channel entry of one layer (channel.py:268-313); a group's values sit under
    `group_key`, with "config" as the fallback key."""
    resolved: dict[str, Any] = {}
    defaults = block.get("defaults")
    if isinstance(defaults, Mapping):
        resolved.update(defaults)
    for grp in _groups(block):
        if _selects(grp.get("channels"), hw):
            values = grp.get(group_key)
            if values is None and group_key != "config":
                values = grp.get("config")
            if isinstance(values, Mapping):
                resolved.update(values)

    chan_block = block.get("channels")
    if not isinstance(chan_block, Mapping):
        chan_block = block
    for key, values in chan_block.items():
        if isinstance(key, str) and key in _RESERVED:
            continue
        parsed = parse_channel_key(key)
        if parsed is None:
            raise _bad_key(key)
        if parsed != hw:
            continue
        if not isinstance(values, Mapping):
            raise ValueError(
                f"Invalid channel config for {key!r}; expected a mapping, got "
                f"{type(values).__name__}."
            )
        resolved.update(values)
        break
    return resolved


VALID_POLARITIES = ("positive", "negative")


def channel_metadata_layers(context: Any, run_id: str) -> list[Mapping]:
    """`channel_metadata` of the context config, then of the run config (channel.py:324-343)."""
    config = getattr(context, "config", {})
    base = config.get("channel_metadata") if isinstance(config, Mapping) else None
    run_config: Any = {}
    getter = getattr(context, "get_run_config", None)
    if callable(getter):
        try:
            run_config = getter(run_id)
        except Exception:
            run_config = {}
    override = run_config.get("channel_metadata") if isinstance(run_config, Mapping) else None
    return [layer for layer in (base, override) if isinstance(layer, Mapping)]


def metadata_polarity(layers: Sequence[Mapping], board: int, channel: int) -> str:
    """Polarity of one hardware channel from the metadata layers, later layers winning; anything but "positive" /
    "negative" is "unknown" (channel.py:192-210, 536-548)."""
    resolved: dict[str, Any] = {}
    for layer in layers:
        resolved.update(_layer_values(layer, (int(board), int(channel)), "metadata"))
    polarity = resolved.get("polarity", "unknown")
    return polarity if isinstance(polarity, str) and polarity in VALID_POLARITIES else "unknown"


def polarity_lookup(layers: Sequence[Mapping], boards: np.ndarray, channels: np.ndarray) -> dict[tuple[int, int], str]:
    """{(board, channel): polarity} over the distinct channels present (waveforms.py:293-314)."""
    if not layers or len(boards) == 0:
        return {}
    keys = np.unique(np.stack([np.asarray(boards, dtype=np.int64), np.asarray(channels, dtype=np.int64)], axis=1), axis=0)
    return {(int(b), int(c)): metadata_polarity(layers, int(b), int(c)) for b, c in keys}


def per_record_option(
    boards: np.ndarray,
    channels: np.ndarray,
    channel_config: Any,
    run_id: str,
    base_values: Mapping[str, Any],
) -> dict[tuple[int, int], dict[str, Any]]:
    """Resolve options once per distinct (board, channel) present in the records."""
    keys = np.stack([np.asarray(boards, dtype=np.int64), np.asarray(channels, dtype=np.int64)], axis=1)
    out: dict[tuple[int, int], dict[str, Any]] = {}
    for b, c in np.unique(keys, axis=0) if len(keys) else ():
        out[(int(b), int(c))] = resolve_channel_values(channel_config, run_id, int(b), int(c), base_values)
    return out


def scatter_per_record(
    boards: np.ndarray,
    channels: np.ndarray,
    per_channel: Mapping[tuple[int, int], Any],
    default: float,
    dtype=np.float64,
) -> np.ndarray:
    """Expand {(board, channel): value} into a per-record array."""
    boards = np.asarray(boards)
    channels = np.asarray(channels)
    out = np.full(len(boards), default, dtype=dtype)
    for (b, c), value in per_channel.items():
        out[(boards == b) & (channels == c)] = value
    return out


__all__ = [
    "parse_channel_key",
    "resolve_channel_values",
    "per_record_option",
    "scatter_per_record",
    "channel_metadata_layers",
    "metadata_polarity",
    "polarity_lookup",
]
