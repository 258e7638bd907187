"""Generate tests/golden/legacy_events_df.npz from the reference's DataFramePlugin, GroupedEventsPlugin and PairedEventsPlugin
(waveform_analysis/core/plugins/builtin/cpu/dataframe.py, event_analysis.py).  Run where the reference package is
importable, as make_golden.py is:

    python tests/golden/make_events_golden.py

Every case runs the three plugins through a minimal context (config lookup plugin-nested > global > default,
get_run_config, has_explicit_config) on small synthetic tables: clusters of 1-5 rows over 16 channels on two boards,
all timestamps distinct and the channels of every event distinct (the reference's sorts are unstable).  Stored, as arrays only, per case and product
("<case>/<product>/..."): column names and dtypes as strings, the index, every scalar column, and every ragged column
flattened with its offsets.  Inputs and each case's config (JSON text) are stored too, and "err/<name>" holds the
expected error texts.
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from waveform_analysis.core.plugins.builtin.cpu.dataframe import DataFramePlugin  # noqa: E402
from waveform_analysis.core.plugins.builtin.cpu.event_analysis import (  # noqa: E402
    GroupedEventsPlugin,
    PairedEventsPlugin,
)

OUT = os.path.join(REPO, "tests", "golden", "legacy_events_df.npz")
RUN_ID = "run_0"


class Ctx:
    """The slice of Context the three plugins read."""

    def __init__(self, config, data, run_config=None, explicit=()):
        self.config = dict(config)
        self._data = dict(data)
        self._results = {}
        self._run_config = run_config
        self._explicit = set(explicit)
        # (not `_plugins`: the reference checks that one for the registration of its inputs, which come from _data)
        self._registry = {p.provides: p for p in (DataFramePlugin(), GroupedEventsPlugin(), PairedEventsPlugin())}

    def get_config(self, plugin, name):
        block = self.config.get(plugin.provides)
        if isinstance(block, dict) and name in block:
            return block[name]
        if name in self.config:
            return self.config[name]
        opt = plugin.options.get(name)
        return None if opt is None else opt.default

    def has_explicit_config(self, plugin, name):
        return (plugin.provides, name) in self._explicit

    def get_run_config(self, run_id):
        return self._run_config if self._run_config is not None else {}

    def get_data(self, run_id, name):
        if name in self._results:
            return self._results[name]
        if name in self._data:
            return self._data[name]
        value = self._registry[name].compute(self, run_id)
        self._results[name] = value
        return value


def make_tables(seed: int, n_clusters: int):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 6, n_clusters)
    gaps = rng.integers(20_000, 600_000, n_clusters)                 # ps between cluster starts
    gaps[::3] = 6_000_000      # a 5000 ns window spans at most three clusters (<= 15 rows)
    starts = 10_000_000 + np.cumsum(gaps)
    ts = []
    for s, k in zip(starts, sizes):
        ts.extend(s + np.sort(rng.choice(180_000, size=k, replace=False)))
    ts = np.asarray(ts, dtype=np.int64)
    assert len(np.unique(ts)) == len(ts)
    n = len(ts)
    # channel = time rank mod 16: the rows of an event (a run in time order, <= 16 rows) have distinct channels, so
    # the reference's unstable channel sort has one answer; the wrap-around still reorders events by channel
    channel = (np.arange(n) % 16).astype(np.int16)
    perm = rng.permutation(n)                                           # input order is not time order
    ts, channel = ts[perm], channel[perm]
    board = rng.integers(0, 2, n).astype(np.int16)
    record_id = rng.permutation(n).astype(np.int64) + 1000
    rec = np.zeros(n, dtype=[("timestamp", "i8"), ("board", "i2"), ("channel", "i2"), ("record_id", "i8")])
    rec["timestamp"], rec["board"], rec["channel"], rec["record_id"] = ts, board, channel, record_id
    bf = np.zeros(n, dtype=[("height", "f4"), ("amp", "f4"), ("area", "f4"), ("max_abs_diff", "f4")])
    bf["height"] = rng.uniform(5, 400, n).astype(np.float32)
    bf["amp"] = rng.uniform(5, 500, n).astype(np.float32)
    bf["area"] = rng.uniform(-50, 4000, n).astype(np.float32)
    bf["max_abs_diff"] = rng.uniform(0, 90, n).astype(np.float32)
    return rec, bf


def drop_field(a: np.ndarray, name: str) -> np.ndarray:
    keep = [f for f in a.dtype.names if f != name]
    out = np.zeros(len(a), dtype=[(f, a.dtype[f]) for f in keep])
    for f in keep:
        out[f] = a[f]
    return out


GAIN_ALL = {f"{b}:{c}": 10.0 + b * 3.5 + c * 0.25 for b in range(2) for c in range(16)}
GAIN_PARTIAL = {"0:1": 12.5, "0:2": -3.0, "1:7": "bad", (1, 3): 20.0, "0:5": {"gain_adc_per_pe": 8.0}}
GAIN_RUN = {"calibration": {"gain_adc_per_pe": {"0:0": 11.0, "0:3": 9.5, "1:15": 30.0}}}
GAIN_RUN_TOP = {"gain_adc_per_pe": {"channels": {"1:1": 14.0, "0:4": 16.0}}}


def json_key(gain):
    """JSON keeps string keys only: (board, channel) keys are written as "b,c" and restored by the test."""
    if not isinstance(gain, dict):
        return gain
    return {(f"{k[0]},{k[1]}" if isinstance(k, tuple) else k): json_key(v) for k, v in gain.items()}


# name -> (table, source, config, run_config, explicit keys)
def cases():
    base = {"df_events": {"time_window_ns": 100.0}}
    rec_cfg = {"df": {"wave_source": "records"}, "basic_features": {"wave_source": "records"}}
    return {
        "records_plain": ("rec", {**rec_cfg, **base}, None, ()),
        "st_plain": ("st", dict(base), None, ()),
        "records_gain_explicit": ("rec", {**rec_cfg, **base, "gain_adc_per_pe": GAIN_ALL}, None, (("df", "gain_adc_per_pe"),)),
        "st_gain_partial": ("st", {**base, "df": {"gain_adc_per_pe": GAIN_PARTIAL}}, None, ()),
        "st_gain_run": ("st", dict(base), GAIN_RUN, ()),
        "records_gain_run_top": ("rec", {**rec_cfg, **base}, GAIN_RUN_TOP, ()),
        "st_gain_explicit_over_run": ("st", {**base, "df": {"gain_adc_per_pe": GAIN_PARTIAL}}, GAIN_RUN, (("df", "gain_adc_per_pe"),)),
        "records_no_board": ("rec_no_board", {**rec_cfg, **base}, None, ()),
        "records_no_record_id": ("rec_no_rid", {**rec_cfg, **base}, None, ()),
        "st_no_board_no_rid": ("st_bare", dict(base), None, ()),
        "window_0": ("st", {"df_events": {"time_window_ns": 0.0}, "time_window_ns": 100.0}, None, ()),
        "window_5000": ("st", {"df_events": {"time_window_ns": 5000.0}, "time_window_ns": 5000.0, "n_channels": 3}, None, ()),
        "pair_drop_some": ("st", {"df_events": {"time_window_ns": 5000.0}, "time_window_ns": 60.0}, None, ()),
        "pair_drop_all": ("rec", {**rec_cfg, "df_events": {"time_window_ns": 200.0}, "time_window_ns": -1000.0}, None, ()),
        "n_channels_3": ("rec", {**rec_cfg, **base, "n_channels": 3, "start_channel_slice": 2}, None, ()),
    }


def put_frame(out: dict, prefix: str, frame) -> None:
    out[f"{prefix}/columns"] = np.array(list(frame.columns), dtype=str)
    out[f"{prefix}/dtypes"] = np.array([str(t) for t in frame.dtypes], dtype=str)
    out[f"{prefix}/index"] = frame.index.to_numpy().astype(np.int64)
    for k, col in enumerate(frame.columns):
        values = frame[col].to_numpy()
        if values.dtype == object:
            pieces = [np.asarray(v) for v in values]
            lens = np.array([len(p) for p in pieces], dtype=np.int64)
            out[f"{prefix}/c{k}/offsets"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            out[f"{prefix}/c{k}/flat"] = (np.concatenate(pieces) if len(pieces) and lens.sum() else np.zeros(0))
        else:
            out[f"{prefix}/c{k}"] = values


def main() -> None:
    rec, bf = make_tables(2026, 100)
    st = rec.copy()                        # dense branch: the same rows as a (sample-less) st_waveforms table
    tables = {"rec": rec, "st": st, "rec_no_board": drop_field(rec, "board"), "rec_no_rid": drop_field(rec, "record_id"),
              "st_bare": drop_field(drop_field(st, "board"), "record_id")}
    out: dict = {"bf": bf}
    for name, t in tables.items():
        out[f"table/{name}"] = t
    for name, (table, config, run_config, explicit) in cases().items():
        source = "records" if table.startswith("rec") else "st_waveforms"
        ctx = Ctx(config, {source: tables[table], "basic_features": bf}, run_config, explicit)
        df = ctx.get_data(RUN_ID, "df")
        ev = ctx.get_data(RUN_ID, "df_events")
        paired = ctx.get_data(RUN_ID, "df_paired")
        put_frame(out, f"{name}/df", df)
        put_frame(out, f"{name}/df_events", ev)
        put_frame(out, f"{name}/df_paired", paired)
        out[f"{name}/setup"] = np.array(json.dumps({"table": table, "source": source, "config": json_key(config),
                                                    "run_config": json_key(run_config),
                                                    "explicit": [list(e) for e in explicit]}))
    # error texts
    errors = {}
    rec_cfg = {"df": {"wave_source": "records"}, "basic_features": {"wave_source": "records"}}
    for ename, source, table, config, bf_in in (
        ("len_records", "records", rec[:-3], rec_cfg, bf),
        ("len_st", "st_waveforms", st[:-2], {}, bf),
        ("bf_not_records", "records", rec, {"df": {"wave_source": "records"}}, bf),
        ("bf_not_array", "st_waveforms", st, {}, [bf]),
    ):
        ctx = Ctx(config, {source: table, "basic_features": bf_in})
        try:
            ctx.get_data(RUN_ID, "df")
        except ValueError as exc:
            errors[ename] = str(exc)
        else:
            raise AssertionError(ename)
    for k, v in errors.items():
        out[f"err/{k}"] = np.array(v)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(cases())} cases")


if __name__ == "__main__":
    main()
