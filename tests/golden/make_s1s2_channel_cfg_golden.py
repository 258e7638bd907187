"""Generate tests/golden/s1s2_channel_cfg.npz: the reference's S1/S2 chain on the ragged records run of
tests/golden/c5_width_records.npz under per-channel filter settings and fixed baselines.  Run where the reference package
is importable, as make_golden.py is:

    python tests/golden/make_s1s2_channel_cfg_golden.py

Chain: WavePoolFilteredPlugin (channel_config: 0:1 and 0:5 SG(7, 3), 0:2 SG(21, 4), 0:6 a Butterworth band pass, the
other channels the run-wide SG(11, 2)), HitFinderPlugin on the records route (use_filtered, the ragged run's hit options),
WaveformWidthPlugin._calculate_width_from_peak on the record slices of wave_pool as in make_width_records_golden.py (the
reference has no records route for waveform_width), BasicFeaturesPlugin on the records route (channel_config: fixed
baseline 8000.0 on 0:1, 0.0 on 0:4) and S1S2ClassifierPlugin under two range sets: the C5 ranges, and the C5 ranges with an
S1 area range that the fixed baselines move rows out of.

Asserted here: every filter group has a hit, labels 1 and 2 both occur, the chain without the settings gives another
table, and under the second range set the fixed baselines change a label.
Stored: arrays only -- the table of every stage, the labels without the fixed baselines under the second set, and the
configuration as JSON bytes.
"""

from __future__ import annotations

import io
import json
import os
import sys
import warnings
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from waveform_analysis.core.plugins.builtin.cpu.basic_features import BasicFeaturesPlugin  # noqa: E402
from waveform_analysis.core.plugins.builtin.cpu.peak_finding import HitFinderPlugin  # noqa: E402
from waveform_analysis.core.plugins.builtin.cpu.records import WavePoolFilteredPlugin  # noqa: E402
from waveform_analysis.core.plugins.builtin.cpu.s1_s2_classifier import S1S2ClassifierPlugin  # noqa: E402
from waveform_analysis.core.plugins.builtin.cpu.waveform_width import (  # noqa: E402
    WAVEFORM_WIDTH_DTYPE,
    WaveformWidthPlugin,
)

from tests import s1s2_chain_util as U  # noqa: E402
from tests import s1s2_settings_util as T  # noqa: E402

OUT = T.FIXTURE


class Ctx:
    """Minimal context (as in make_golden.py): config lookup order plugin-nested > namespaced > global > default."""

    def __init__(self, config, data):
        self.config = dict(config)
        self._data = dict(data)
        self._plugins = {}

    def get_config(self, plugin, name):
        prov = plugin.provides
        if isinstance(self.config.get(prov), dict) and name in self.config[prov]:
            return self.config[prov][name]
        if f"{prov}.{name}" in self.config:
            return self.config[f"{prov}.{name}"]
        if name in self.config:
            return self.config[name]
        if name in plugin.options:
            return plugin.options[name].default
        return None

    def get_data(self, run_id, name):
        return self._data.get(name)


def write_npz(path, arrays):
    """np.savez_compressed with a fixed entry date, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def widths(hits, rec, pool):
    """waveform_width.py:153-190 with the record's slice for the dense row, default options, sampling rate 0.5."""
    plugin = WaveformWidthPlugin()
    kw = {name: plugin.options[name].default for name in ("rise_low", "rise_high", "fall_high", "fall_low", "interpolation")}
    rows = []
    for peak in hits:
        r = int(peak["record_id"])
        off, L = int(rec["wave_offset"][r]), int(rec["event_length"][r])
        with np.errstate(all="ignore"):
            row = plugin._calculate_width_from_peak(pool[off : off + L], peak["position"], peak["timestamp"], peak["board"],
                                                    peak["channel"], r, kw["rise_low"], kw["rise_high"], kw["fall_high"],
                                                    kw["fall_low"], 0.5, kw["interpolation"])
        if row is not None:
            rows.append(row)
    return np.array(rows, dtype=WAVEFORM_WIDTH_DTYPE)


def chain(rec, pool, hit_kw, filter_cc, baseline_cc):
    """The tables of the stages in front of the classifier."""
    data = {"records": rec, "wave_pool": pool}
    data["wave_pool_filtered"] = WavePoolFilteredPlugin().compute(
        Ctx({"max_workers": 1, "wave_pool_filtered": {"channel_config": filter_cc}}, data), "run")
    data["hit"] = HitFinderPlugin().compute(Ctx({"wave_source": "records", "use_filtered": True, **hit_kw}, data), "run")
    data["waveform_width"] = widths(data["hit"], rec, pool)
    data["basic_features"] = BasicFeaturesPlugin().compute(
        Ctx({"wave_source": "records", "basic_features": {"channel_config": baseline_cc}}, data), "run")
    return data


def classify(data, ranges):
    return S1S2ClassifierPlugin().compute(Ctx(ranges, data), "run")


def main():
    warnings.simplefilter("ignore", RuntimeWarning)  # np.mean of an empty record
    rec, pool, hit_kw = U.run("ragged")
    data = chain(rec, pool, hit_kw, T.FILTER_CC, T.BASELINE_CC)
    plain = chain(rec, pool, hit_kw, None, None)
    no_fixed = chain(rec, pool, hit_kw, T.FILTER_CC, None)
    out = {name: data[name] for name in ("wave_pool_filtered", "hit", "waveform_width", "basic_features")}
    for name, ranges in T.RANGE_SETS.items():
        out[f"s1_s2_{name}"] = classify(data, ranges)
    out["labels_area_no_fixed"] = classify(no_fixed, T.AREA_RANGES)["label"]
    out["config_json"] = np.frombuffer(json.dumps(
        {"wave_pool_filtered": {"channel_config": T.FILTER_CC}, "basic_features": {"channel_config": T.BASELINE_CC},
         "hit": hit_kw, "ranges": {k: {n: (list(v) if v is not None else None) for n, v in r.items()}
                                   for k, r in T.RANGE_SETS.items()}}, sort_keys=True).encode(), dtype=np.uint8)

    hits, rows = out["hit"], out["s1_s2_c5"]
    for g in range(len(T.KEYS)):
        chans = [c for c in range(14) if T.GROUP_OF_CHANNEL.get(c, 0) == g]
        assert np.isin(hits["channel"], chans).any(), f"filter group {g} has no hit"
    assert {1, 2} <= set(rows["label"].tolist())
    without = classify(plain, U.C5_RANGES)
    assert len(without) != len(rows) or without.tobytes() != rows.tobytes()
    changed = int(np.count_nonzero(out["s1_s2_area"]["label"] != out["labels_area_no_fixed"]))
    assert changed >= 1, "the second range set does not see the fixed baselines"
    write_npz(OUT, out)
    print(f"{len(rows)} rows {U.counts(rows)} against {len(without)} {U.counts(without)} without the settings; "
          f"{int(np.count_nonzero(data['wave_pool_filtered'] != plain['wave_pool_filtered']))} filtered samples and "
          f"{sum(a.tobytes() != b.tobytes() for a, b in zip(data['basic_features'], plain['basic_features']))} feature "
          f"rows differ; area set: {U.counts(out['s1_s2_area'])}, {changed} labels changed by the fixed baselines")
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
