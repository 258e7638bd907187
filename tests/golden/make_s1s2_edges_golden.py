"""Generate tests/golden/s1s2_edges.npz: the labels the reference's S1S2ClassifierPlugin
(waveform_analysis/core/plugins/builtin/cpu/s1_s2_classifier.py:133-228) gives on the ragged edge run of
tests/s1s2_edges_util.py under every range set of `bound_sets`.  Run where the reference package is importable, as
make_golden.py is:

    python tests/golden/make_s1s2_edges_golden.py

Inputs: the oracle's waveform_width rows (records route, widths on wave_pool) and basic_features rows of the run, once
with and once without interpolation; the sets are built on each table's own kept rows, so every bound sits on a value
that table holds.  NaN and infinite bounds and a conflict_policy outside the reference's three go to the plugin as they
are; `strict` with no range configured gives its error text.

Stored: arrays only -- the two width tables and the feature table (width_ns / area live there, once), the sets as JSON
bytes in sorted-name order, and one int8 label row per set in that order.
"""

from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from waveform_analysis.core.plugins.builtin.cpu.s1_s2_classifier import S1S2ClassifierPlugin  # noqa: E402

from tests import s1s2_edges_util as E  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "s1s2_edges.npz")


class Ctx:
    """Minimal context (as in make_golden.py): config lookup order plugin-nested > namespaced > global > default."""

    def __init__(self, config, data):
        self.config = dict(config)
        self._data = dict(data)

    def get_config(self, plugin, name):
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


def main():
    out = {}
    plugin = S1S2ClassifierPlugin()
    for i, interpolation in enumerate((False, True)):
        _hits, widths, feats = E.oracle_tables("ragged", interpolation=interpolation)
        data = {"waveform_width": widths, "basic_features": feats}
        sets = E.bound_sets(E.oracle_rows("ragged", {}, interpolation=interpolation))
        labels = np.zeros((len(sets), len(widths)), dtype=np.int8)
        for k, name in enumerate(sorted(sets)):
            rows = plugin.compute(Ctx(sets[name], data), "run")
            assert len(rows) == len(widths)
            labels[k] = rows["label"]
        out[f"widths_{i}"] = widths
        out[f"sets_{i}"] = np.frombuffer(E.to_json(sets), dtype=np.uint8)
        out[f"labels_{i}"] = labels
        out["features"] = feats
        print(f"interpolation={interpolation}: {len(widths)} rows, {len(sets)} sets, "
              f"label counts {np.bincount(labels.reshape(-1), minlength=3).tolist()}")
    try:
        plugin.compute(Ctx({"strict": True}, data), "run")
        raise SystemExit("strict with no range configured did not raise")
    except ValueError as err:
        out["strict_text"] = np.frombuffer(str(err).encode(), dtype=np.uint8)
    write_npz(OUT, out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
