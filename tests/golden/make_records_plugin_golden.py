"""Generate tests/golden/vx2730csv_records_plugin.npz (both adapters; the vx2730csv_ prefix keeps it out of the
per-case parity suites) from the reference's RecordsPlugin / WavePoolPlugin
(waveform_analysis/core/plugins/builtin/cpu/records.py).  Run where the reference package is importable, as
make_golden.py is:

    python tests/golden/make_records_plugin_golden.py

Inputs are the files of the existing fixtures (vx2730csv_files.npz texts, v1725bin_files.npz blobs), written to a
temporary directory with a fixed modification time (the vx2730 adapter takes records.time's epoch from the first
file's stat).  channel_metadata is set in the context-config layer and in the run-config layer, so the records carry
the polarity of both layers.  Only arrays are stored.
"""

from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from waveform_analysis.core.plugins.builtin.cpu.records import RecordsPlugin, WavePoolPlugin  # noqa: E402

from tests import golden_util as G  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
FILE_MTIME = 1_700_000_123.5   # seconds; the epoch of records.time is this times 1e9

# context-config layer, then run-config layer (later wins per key)
METADATA_CONTEXT = {
    "defaults": {"polarity": "negative"},
    "groups": [{"name": "pos", "channels": ["0:3", [1, 7], "1:5"], "metadata": {"polarity": "positive"}}],
    "channels": {"0:1": {"polarity": "positive", "geometry": "top"}},
}
METADATA_RUN = {
    "channels": {"0:0": {"polarity": "bogus"}, "1:2": {"polarity": "positive"}, "0:4": {"geometry": "x"}},
}
RUN_ID = "run_0"


class Ctx:
    """The slice of Context that RecordsPlugin / WavePoolPlugin read."""

    def __init__(self, config, raw_files, plugins, run_config):
        self.config = dict(config)
        self._data = {"raw_files": raw_files}
        self._results = {}
        self._plugins = {p.provides: p for p in plugins}
        self._run_config = run_config

    def get_plugin(self, name):
        return self._plugins[name]

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

    def get_run_config(self, run_id):
        return self._run_config

    def get_data(self, run_id, name):
        if (run_id, name) in self._results:
            return self._results[(run_id, name)]
        if name in self._data:
            return self._data[name]
        plugin = self._plugins[name]
        value = plugin.compute(self, run_id)
        self._results[(run_id, name)] = value
        return value

    def _set_data(self, run_id, name, value):
        self._results[(run_id, name)] = value

    def key_for(self, run_id, data_name):
        return f"{run_id}-{data_name}-key"


def write(tmp, name, data):
    path = os.path.join(tmp, name)
    with open(path, "wb") as fh:
        fh.write(data)
    os.utime(path, (FILE_MTIME, FILE_MTIME))
    return path


def build(config, raw_files):
    ctx = Ctx(config, raw_files, [RecordsPlugin(), WavePoolPlugin()], {"channel_metadata": METADATA_RUN})
    records = ctx.get_data(RUN_ID, "records")
    pool = ctx.get_data(RUN_ID, "wave_pool")
    return records, pool


def main():
    out = {}
    tmp = tempfile.mkdtemp(prefix="wfa_records_plugin_")
    groups, _variants, _fx = G.load_vx2730csv()
    paths = [[write(tmp, fname, text) for fname, text in group] for group in groups]
    base = {"channel_metadata": METADATA_CONTEXT, "show_progress": False}
    out["vx2730_records"], out["vx2730_wave_pool"] = build(base | {"daq_adapter": "vx2730"}, paths)

    z = np.load(os.path.join(OUT, "v1725bin_files.npz"), allow_pickle=False)
    names = bytes(z["names"]).decode().split("\n")
    vpaths = [write(tmp, name, bytes(z[f"blob{k}"])) for k, name in enumerate(names)]
    raw = [[vpaths[0], vpaths[1]], [vpaths[2], vpaths[0]]]          # a duplicated path: kept once
    out["v1725_records"], out["v1725_wave_pool"] = build(base | {"daq_adapter": "v1725"}, raw)

    out["options_json"] = np.frombuffer(json.dumps({
        "file_mtime": FILE_MTIME, "run_id": RUN_ID, "metadata_context": METADATA_CONTEXT,
        "metadata_run": METADATA_RUN, "v1725_groups": [[0, 1], [2, 0]]}).encode(), dtype=np.uint8)
    path = os.path.join(OUT, "vx2730csv_records_plugin.npz")
    np.savez_compressed(path, **out)
    print(f"vx2730csv_records_plugin: vx2730 {len(out['vx2730_records'])} records, "
          f"v1725 {len(out['v1725_records'])} records, "
          f"polarities {sorted(set(out['vx2730_records']['polarity']) | set(out['v1725_records']['polarity']))} "
          f"-> {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
