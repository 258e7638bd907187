"""Generate tests/golden/vx2730csv_st_waveforms.npz (both adapters; the vx2730csv_ prefix keeps it out of the per-case
parity suites) from the reference's WaveformsPlugin (waveform_analysis/core/plugins/builtin/cpu/waveforms.py).  Run
where the reference package is importable, as make_records_plugin_golden.py is:

    python tests/golden/make_st_waveforms_golden.py

Inputs are the files of the existing fixtures (vx2730csv_files.npz texts, v1725bin_files.npz blobs) plus a few
variants of them (a comma-delimited file, header rows in a non-first file, blank lines, an empty file, ragged rows),
written to a temporary directory with a fixed modification time.  Every file text is stored once (`file_<name>`);
`cases_json` lists per case the options, the channel lists (file names, "<missing>" for a path that does not exist)
and the upstream baselines.  The reference's own sniffing and wave-length detection results are stored too
(`layout_json`).  Only arrays are stored.
"""

from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from waveform_analysis.core.plugins.builtin.cpu import waveforms as W  # noqa: E402
from waveform_analysis.utils.formats import VX2730_SPEC  # noqa: E402

from tests import golden_util as G  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
FILE_MTIME = 1_700_000_123.5
MISSING = "<missing>"

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
    """The slice of Context that WaveformsPlugin reads."""

    def __init__(self, config, data, run_config):
        self.config = dict(config)
        self._data = dict(data)
        self._run_config = run_config
        self.profiler = None

        class _Log:
            def info(self, *a, **k):
                pass

            warning = debug = error = info

        self.logger = _Log()

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
        return self._data[name]


def _variants(groups):
    """Extra file texts derived from the fixture files."""
    texts = {name: text for group in groups for name, text in group}
    ch0 = texts["DataR_CH0@VX2730_run_1.CSV"]
    header = texts["DataR_CH0@VX2730_run.CSV"].split(b"\n", 1)[0] + b"\n"
    lines = ch0.split(b"\n")
    extra = {
        "comma_CH1_run_1.CSV": texts["DataR_CH1@VX2730_run_1.CSV"].replace(b";", b","),
        "header_CH0_run_1.CSV": header + ch0,
        "blank_CH0_run_1.CSV": b"\n\n" + b"\n".join(lines[:3]) + b"\n\n\n" + b"\n".join(lines[3:]) + b"\n\n",
        "empty.CSV": b"",
    }
    cut = lines[2].rsplit(b";", 10)[0]           # row 2 with 10 samples fewer
    extra["ragged_in_file.CSV"] = b"\n".join(lines[:2] + [cut] + lines[3:])
    wide = [ln + b";8000;8001;8002;8003" if ln.strip() else ln for ln in lines]   # every row 4 samples wider
    extra["wider_CH0.CSV"] = b"\n".join(wide)
    return extra


def _cases():
    base = [["DataR_CH0@VX2730_run.CSV", "DataR_CH0@VX2730_run_1.CSV", "DataR_CH0@VX2730_run_2.CSV"], [],
            ["DataR_CH1@VX2730_run.CSV", "DataR_CH1@VX2730_run_1.CSV"], ["DataR_CH5@VX2730_run.CSV"]]
    meta = {"channel_metadata": METADATA_CONTEXT}
    c = [
        ("default", base, meta, None),
        ("nometa", base, {}, None),
        ("wl_short", base, meta | {"wave_length": 50}, None),
        ("wl_short_odd", base, meta | {"wave_length": 61}, None),
        ("wl_long_odd", base, meta | {"wave_length": 141}, None),
        ("bs_int", base, meta | {"baseline_samples": 25}, None),
        ("bs_tuple", base, meta | {"baseline_samples": (10, 60)}, None),
        ("bs_list", base, meta | {"baseline_samples": [5, 30]}, None),
        ("bs_past_end", base, meta | {"baseline_samples": (100, 200)}, None),
        ("dt", base, meta | {"dt": 3}, None),
        ("dt_deprecated", base, meta | {"sampling_interval_ns": 7}, None),
        ("streaming", base, meta | {"streaming_mode": True}, None),
        ("streaming_wl_odd", base, meta | {"streaming_mode": True, "wave_length": 99}, None),
        ("upstream", base, meta | {"use_upstream_baseline": True}, "upstream"),
        ("comma", [base[0], ["DataR_CH1@VX2730_run.CSV", "comma_CH1_run_1.CSV"], base[3]], meta, None),
        ("header_not_first", [["DataR_CH0@VX2730_run.CSV", "header_CH0_run_1.CSV"], base[3]], meta, None),
        ("blank_lines", [["DataR_CH0@VX2730_run.CSV", "blank_CH0_run_1.CSV"], base[2]], meta, None),
        ("empty_list_file", [[], ["empty.CSV", "DataR_CH0@VX2730_run_2.CSV", MISSING], [],
                             ["DataR_CH5@VX2730_run.CSV", "empty.CSV"]], meta, None),
        ("detect_skips_empty", [["empty.CSV"], ["DataR_CH5@VX2730_run.CSV"], base[0]], meta, None),
        ("ragged_in_file", [["ragged_in_file.CSV"], base[3]], meta, None),
        ("ragged_across_files", [["DataR_CH0@VX2730_run.CSV", "wider_CH0.CSV"], base[3]], meta, None),
        ("empty_raw_files", [], meta, None),
        ("empty_raw_files_wl", [], meta | {"wave_length": 77}, None),
    ]
    return c


def _upstream(n_rows_per_list):
    """One array of matching length for list 0, a mismatching one for list 2, nothing for the rest."""
    rng = np.random.default_rng(5)
    out = [rng.normal(8000, 3, n_rows_per_list[0]), None, rng.normal(8000, 3, n_rows_per_list[2] + 1)]
    return out


def write(tmp, name, data):
    path = os.path.join(tmp, name)
    with open(path, "wb") as fh:
        fh.write(data)
    os.utime(path, (FILE_MTIME, FILE_MTIME))
    return path


def run(config, raw_files, baseline=None):
    data = {"raw_files": raw_files}
    if baseline is not None:
        data["baseline"] = baseline
    ctx = Ctx(config | {"show_progress": False}, data, {"channel_metadata": METADATA_RUN})
    plugin = W.WaveformsPlugin()
    try:
        return plugin.compute(ctx, RUN_ID), None
    except Exception as exc:   # noqa: BLE001 -- the fixture records what the reference raises
        return None, f"{type(exc).__name__}: {exc}"


def main():
    out = {}
    tmp = tempfile.mkdtemp(prefix="wfa_st_waveforms_")
    groups, _variants_unused, _fx = G.load_vx2730csv()
    texts = {name: text for group in groups for name, text in group}
    texts.update(_variants(groups))
    paths = {name: write(tmp, name, text) for name, text in texts.items()}
    paths[MISSING] = os.path.join(tmp, "does_not_exist.CSV")
    for name, text in texts.items():
        out["file_" + name] = np.frombuffer(text, dtype=np.uint8)

    layout = {name: list(W._sniff_csv_layout(p)) for name, p in paths.items()}
    cases = []
    for name, lists, config, upstream in _cases():
        raw = [[paths[f] for f in group] for group in lists]
        baseline = None
        if upstream:
            counts = [len(run(config | {"use_upstream_baseline": False}, [g])[0]) for g in raw]
            baseline = _upstream(counts)
            for k, b in enumerate(baseline):
                if b is not None:
                    out[f"upstream_{name}_{k}"] = b
        arr, err = run(config | {"daq_adapter": "vx2730"}, raw, baseline)
        detected = W._detect_wave_length_from_files(raw, VX2730_SPEC.columns) if raw else None
        cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in config.items()}
        cases.append({"name": name, "adapter": "vx2730", "lists": lists, "config": cfg, "error": err,
                      "upstream": [b is not None for b in baseline] if baseline else None,
                      "baseline_tuple": isinstance(config.get("baseline_samples"), tuple),
                      "detected_wave_length": detected})
        if arr is not None:
            out[f"st_{name}"] = arr
        print(name, err or (len(arr), arr.dtype["wave"].shape))

    z = np.load(os.path.join(OUT, "v1725bin_files.npz"), allow_pickle=False)
    vnames = bytes(z["names"]).decode().split("\n")
    for k, name in enumerate(vnames):
        blob = bytes(z[f"blob{k}"])
        paths[name] = write(tmp, name, blob)
        out["file_" + name] = np.frombuffer(blob, dtype=np.uint8)
    v_lists = [[vnames[0], vnames[1]], [vnames[2], vnames[0]]]   # a duplicated path: kept once
    meta = {"channel_metadata": METADATA_CONTEXT}
    for name, lists, config in [("v1725_default", v_lists, meta),
                                ("v1725_wl", v_lists, meta | {"wave_length": 301}),
                                ("v1725_dt", [[vnames[2]], [vnames[1]]], meta | {"dt": 2, "use_upstream_baseline": True}),
                                ("v1725_empty", [], meta)]:
        raw = [[paths[f] for f in group] for group in lists]
        baseline = [np.zeros(1000)] * len(raw) if config.get("use_upstream_baseline") else None
        arr, err = run(config | {"daq_adapter": "v1725"}, raw, baseline)
        cases.append({"name": name, "adapter": "v1725", "lists": lists, "config": config, "error": err,
                      "upstream": None, "baseline_tuple": False, "detected_wave_length": None})
        if arr is not None:
            out[f"st_{name}"] = arr
        print(name, err or (len(arr), arr.dtype["wave"].shape))

    out["cases_json"] = np.frombuffer(json.dumps({
        "file_mtime": FILE_MTIME, "run_id": RUN_ID, "metadata_context": METADATA_CONTEXT,
        "metadata_run": METADATA_RUN, "missing": MISSING, "cases": cases}).encode(), dtype=np.uint8)
    out["layout_json"] = np.frombuffer(json.dumps({n: v for n, v in layout.items() if n != MISSING}).encode(),
                                       dtype=np.uint8)
    path = os.path.join(OUT, "vx2730csv_st_waveforms.npz")
    np.savez_compressed(path, **out)
    print(f"vx2730csv_st_waveforms: {len(cases)} cases -> {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
