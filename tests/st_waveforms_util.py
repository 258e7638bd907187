"""Cases of tests/golden/vx2730csv_st_waveforms.npz (made by make_st_waveforms_golden.py from the reference's
WaveformsPlugin): the file texts, the channel lists and options of every case, and a Context to run one."""

from __future__ import annotations

import json
import os

import numpy as np

from tests import golden_util as G
from waveformanalysis_amd.plugin_api import SimpleContext

FIXTURE = os.path.join(G.GOLDEN, "vx2730csv_st_waveforms.npz")


def load():
    """-> (meta dict with "cases", files {name: bytes}, arrays {key: array}, layout {file: (delimiter, skiprows)})."""
    z = np.load(FIXTURE, allow_pickle=False)
    d = {k: z[k] for k in z.files}
    meta = json.loads(bytes(d.pop("cases_json")).decode())
    layout = {k: tuple(v) for k, v in json.loads(bytes(d.pop("layout_json")).decode()).items()}
    files = {k[len("file_"):]: bytes(v) for k, v in d.items() if k.startswith("file_")}
    return meta, files, d, layout


def case_config(case) -> dict:
    config = dict(case["config"])
    if case["baseline_tuple"]:
        config["baseline_samples"] = tuple(config["baseline_samples"])
    config["daq_adapter"] = case["adapter"]
    return config


class RunCtx(SimpleContext):
    def __init__(self, *a, run_config=None, **kw):
        super().__init__(*a, **kw)
        self.run_config = run_config or {}

    def get_run_config(self, run_id):
        return self.run_config


def write_files(tmp_path, meta, files) -> dict:
    """Every fixture file under tmp_path with the fixture's mtime -> {name: path}."""
    paths = {}
    for name, text in files.items():
        p = os.path.join(str(tmp_path), name)
        with open(p, "wb") as fh:
            fh.write(text)
        os.utime(p, (meta["file_mtime"], meta["file_mtime"]))
        paths[name] = p
    paths[meta["missing"]] = os.path.join(str(tmp_path), "does_not_exist.CSV")
    return paths


def context(case, meta, arrays, paths, plugin, extra_config=None) -> tuple[RunCtx, list]:
    raw = [[paths[f] for f in group] for group in case["lists"]]
    data = {"raw_files": raw}
    if case["upstream"] is not None:
        data["baseline"] = [arrays[f"upstream_{case['name']}_{k}"] if present else None
                            for k, present in enumerate(case["upstream"])]
    elif case["config"].get("use_upstream_baseline"):
        data["baseline"] = [np.zeros(1000)] * len(raw)
    ctx = RunCtx(case_config(case) | (extra_config or {}), data, [plugin],
                 run_config={"channel_metadata": meta["metadata_run"]})
    return ctx, raw
