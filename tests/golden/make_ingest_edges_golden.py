"""Generate tests/golden/ingest_edges.npz from the reference's own readers and builders, on the edge files of
tests/ingest_edges_util.py.  Run by hand where the reference package is importable (WFA_REFERENCE may name its tree),
from any scratch directory, as make_records_plugin_golden.py is:

    python tests/golden/make_ingest_edges_golden.py

CSV: the VX2730-layout rows of csv_phases / csv_tile_seams, one file per row width (vx_files), limited to CSV_MAX_BYTES
of text to keep the fixture small.  Every file is read with the reference's VX2730Reader.read_file (its pyarrow or
pandas backend: polars is not installed here) and the bundle is built with build_records_from_raw_files.  The reference
stores samples as int16, so only rows whose samples are <= 32767 are used (vx_files(max_sample=32767)): the '+65535'
rows of the seam table are checked against the oracle alone.
V1725: the crafted streams of v1725_file_groups, read with V1725Reader.iter_waves and built with
build_records_from_v1725_files (dt_ns = 4).

Where the reference raises, the case name goes to `reference_raises` instead of a table; the tests then use the oracle
for that case alone.  Only arrays are stored: input bytes, the reference's tables, lists of names.  The archive is
written with fixed zip timestamps, so a second run gives the same bytes.
"""

from __future__ import annotations

import io
import os
import sys
import tempfile
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("WFA_REFERENCE"):
    sys.path.insert(0, os.environ["WFA_REFERENCE"])
sys.path.insert(0, REPO)

from waveform_analysis.core.processing.records_builder import (  # noqa: E402
    build_records_from_raw_files,
    build_records_from_v1725_files,
)
from waveform_analysis.utils.formats.v1725 import V1725Reader  # noqa: E402
from waveform_analysis.utils.formats.vx2730 import VX2730Reader  # noqa: E402

from tests import ingest_edges_util as U  # noqa: E402

CSV_MAX_BYTES = 150_000
V1725_DT_NS = 4


def save_npz(path, arrays):
    """np.savez_compressed with a fixed timestamp on every member (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def names_array(names):
    return np.frombuffer("\n".join(names).encode(), dtype=np.uint8)


def main():
    out, raises = {}, []
    tmp = tempfile.mkdtemp(prefix="wfa_ingest_edges_")

    lists = U.vx_files(max_sample=U.FIXTURE_MAX_SAMPLE, max_bytes=CSV_MAX_BYTES)
    paths = []
    for g in lists:
        paths.append([])
        for k, (name, text) in enumerate(g):
            p = os.path.join(tmp, name)
            with open(p, "wb") as fh:
                fh.write(text)
            paths[-1].append(p)
            key = "csv_" + name.replace("@", "_at_").replace(".", "_dot_")
            out[key + "_text"] = np.frombuffer(text, dtype=np.uint8)
            try:
                rows = np.asarray(VX2730Reader().read_file(p, is_first_file=(k == 0)))
                if rows.ndim != 2 or rows.size == 0:
                    raise ValueError(f"read_file gave shape {rows.shape}")
                table = np.zeros(rows.shape, dtype=np.int64)
                for c in range(rows.shape[1]):
                    if c == 5 and rows.dtype == object and any(isinstance(v, str) for v in rows[:, c]):
                        continue   # FLAGS as hex text: the reader hands the strings through, the fixture stores 0
                    col = rows[:, c].astype(np.float64)
                    if not np.all(np.isfinite(col)):
                        raise ValueError(f"column {c} holds a non-finite value")
                    table[:, c] = [int(v) for v in rows[:, c]]
                out[key + "_rows"] = table
            except Exception as exc:   # noqa: BLE001 -- the fixture records what the reference raises
                print(f"reference raises on {name}: {type(exc).__name__}: {exc}")
                raises.append(name)
    out["csv_names"] = names_array([n for g in lists for n, _t in g])
    out["csv_max_bytes"] = np.int64(CSV_MAX_BYTES)
    try:
        b = build_records_from_raw_files(paths, adapter_name="vx2730", show_progress=False, part_size=None, default_dt_ns=2)
        out["csv_records"], out["csv_wave_pool"] = b.records, b.wave_pool
    except Exception as exc:   # noqa: BLE001
        print(f"reference raises on the csv bundle: {type(exc).__name__}: {exc}")
        raises.append("csv_bundle")

    files = U.v1725_file_groups()
    vpaths = []
    for k, (name, blob) in enumerate(files):
        p = os.path.join(tmp, name)
        with open(p, "wb") as fh:
            fh.write(blob)
        vpaths.append(p)
        out[f"v1725_blob{k}"] = np.frombuffer(blob, dtype=np.uint8)
        try:
            waves = list(V1725Reader().iter_waves([p]))
            out[f"v1725_index{k}"] = np.array([(w.channel, w.timestamp, int(w.trunc), w.baseline, len(w.waveform)) for w in waves],
                                             dtype=np.int64).reshape(-1, 5)
        except Exception as exc:   # noqa: BLE001
            print(f"reference raises on {name}: {type(exc).__name__}: {exc}")
            raises.append(name)
    out["v1725_names"] = names_array([n for n, _b in files])
    try:
        b = build_records_from_v1725_files(vpaths, dt_ns=V1725_DT_NS)
        out["v1725_records"], out["v1725_wave_pool"] = b.records, b.wave_pool
    except Exception as exc:   # noqa: BLE001
        print(f"reference raises on the v1725 bundle: {type(exc).__name__}: {exc}")
        raises.append("v1725_bundle")

    out["reference_raises"] = names_array(raises)
    path = os.path.join(REPO, "tests", "golden", "ingest_edges.npz")
    save_npz(path, out)
    print(f"ingest_edges: {len(out['csv_names'].tobytes().split())} csv files, {len(files)} v1725 files, "
          f"reference_raises {raises} -> {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
