"""HipWaveformsPlugin on the GPU: every case of tests/golden/vx2730csv_st_waveforms.npz (made by the reference's
WaveformsPlugin) through a Context, byte for byte; many small pack batches and many small decode parts against the
one-shot build; a synthetic ~10^7-sample CSV run against a numpy construction; every sample source of wfa_st_pack."""

import os

import numpy as np
import pytest

from tests import st_waveforms_util as U
from waveformanalysis_amd import st_builder as SB
from waveformanalysis_amd.device import DeviceSession
from waveformanalysis_amd.dtypes import create_record_dtype
from waveformanalysis_amd.plugins import HipWaveformsPlugin

pytestmark = pytest.mark.gpu


def _build(case, meta, arrays, paths, **plugin_kw):
    ctx, _raw = U.context(case, meta, arrays, paths, HipWaveformsPlugin(**plugin_kw))
    return ctx.get_data("r0", "st_waveforms")


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    meta, files, arrays, _layout = U.load()
    paths = U.write_files(tmp_path_factory.mktemp("st"), meta, files)
    return meta, arrays, paths


def test_every_case_byte_identical(fixture):
    meta, arrays, paths = fixture
    for case in meta["cases"]:
        want = arrays.get("st_" + case["name"])
        if want is None:   # the reference raises (ragged rows inside one file)
            with pytest.raises(RuntimeError, match="rows with 93 and 103 fields"):
                _build(case, meta, arrays, paths)
            continue
        got = _build(case, meta, arrays, paths)
        assert got.dtype == want.dtype, case["name"]
        assert got.tobytes() == want.tobytes(), case["name"]


@pytest.mark.parametrize("name", ["default", "wl_short_odd", "wl_long_odd", "comma", "blank_lines", "v1725_default",
                                  "v1725_wl"])
def test_small_batches_and_parts_equal_one_shot(fixture, name):
    meta, arrays, paths = fixture
    case = next(c for c in meta["cases"] if c["name"] == name)
    one = _build(case, meta, arrays, paths)
    stride = one.dtype.itemsize
    for kw in ({"pack_batch_bytes": 1}, {"pack_batch_bytes": 3 * stride + 5}, {"pack_batch_bytes": 7 * stride},
               {"part_bytes": 97}, {"part_bytes": 1000, "pack_batch_bytes": 2 * stride - 1}):
        got = _build(case, meta, arrays, paths, **kw)
        assert got.tobytes() == one.tobytes(), (name, kw)
    assert one.tobytes() == arrays["st_" + name].tobytes()


def _synthetic_run(tmp_path, rng, widths, rows_per_file, files_per_list):
    """CSV files of several channel lists (one sample count per list) and the numpy table they must give."""
    raw, lists = [], []
    for k, w in enumerate(widths):
        group, parts = [], []
        for f in range(files_per_list):
            n = rows_per_file
            wave = rng.integers(0, 65536, (n, w), dtype=np.int64)
            ts = rng.integers(0, 2**40, n, dtype=np.int64)
            head = np.stack([np.full(n, k % 3), np.full(n, k), ts, np.zeros(n, np.int64), np.ones(n, np.int64),
                             np.zeros(n, np.int64), np.ones(n, np.int64)], axis=1)
            table = np.concatenate([head, wave], axis=1)
            lines = "\n".join(";".join(map(str, row)) for row in table.tolist())
            hdr = "BOARD;CHANNEL;TIMETAG;ENERGY;ENERGYSHORT;FLAGS;PROBE_CODE;SAMPLES\n" if f == 0 else ""
            p = os.path.join(str(tmp_path), f"syn_{k}_{f}.CSV")
            with open(p, "w") as fh:
                fh.write(hdr + lines + "\n")
            group.append(p)
            parts.append((head, wave))
        raw.append(group)
        lists.append(parts)
    return raw, lists


def _numpy_table(lists, widths, L, dt):
    rows = []
    for w, parts in zip(widths, lists):
        for head, wave in parts:
            n = len(head)
            t = np.zeros(n, dtype=create_record_dtype(L))
            t["baseline"] = wave[:, 0:min(40, w)].mean(axis=1)
            t["baseline_upstream"] = np.nan
            t["polarity"] = "unknown"
            t["timestamp"] = head[:, 2]
            t["dt"] = dt
            t["event_length"] = min(w, L)
            t["board"] = head[:, 0]
            t["channel"] = head[:, 1]
            m = min(w, L)
            t["wave"][:, :m] = wave[:, :m].astype(np.uint16).view(np.int16)
            rows.append(t)
    out = np.concatenate(rows)
    out["record_id"] = np.arange(len(out))
    return out


@pytest.mark.parametrize("L", [1499, 800])
def test_synthetic_run_against_numpy(tmp_path, L):
    rng = np.random.default_rng(L)
    widths = [1500, 777, 1203]
    raw, lists = _synthetic_run(tmp_path, rng, widths, rows_per_file=1100, files_per_list=2)
    want = _numpy_table(lists, widths, L, 2)
    assert sum(len(h) * w for w, p in zip(widths, lists) for h, _w in p) > 7_000_000
    p = HipWaveformsPlugin(part_bytes=3 << 20, pack_batch_bytes=(5 << 20) + 3)
    ctx = U.RunCtx({"wave_length": L}, {"raw_files": raw}, [p])
    got = ctx.get_data("r0", "st_waveforms")
    assert got.dtype == want.dtype
    for name in want.dtype.names:
        a, b = got[name], want[name]
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), name
    assert got.tobytes() == want.tobytes()


def test_pack_sources_agree():
    """host pool, resident CSV samples, CSV arena and resident wave_pool give the same rows."""
    rng = np.random.default_rng(3)
    n = 333
    lens = rng.integers(0, 90, n).astype(np.int32)
    rows = ["1;2;%d;0;0;0;1;%s" % (i, ";".join(map(str, rng.integers(0, 65536, k)))) if k else "1;2;%d;0;0;0;1" % i
            for i, k in enumerate(lens)]
    text = ("\n".join(rows) + "\n").encode()
    cols = {"baseline": rng.normal(size=n), "baseline_upstream": np.nan, "timestamp": np.arange(n) * 7,
            "record_id": np.arange(n), "dt": 3, "event_length": np.minimum(lens, 61), "board": rng.integers(-5, 5, n),
            "channel": rng.integers(0, 64, n)}
    codes = rng.integers(0, 3, n)
    table = ["negative", "positive", ""]
    with DeviceSession(0) as sess:
        dec = sess.csv_decode(text, download_samples=True)
        so = dec["sample_offset"]
        ln = np.maximum(dec["n_fields"] - 7, 0)
        np.testing.assert_array_equal(ln, lens)
        want = np.zeros(n, dtype=create_record_dtype(61))
        for k, v in cols.items():
            want[k] = v
        want["polarity"] = np.asarray(table)[codes]
        for r in range(n):
            m = min(int(lens[r]), 61)
            want["wave"][r, :m] = dec["samples"][so[r]:so[r] + m].view(np.int16)
        got_csv = sess.st_pack(61, so, ln, cols, codes, table, source="csv", src_samples=dec["n_samples"])
        got_host = sess.st_pack(61, so, ln, cols, codes, table, source="host", src_pool=dec["samples"],
                                batch_bytes=1000)
        sess.csv_arena_reserve(10, keep_filled=False)
        part = sess.csv_decode_part(text, 0)
        got_arena = sess.st_pack(61, part["sample_offset"], ln, cols, codes, table, source="arena",
                                 src_samples=part["n_samples"])
        off, _ = sess.pool_gather(so, ln, dec["samples"], download=False)
        got_pool = sess.st_pack(61, off, ln, cols, codes, table, source="pool", src_samples=int(ln.sum()),
                                batch_bytes=1)
        for got in (got_csv, got_host, got_arena, got_pool):
            assert got.tobytes() == want.tobytes()
        with pytest.raises(ValueError, match="outside the source"):
            sess.st_pack(61, so + 5, ln, cols, codes, table, source="host", src_pool=dec["samples"])
        with pytest.raises(ValueError, match="polarity code"):
            sess.st_pack(61, so, ln, cols, codes + 3, table, source="host", src_pool=dec["samples"])
    assert SB.check_st_layout(61) == want.dtype
