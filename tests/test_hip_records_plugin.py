"""HipRecordsPlugin / HipWavePoolPlugin on the GPU: raw files -> records + wave_pool through a Context, against the
bundles of the reference's builders (vx2730csv_files.npz, v1725bin_files.npz) and plugins
(vx2730csv_records_plugin.npz); the multi-part CSV decode into the session's sample arena against the one-part build
and the oracle; one build per run; the gathered pool handed to hit_threshold without another upload."""

import json
import os

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from waveformanalysis_amd import _lib
from waveformanalysis_amd import records_builder as RB
from waveformanalysis_amd.device import DeviceSession, default_pool
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipThresholdHitPlugin
from waveformanalysis_amd.plugins import records as R

pytestmark = pytest.mark.gpu


class RunCtx(SimpleContext):
    def __init__(self, *a, run_config=None, **kw):
        super().__init__(*a, **kw)
        self.run_config = run_config or {}

    def get_run_config(self, run_id):
        return self.run_config


def _write(tmp_path, groups, mtime=None):
    paths = []
    for g in groups:
        paths.append([])
        for fname, text in g:
            p = tmp_path / fname
            p.write_bytes(text)
            if mtime is not None:
                os.utime(p, (mtime, mtime))
            paths[-1].append(str(p))
    return paths


def _plugins(part_bytes=None):
    return [R.HipRecordsPlugin(part_bytes), R.HipWavePoolPlugin(part_bytes)]


def _run(config, raw_files, part_bytes=None, run_config=None, run_id="r0"):
    ctx = RunCtx(config, {"raw_files": raw_files}, _plugins(part_bytes), run_config=run_config)
    return ctx, ctx.get_data(run_id, "records"), ctx.get_data(run_id, "wave_pool")


def test_vx2730_variants_match_reference_bundles(tmp_path):
    groups, variants, fx = G.load_vx2730csv()
    paths = _write(tmp_path, groups)
    for k, v in enumerate(variants):
        cfg = {"dt": v["default_dt_ns"], "show_progress": False}
        if "baseline_samples" in v:
            cfg["baseline_samples"] = v["baseline_samples"]
        if "part_size" in v:
            cfg["records_part_size"] = v["part_size"]   # does not change the output
        if "epoch_ns" not in v:
            cfg["daq_adapter"] = None                      # no adapter: no file epoch, like the builder fixture
            _ctx, rec, pool = _run(cfg, paths)
            G.assert_struct_equal(rec, fx[f"records_{k}"], what=f"variant {k}")
            np.testing.assert_array_equal(pool, fx[f"wave_pool_{k}"])
            continue
        _ctx, rec, pool = _run(cfg, paths)                 # vx2730 adapter: epoch of the first file
        st = os.stat(paths[0][0])
        epoch = int(getattr(st, "st_birthtime", st.st_mtime) * 1e9)
        want, want_pool = O.build_records_from_vx2730_texts([[t for _f, t in g] for g in groups],
                                                             default_dt_ns=v["default_dt_ns"],
                                                             baseline_samples=v["baseline_samples"], epoch_ns=epoch)
        G.assert_struct_equal(rec, want, what=f"variant {k}")
        np.testing.assert_array_equal(pool, want_pool)
        keep = [n for n in rec.dtype.names if n != "time"]
        G.assert_struct_equal(rec[keep], fx[f"records_{k}"][keep], what=f"variant {k} without time")


def test_v1725_duplicate_path_matches_reference(tmp_path):
    z = np.load(os.path.join(G.GOLDEN, "v1725bin_files.npz"), allow_pickle=False)
    names = bytes(z["names"]).decode().split("\n")
    paths = []
    for k, name in enumerate(names):
        (tmp_path / name).write_bytes(bytes(z[f"blob{k}"]))
        paths.append(str(tmp_path / name))
    _ctx, rec, pool = _run({"daq_adapter": "v1725"}, [[paths[0], paths[1]], [paths[2], paths[0]], []])
    G.assert_struct_equal(rec, z["records"])                 # dt 4 from the adapter's 250 MHz
    np.testing.assert_array_equal(pool, z["wave_pool"])


def test_polarity_matches_reference_plugins(tmp_path):
    z = np.load(os.path.join(G.GOLDEN, "vx2730csv_records_plugin.npz"), allow_pickle=False)
    opt = json.loads(bytes(z["options_json"]).decode())
    cfg = {"channel_metadata": opt["metadata_context"]}
    run_cfg = {"channel_metadata": opt["metadata_run"]}
    groups, _variants, _fx = G.load_vx2730csv()
    paths = _write(tmp_path, groups, mtime=opt["file_mtime"])
    _ctx, rec, pool = _run(cfg | {"daq_adapter": "vx2730"}, paths, run_config=run_cfg, run_id=opt["run_id"])
    G.assert_struct_equal(rec, z["vx2730_records"], what="vx2730")
    np.testing.assert_array_equal(pool, z["vx2730_wave_pool"])

    v = np.load(os.path.join(G.GOLDEN, "v1725bin_files.npz"), allow_pickle=False)
    names = bytes(v["names"]).decode().split("\n")
    vpaths = []
    for k, name in enumerate(names):
        (tmp_path / name).write_bytes(bytes(v[f"blob{k}"]))
        vpaths.append(str(tmp_path / name))
    raw = [[vpaths[i] for i in g] for g in opt["v1725_groups"]]
    _ctx, rec, pool = _run(cfg | {"daq_adapter": "v1725"}, raw, run_config=run_cfg, run_id=opt["run_id"])
    G.assert_struct_equal(rec, z["v1725_records"], what="v1725")
    np.testing.assert_array_equal(pool, z["v1725_wave_pool"])


def test_small_parts_equal_one_part(tmp_path):
    groups, _variants, _fx = G.load_vx2730csv()
    paths = _write(tmp_path, groups)
    with DeviceSession(0) as sess:
        one = RB.build_records_from_vx2730_files(paths, 2, 25, session=sess)
        bodies = [RB.vx2730_body(t, k == 0) for g in groups for k, (_f, t) in enumerate(g)]
        for part_bytes in (1024, 1500, 2048, 3000, 4096):
            plan = RB.vx2730_parts([b for b in bodies if b], part_bytes)
            assert len(plan) > 1 and any(b < len(bodies[f]) for p in plan for f, _a, b in p)  # a file cut mid-way
            got = RB.build_records_from_vx2730_files(paths, 2, 25, session=sess, part_bytes=part_bytes)
            G.assert_struct_equal(got.records, one.records, what=f"part_bytes={part_bytes}")
            np.testing.assert_array_equal(got.wave_pool, one.wave_pool)
    cfg = {"daq_adapter": None, "dt": 2}
    _ctx, rec, pool = _run(cfg, paths, part_bytes=1024)
    _ctx, rec1, pool1 = _run(cfg, paths)
    G.assert_struct_equal(rec, rec1)
    np.testing.assert_array_equal(pool, pool1)


def _big_run(tmp_path, seed=11, files_per_channel=4, rows_per_file=2500, L=1000):
    """3 channels x 4 files x 2500 rows x 1000 samples = 3e7 samples, timestamp ties across channels."""
    rng = np.random.default_rng(seed)
    tbl = [str(i).encode() for i in range(65536)]
    groups = []
    for ch in range(3):
        group = []
        for k in range(files_per_channel):
            ts = np.sort(rng.integers(0, 5000, rows_per_file)) * 1000 + k * 10**7
            waves = rng.integers(0, 16384, (rows_per_file, L)).astype(np.uint16)
            waves[:, ::97] = rng.integers(0, 10, (rows_per_file, len(range(0, L, 97))))   # short fields too
            lines = [b"%d;%d;%d;1;2;0x1f;1;" % (ch // 2, ch, t) + b";".join(map(tbl.__getitem__, w.tolist()))
                     for t, w in zip(ts.tolist(), waves)]
            head = b"BOARD;CHANNEL;TIMETAG;ENERGY;ENERGYSHORT;FLAGS;PROBE_CODE;SAMPLES\n" if k == 0 else b""
            group.append((f"DataR_CH{ch}@big_{k}.CSV", head + b"\n".join(lines) + b"\n"))
        groups.append(group)
    return groups


def test_large_run_in_16mib_parts_matches_oracle(tmp_path):
    groups = _big_run(tmp_path)
    paths = _write(tmp_path, groups)
    bodies = [RB.vx2730_body(t, k == 0) for g in groups for k, (_f, t) in enumerate(g)]
    plan = RB.vx2730_parts(bodies, 16 << 20)
    assert len(plan) > 4 and any(b < len(bodies[f]) for p in plan for f, _a, b in p)
    with DeviceSession(0) as sess:
        got = RB.build_records_from_vx2730_files(paths, 2, (5, 105), session=sess, part_bytes=16 << 20)
        filled, cap = sess.csv_arena_filled()
    assert filled == len(got.wave_pool) == 3 * 10**7 and cap >= filled
    want, want_pool = O.build_records_from_vx2730_texts([[t for _f, t in g] for g in groups], default_dt_ns=2,
                                                         baseline_samples=(5, 105))
    G.assert_struct_equal(got.records, want)
    np.testing.assert_array_equal(got.wave_pool, want_pool)


def test_arena_refuses_parts_outside_the_reserve():
    with DeviceSession(0) as sess:
        lib, h = _lib.load(), sess._h
        text = np.frombuffer(b"1;2;3;4;5;6;7;10;11\n1;2;4;4;5;6;7;12;13\n", dtype=np.uint8)
        sess.csv_arena_reserve(3)
        import ctypes as C

        n, ns = C.c_int64(0), C.c_int64(0)
        _lib.check(lib.wfa_csv_arena_count(h, text.ctypes.data, text.size, ord(";"), 7, C.byref(n), C.byref(ns)))
        assert (n.value, ns.value) == (2, 4)
        cols = np.array([0, 1, 2], dtype=np.int32)
        meta = np.zeros((2, 3), dtype=np.int64)
        so = np.zeros(2, dtype=np.int64)
        for base in (0, 1, -1):   # 4 samples do not fit in 3; base 1 is past the filled extent 0
            with pytest.raises(ValueError, match="arena part"):
                _lib.check(lib.wfa_csv_arena_fill(h, base, 2, 3, cols.ctypes.data, meta.ctypes.data, None, None,
                                                  so.ctypes.data, 4))
        d = sess.csv_decode_part(text, 0)            # grows the arena
        np.testing.assert_array_equal(d["sample_offset"], [0, 2])
        d = sess.csv_decode_part(text, 4)
        np.testing.assert_array_equal(d["sample_offset"], [4, 6])
        assert sess.csv_arena_filled()[0] == 8
        off, pool = sess.csv_arena_gather([6, 0, 4], [2, 2, 1])
        np.testing.assert_array_equal(pool, [12, 13, 10, 11, 10])
        np.testing.assert_array_equal(off, [0, 2, 4])
        with pytest.raises(ValueError, match="outside the source pool of 8 samples"):
            sess.csv_arena_gather([7], [2])
        sess.release_scratch()                       # the arena stays
        assert sess.csv_arena_filled()[0] == 8
        off, pool = sess.csv_arena_gather([2], [2])
        np.testing.assert_array_equal(pool, [12, 13])


def test_records_then_wave_pool_builds_once(tmp_path, monkeypatch):
    groups, _variants, fx = G.load_vx2730csv()
    paths = _write(tmp_path, groups)
    calls = []
    real = RB.build_records_from_vx2730_files

    def counted(*a, **kw):
        calls.append(kw.get("part_bytes"))
        return real(*a, **kw)

    monkeypatch.setattr(RB, "build_records_from_vx2730_files", counted)
    ctx, rec, pool = _run({"daq_adapter": None, "dt": 2}, paths, part_bytes=2048)
    assert len(calls) == 1 and calls[0] == 2048
    assert ctx.get_data("r0", "wave_pool") is pool
    keys = [k for k in ctx._results if k[1].startswith("_records_bundle")]
    assert keys == [("r0", "_records_bundle-r0-records-key")]
    np.testing.assert_array_equal(pool, fx["wave_pool_0"])
    ctx.get_data("r1", "wave_pool")                  # another run builds again
    assert len(calls) == 2


def test_resident_pool_reaches_hit_threshold(tmp_path, monkeypatch):
    """records -> wave_pool -> hit_threshold on one context: the hit pass finds the gathered pool on the device (no
    upload), also after extra cleanup() calls, which keep the arena and the gathered pool."""
    groups, _variants, _fx = G.load_vx2730csv()
    paths = _write(tmp_path, groups)
    hit_cfg = {"wave_source": "records", "threshold": 8.0}
    plugins = _plugins(1500)
    ctx = RunCtx({"daq_adapter": None, "dt": 2, "hit_threshold": hit_cfg}, {"raw_files": paths},
                 plugins + [HipThresholdHitPlugin()])
    rec = ctx.get_data("r0", "records")
    pool = ctx.get_data("r0", "wave_pool")
    for p in plugins:
        p.cleanup(ctx)
    sess = default_pool().session()
    assert sess.csv_arena_filled()[0] == len(pool)
    uploads = []
    real = DeviceSession.upload_pool

    def counted(self, p):
        uploads.append(len(p))
        return real(self, p)

    monkeypatch.setattr(DeviceSession, "upload_pool", counted)
    hits = ctx.get_data("r0", "hit_threshold")
    assert uploads == [] and len(hits) > 0
    monkeypatch.setattr(DeviceSession, "upload_pool", real)
    plain = SimpleContext({"hit_threshold": hit_cfg}, {"records": rec.copy(), "wave_pool": pool.copy()},
                          [HipThresholdHitPlugin()])
    want = plain.get_data("r0", "hit_threshold")
    assert hits.dtype == want.dtype and hits.tobytes() == want.tobytes()
