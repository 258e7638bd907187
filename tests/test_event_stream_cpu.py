"""The event stream without a GPU: the carry-and-horizon rule (numpy restatement, tests/event_stream_util.py) against the
frames the reference recorded, the horizons HipHitGroupedStream computes, its call sequence and refusals on a device
double, the profile, the declared C symbols and events_frame."""

import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import event_stream_util as E
from tests import stream_hits_util as S
from waveformanalysis_amd import _lib, plugins
from waveformanalysis_amd.dtypes import EVENT_HIT_DTYPE, RECORDS_DTYPE
from waveformanalysis_amd.event_grouping import EVENT_COLUMNS
from waveformanalysis_amd.event_stream import (
    HipHitGroupedStream,
    abs_windows,
    chunk_horizons,
    events_frame,
    horizon_margin,
    horizon_of,
    run_magnitude,
)
from waveformanalysis_amd.plugin_api import SimpleContext

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("wfa_event_stream_begin", "wfa_event_stream_push", "wfa_event_stream_fill", "wfa_event_stream_end")


def _ctx(run, config=None, pool=None):
    ctx = SimpleContext({"wave_source": "records", **(config or {})}, {"wave_pool": run.pool, "records": run.records})
    if pool is not None:
        ctx.wfa_device_pool = pool
    return ctx


# ---- the rule ----------------------------------------------------------------------------------------------------------
def _assert_recorded(rows, z, tag):
    ids = rows["event_id"]
    starts = np.concatenate([[0], np.flatnonzero(np.diff(ids)) + 1])
    np.testing.assert_array_equal(ids[starts], np.arange(len(starts)))
    np.testing.assert_array_equal(rows["t_min"][starts], z[f"{tag}_t_min"])
    np.testing.assert_array_equal(rows["t_max"][starts], z[f"{tag}_t_max"])
    np.testing.assert_array_equal(np.diff(np.concatenate([starts, [len(rows)]])), z[f"{tag}_n_hits"])
    for column, field in E.PER_HIT:
        np.testing.assert_array_equal(rows[field], z[f"{tag}_{column}"], err_msg=f"{tag} {column}")


@pytest.mark.parametrize("name", E.GOLDEN_TABLES)
def test_rule_gives_the_static_events_and_the_recorded_frames(name):
    hits, windows, z = E.golden(name)
    n = len(hits)
    assert len(windows) == 4
    for w in windows:
        tag = f"w{int(w)}"
        want = E.static_rows(hits, w)
        _assert_recorded(want, z, tag)
        for chunk_size in (1, 2, 3, 7, 64, 1000, n, n + 1):
            stream = E.NumpyStream(w)
            got = E.stream_rows(stream.push, hits, chunk_size)
            assert got.tobytes() == want.tobytes(), (name, w, chunk_size)
            if chunk_size in (1, 7, 64):
                _assert_recorded(got, z, tag)


def test_rule_boundary_is_strict():
    # event [0, 4000] ps, window 1 ns: max + gap = 5000.  A later hit at 5000 joins (static rule: opens iff >).
    hits = E.make_hits([(0, 4000, 0, 0), (5000, 2000, 0, 1), (50_000, 2000, 0, 0)])
    want = E.static_rows(hits, 1.0)
    assert want["event_id"].tolist() == [0, 0, 1]
    stream = E.NumpyStream(1.0)
    out, carry = stream.push(hits[:1], 5000.0)          # max + gap == H: stays open
    assert len(out) == 0 and carry == 1
    stream = E.NumpyStream(1.0)
    out, carry = stream.push(hits[:1], 5001.0)          # one ps more: closes
    assert len(out) == 1 and carry == 0


# ---- horizons ----------------------------------------------------------------------------------------------------------
def _brute_horizons(chunks):
    out = []
    for k in range(len(chunks)):
        later = [int(c.data["timestamp"].min()) for c in chunks[k + 1:] if len(c.data)]
        out.append(float(min(later)) if later else math.inf)
    return out


@pytest.mark.parametrize("name,chunk_size", [("ragged", 50), ("shuffled", 50), ("mixed", 100), ("ragged", 1)])
def test_horizons_of_the_fixture_runs(name, chunk_size):
    run = S.run(name)
    chunks = run.chunks(chunk_size)
    got = chunk_horizons(chunks)
    assert got == _brute_horizons(chunks) and got[-1] == math.inf
    assert all(a <= b for a, b in zip(got[:-1], got[1:]))
    # every hit of a later chunk starts at or above the horizon
    want = run.want(False)
    a0, _ = abs_windows(want)
    chunk_of = {int(r): k for k, c in enumerate(chunks) for r in c.data["record_id"]}
    k_of_row = np.array([chunk_of[int(r)] for r in want["record_id"]])
    for k, h in enumerate(got):
        assert not np.any(a0[k_of_row > k] < h)
    if name == "mixed":   # a time break between two chunks is just a larger step of the horizon
        assert max(b - a for a, b in zip(got[:-2], got[1:-1])) > 10**13


def test_horizons_of_an_unsorted_run_and_empty_chunks():
    rec = S.run("ragged").records
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(rec))
    chunks = [SimpleNamespace(data=rec[perm[lo : lo + 37]]) for lo in range(0, len(rec), 37)]
    chunks.insert(3, SimpleNamespace(data=rec[:0]))
    got = chunk_horizons(chunks)
    assert got == _brute_horizons(chunks)
    assert got[2] == got[3]            # a chunk without records changes nothing
    assert chunk_horizons([]) == []


def test_margin_rule():
    assert horizon_margin(2**53 - 1) == 0.0 and horizon_of(12345, 0.0) == 12345.0
    assert horizon_margin(2**53) == 4.0
    assert horizon_margin(2**60) == 512.0           # one ulp is 256 ps
    assert horizon_margin(2**62) == 2048.0
    assert horizon_of(None, 512.0) == math.inf
    h = horizon_of(2**60 + 1000, 512.0)
    assert h < float(2**60 + 1000) - 512.0 and h >= float(2**60 + 1000) - 512.0 - 256.0
    rec = np.zeros(2, dtype=RECORDS_DTYPE)
    rec["timestamp"], rec["dt"], rec["event_length"] = [2**60, 2**60 + 10**6], 4, [100, 50]
    assert run_magnitude(rec) == 2**60 + 10**6 + 4 * 1000 * 100
    # the bound holds for hits whose windows round: brute force around 2^60 and 2^62 with dt = 3 ns
    rng = np.random.default_rng(9)
    for base in (2**60, 2**62 - 10**9):
        rec_ts = base + rng.integers(0, 10**8, 2000)
        pos, start = rng.integers(0, 500, 2000), rng.integers(0, 500, 2000)
        hits = np.zeros(2000, dtype=E.THRESHOLD_HIT_DTYPE)
        hits["dt"], hits["position"], hits["edge_start"] = 3, pos, np.minimum(start, pos)
        hits["timestamp"] = rec_ts + pos * 3000
        a0, _ = abs_windows(hits)
        margin = horizon_margin(int(rec_ts.max()) + 500 * 3000)
        assert np.all(a0 >= np.array([horizon_of(int(t), margin) for t in rec_ts]))
        assert np.any(a0 < rec_ts.astype(np.float64)) or base < 2**61   # without the margin the bound fails


# ---- the plugin on a device double ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,chunk_size,workers", [("ragged", 50, 1), ("ragged", 50, 4), ("mixed", 100, 4),
                                                     ("shuffled", 7, 4), ("sparse", 60, 4), ("ragged", 1000, 4)])
def test_plugin_rows_equal_the_static_rule(name, chunk_size, workers):
    run = S.run(name)
    pool = E.event_pool()
    plugin = HipHitGroupedStream(device_pool=pool, time_window_ns=100.0)
    plugin.chunk_size = chunk_size
    outs = list(plugin.run_chunks(run.chunks(chunk_size), _ctx(run), "run", max_workers=workers))
    want = E.static_rows(run.want(False), 100.0)
    got = np.concatenate([o.data for o in outs])
    assert got.dtype == EVENT_HIT_DTYPE and got.tobytes() == want.tobytes()
    for o in outs:
        assert len(o.data) and (o.start, o.end) == (int(o.data["t_min"].min()), int(o.data["t_max"].max()) + 1)
        assert o.data_type == "hit_grouped_stream" and o.time_field == "t_min"
    assert plugin.stats["rows_in"] == plugin.stats["rows_out"] == len(want)
    assert plugin.stats["events"] == int(want["event_id"][-1]) + 1


def test_compute_chunks_the_records_of_the_context():
    run = S.run("mixed")
    pool = E.event_pool()
    ctx = _ctx(run, {"time_window_ns": 5000.0}, pool)
    outs = list(HipHitGroupedStream().compute(ctx, "run", streaming_config={"chunk_size": 100}))
    want = E.static_rows(run.want(False), 5000.0)
    assert np.concatenate([o.data for o in outs]).tobytes() == want.tobytes()
    pushes = [c for c in pool.calls if c[0] == "push"]
    assert len(pushes) == len(run.chunks(100)) + 1
    frame = events_frame(want)
    assert list(frame.columns) == EVENT_COLUMNS and len(frame) == int(want["event_id"][-1]) + 1


def test_call_sequence_with_hitless_and_empty_chunks():
    run = S.run("sparse")
    chunks, k_empty = S.sparse_chunks_with_empty()
    pool = E.event_pool()
    plugin = HipHitGroupedStream(device_pool=pool)
    list(plugin.run_chunks(chunks, _ctx(run), "run", max_workers=4))
    calls = pool.calls
    assert calls[0][:2] == ("begin", 100.0) and calls[-1][0] == "end"
    pushes = calls[1:-1]
    assert [c[0] for c in pushes] == ["push"] * (len(chunks) + 1)
    assert len({id(c[-1]) for c in calls}) == 1                       # one session for the whole run
    want = run.want(False)
    per_chunk = [int(np.isin(want["record_id"], c.data["record_id"]).sum()) for c in chunks]
    assert [c[1] for c in pushes] == per_chunk + [0]
    assert per_chunk[k_empty] == 0 and 0 in [n for k, n in enumerate(per_chunk) if k != k_empty]   # hitless chunks too
    assert [c[2] for c in pushes[:-1]] == chunk_horizons(chunks) and pushes[-1][2] == math.inf
    assert calls[0][-1] not in [e["session"] for e in pool.log]       # the ring's sessions are others


@pytest.mark.parametrize("workers", (1, 4))
def test_end_is_called_when_a_chunk_raises(workers, monkeypatch):
    run = S.run("ragged")
    pool = E.event_pool()
    seen = []

    def failing_wait(self):
        seen.append(1)
        if len(seen) == 3:
            raise _lib.WfaError(_lib.WFA_E_HIP, "injected")
        return len(self._rows)

    monkeypatch.setattr(E.EventOracleSession, "hits_wait", failing_wait)
    plugin = HipHitGroupedStream(device_pool=pool)
    with pytest.raises(_lib.WfaError, match="injected"):
        list(plugin.run_chunks(run.chunks(50), _ctx(run), "run", max_workers=workers))
    assert [c[0] for c in pool.calls] == ["begin", "push", "push", "end"]
    assert len(pool._free) == pool._borrowable                        # every session is back in the pool


def test_refusals_before_any_upload():
    run = S.run("ragged")
    for config in ({"hit_merged": {"merge_gap_ns": 20.0}}, {"merge_gap_ns": 5}, {"hit_merged.merge_gap_ns": 1.0}):
        pool = E.event_pool()
        with pytest.raises(ValueError, match="merge_gap_ns"):
            list(HipHitGroupedStream(device_pool=pool).compute(_ctx(run, config), "run"))
        assert pool.uploads == [] and pool.calls == []
    pool = E.event_pool()
    list(HipHitGroupedStream(device_pool=pool).compute(_ctx(run, {"merge_gap_ns": 0.0}), "run"))   # nothing is merged
    small = E.event_pool(max_sessions=2)
    with pytest.raises(ValueError, match="max_sessions >= 3"):
        list(HipHitGroupedStream(device_pool=small).compute(_ctx(run), "run"))
    assert small.uploads == [] and small.calls == []
    with pytest.raises(ValueError, match="time_window_ns must be >= 0"):
        HipHitGroupedStream(time_window_ns=-1.0)
    with pytest.raises(ValueError, match="time_window_ns must be >= 0"):
        list(HipHitGroupedStream(device_pool=E.event_pool()).compute(_ctx(run, {"time_window_ns": -5.0}), "run"))
    with pytest.raises(TypeError, match="unknown options"):
        HipHitGroupedStream(bogus=1)
    with pytest.raises(NotImplementedError):
        HipHitGroupedStream().compute_chunk(run.chunks(50)[0], _ctx(run), "run")


def test_a_pool_of_three_sessions_suffices():
    run = S.run("ragged")
    pool = E.event_pool(max_sessions=3)
    outs = list(HipHitGroupedStream(device_pool=pool).run_chunks(run.chunks(50), _ctx(run), "run", max_workers=4))
    assert np.concatenate([o.data for o in outs]).tobytes() == E.static_rows(run.want(False), 100.0).tobytes()
    assert pool._borrowable == 3


def test_option_precedence_and_pass_through():
    run = S.run("ragged")
    pool = E.event_pool()
    ctx = _ctx(run, {"threshold": 250.0, "time_window_ns": 7.0, "hit_grouped_stream": {"right_extension": 1}}, pool)
    plugin = HipHitGroupedStream(threshold=S.THRESHOLD, left_extension=S.LE)
    cfg = plugin._configure(ctx)
    assert (cfg["threshold"], cfg["left_extension"], cfg["right_extension"], cfg["time_window_ns"]) == (S.THRESHOLD, S.LE, 1, 7.0)
    inner = plugin._inner(cfg, pool)
    inner._configure(ctx)       # the Context cannot win over what the outer stream resolved
    assert (inner.threshold, inner.le, inner.re) == (S.THRESHOLD, S.LE, 1)
    assert HipHitGroupedStream(time_window_ns=3.0)._configure(ctx)["time_window_ns"] == 3.0
    assert HipHitGroupedStream().cfg["time_window_ns"] == 100.0 and HipHitGroupedStream().cfg["dt"] is None
    # use_filtered reaches the hit pass
    plugin = HipHitGroupedStream(device_pool=pool, use_filtered=True)
    outs = list(plugin.run_chunks(run.chunks(150), _ctx(run), "run"))
    assert {e["source"] for e in pool.log} == {_lib.SRC_SG_FUSED}
    assert np.concatenate([o.data for o in outs]).tobytes() == E.static_rows(run.want(True), 100.0).tobytes()
    inner = HipHitGroupedStream(filter_source="wave_pool_filtered", use_filtered=True)
    assert inner._inner(inner.cfg, pool).filter_source == "wave_pool_filtered"


def test_plugin_contract_and_profiles():
    p = HipHitGroupedStream()
    assert p.provides == "hit_grouped_stream" and p.depends_on == ["records", "wave_pool"]
    assert p.is_stateful is True and p.reset_on_break is False and p.save_when == "never"
    assert p.output_dtype == EVENT_HIT_DTYPE and EVENT_HIT_DTYPE.itemsize == 84
    assert [EVENT_HIT_DTYPE.fields[n][1] for n in ("event_id", "t_min", "t_max", "position")] == [0, 8, 16, 24]
    assert {"time_window_ns", "dt", "threshold", "channel_config", "filter_source"} <= set(p.options)
    assert p.options["time_window_ns"].default == 100.0
    assert [q.provides for q in plugins.hip_streaming()] == ["hit_threshold_stream", "signal_peaks_stream", "s1_s2_stream"]
    assert [q.provides for q in plugins.hip_streaming_events()] == \
        ["hit_threshold_stream", "signal_peaks_stream", "s1_s2_stream", "hit_grouped_stream"]
    assert "hip_streaming_events" in plugins.__all__


# ---- the C boundary ----------------------------------------------------------------------------------------------------
def test_declared_symbols_and_abi_version():
    header = open(os.path.join(REPO, "include", "wfa_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES, name
    assert int(re.search(r"#define WFA_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 7
    assert _lib.load().wfa_abi_version() == _lib.ABI_VERSION


def test_entry_points_refuse_a_null_context():
    lib = _lib.load()
    n = C.c_int64(0)
    rows = np.zeros(1, dtype=E.THRESHOLD_HIT_DTYPE)
    assert lib.wfa_event_stream_begin(None, 100.0) == _lib.WFA_E_INVALID
    assert "ctx is null" in _lib.last_error()
    assert lib.wfa_event_stream_push(None, rows.ctypes.data_as(C.c_void_p), 1, 0.0, C.byref(n), C.byref(n), C.byref(n)) == \
        _lib.WFA_E_INVALID
    assert lib.wfa_event_stream_fill(None, None, 0) == _lib.WFA_E_INVALID
    assert lib.wfa_event_stream_end(None) == _lib.WFA_E_INVALID


# ---- events_frame ------------------------------------------------------------------------------------------------------
def test_events_frame_on_hand_made_rows():
    hits = E.make_hits([(1000, 4000, 0, 1), (2000, 4000, 0, 0), (900_000, 4000, 1, 0, 4)])
    rows = E.static_rows(hits, 100.0)
    frame = events_frame(rows)
    assert list(frame.columns) == EVENT_COLUMNS and len(frame) == 2
    assert frame["event_id"].tolist() == [0, 1] and frame["n_hits"].tolist() == [2, 1]
    assert frame["t_min"].tolist() == [1000, 900_000] and frame["t_max"].tolist() == [6000, 904_000]
    assert frame["dt/ns"].tolist() == [5.0, 4.0]
    assert frame["channels"][0].tolist() == [0, 1] and frame["timestamps"][0].tolist() == [2000, 1000]
    assert frame["boards"][1].tolist() == [1] and frame["dt"][1].tolist() == [4]
    assert frame["sample_starts"][0].tolist() == [10, 10] and frame["sample_ends"][0].tolist() == [12, 12]
    for column, dtype in (("dt", np.int32), ("boards", np.int16), ("channels", np.int16), ("heights", np.float32),
                          ("integrals", np.float32), ("timestamps", np.int64), ("record_ids", np.int64),
                          ("sample_starts", np.int32), ("sample_ends", np.int32)):
        assert frame[column][0].dtype == dtype, column
    assert str(frame["event_id"].dtype) == "int64" and str(frame["dt/ns"].dtype) == "float64"
    empty = events_frame(rows[:0])
    assert list(empty.columns) == EVENT_COLUMNS and len(empty) == 0
    # ids that do not start at 0 (the rows of one push) keep their values
    assert events_frame(rows[2:])["event_id"].tolist() == [1]
