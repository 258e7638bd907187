"""The df_events stream without a GPU: the carry-and-horizon rule (numpy restatement, tests/df_event_stream_util.py)
against the static host pass and the frames the reference recorded, df_rows and the horizons, the host refusals and the
call sequence of both plugins on a device double, the frame helpers, event_index across time segments, the profile and
the declared C symbols."""

import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest

from tests import df_event_stream_util as D
from tests import events_util as E
from tests import stream_hits_util as S
from waveformanalysis_amd import _lib, plugins
from waveformanalysis_amd.df_event_stream import (
    HORIZON_END,
    HipGroupedEventsStream,
    chunk_horizons_ts,
    df_rows,
    grouped_events_frame,
    paired_events_frame,
)
from waveformanalysis_amd.dtypes import BASIC_FEATURES_DTYPE, DF_EVENT_ROW_DTYPE, DF_ROW_DTYPE
from waveformanalysis_amd.event_grouping import MULTI_CHANNEL_COLUMNS, _group_multi_channel_order_host
from waveformanalysis_amd.features_stream import HipBasicFeaturesStream
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins.event_analysis import build_events_frame, pair_events

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("wfa_df_event_stream_begin", "wfa_df_event_stream_push", "wfa_df_event_stream_fill",
                "wfa_df_event_stream_end")
Z = D.fixture()


def _ctx(run, config=None, pool=None):
    ctx = SimpleContext({"wave_source": "records", **(config or {})}, {"wave_pool": run.pool, "records": run.records})
    if pool is not None:
        ctx.wfa_device_pool = pool
    return ctx


def _model_rows(rows, window_ns, chunk_size, carries=None):
    return D.stream_rows(D.NumpyDfStream(window_ns).push, rows, chunk_size, carries)


# ---- the rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", (0, 10**9, 2**53 - 500, 2**60, 2**62))
@pytest.mark.parametrize("shuffle", (False, True))
def test_model_equals_the_static_host_pass_on_random_runs(base, shuffle):
    rng = np.random.default_rng(base % 1000 + int(shuffle))
    for trial in range(4):
        n = int(rng.integers(1, 120))
        ts = base + np.cumsum(rng.integers(0, 4, n) * rng.choice([0, 1, 100_000, 3_000_000], n)).astype(np.int64)
        if shuffle:   # unsorted inside a bounded stretch: horizons are suffix minima, never the last row's timestamp
            ts = ts[np.argsort(np.arange(n) + rng.integers(-6, 7, n), kind="stable")]
        rows = D.make_rows(ts, rng.integers(0, 5, n))
        for window_ns in (0.0, 0.0005, 0.001, 100.0, 5000.0):
            want = D.static_rows(rows, window_ns)
            order, bounds = _group_multi_channel_order_host(rows["timestamp"], rows["channel"], window_ns * 1e3)
            np.testing.assert_array_equal(want["record_id"], order)       # record_id = input row
            assert int(want["event_id"][-1]) + 1 == len(bounds) - 1
            for chunk_size in (1, 2, 7, 64, n):
                got = _model_rows(rows, window_ns, chunk_size)
                assert got.tobytes() == want.tobytes(), (base, shuffle, trial, window_ns, chunk_size)


@pytest.mark.parametrize("case", D.FIXTURE_CASES)
def test_model_gives_the_recorded_frames_at_every_chunk_size(case):
    rows, window_ns = D.fixture_rows(Z, case)
    assert len(rows) == 300
    want = D.static_rows(rows, window_ns)
    E.assert_frame_matches(grouped_events_frame(want), Z, f"{case}/df_events")
    E.assert_frame_matches(paired_events_frame(want, **D.pairing_args(Z, case)), Z, f"{case}/df_paired")
    by_time = rows[np.argsort(rows["timestamp"], kind="stable")]         # the order of df; the table's own is another
    assert by_time.tobytes() != rows.tobytes()
    for chunk_size in (1, 7, 64, 300):
        carries = []
        assert _model_rows(rows, window_ns, chunk_size).tobytes() == want.tobytes(), (case, chunk_size)
        assert _model_rows(by_time, window_ns, chunk_size, carries).tobytes() == want.tobytes(), (case, chunk_size)
        if chunk_size < 300:   # a time-sorted run holds back little
            assert max(carries[:-1]) <= 13, (case, chunk_size, max(carries))


def test_the_close_rule_is_strict_and_t_min_t_max_are_not_the_extremes():
    rows = D.make_rows([1000, 900, 1100, 500_000], [3, 5, 1, 0])
    m = D.NumpyDfStream(100.0)
    out, n_carry = m.push(rows[:3], 100_900)               # (double)H == (double)a + w with a = 900: held back
    assert len(out) == 0 and n_carry == 3
    out, n_carry = m.push(None, 100_901)
    assert n_carry == 0 and list(out["channel"]) == [1, 3, 5] and list(out["timestamp"]) == [1100, 1000, 900]
    assert set(out["t_min"]) == {1100} and set(out["t_max"]) == {900} and set(out["n_hits"]) == {3}
    out, n_carry = m.push(rows[3:], 500_000, True)
    assert list(out["event_id"]) == [1] and n_carry == 0


# ---- df_rows and the horizons --------------------------------------------------------------------------------------------
def test_df_rows_columns_and_dtypes():
    run = S.run("ragged")
    rec = run.records[10:20]
    bf = D.oracle_features(rec)
    bf["event_index"] += 10
    rows = df_rows(rec, bf)
    assert rows.dtype == DF_ROW_DTYPE and DF_ROW_DTYPE.itemsize == 40
    assert [DF_ROW_DTYPE.fields[n][1] for n in DF_ROW_DTYPE.names] == [0, 8, 16, 20, 24, 28, 32, 34, 36]
    assert [str(DF_ROW_DTYPE[n]) for n in DF_ROW_DTYPE.names] == \
        ["int64", "int64", "float32", "float32", "float32", "float32", "int16", "int16", "uint32"]
    for name in ("timestamp", "record_id", "board", "channel"):
        np.testing.assert_array_equal(rows[name], rec[name])
    for name in ("area", "height", "amp", "max_abs_diff"):
        np.testing.assert_array_equal(rows[name], bf[name])
    assert not rows["reserved"].any()
    bare = rec[[n for n in rec.dtype.names if n not in ("record_id", "board")]]
    rows = df_rows(bare, bf)
    np.testing.assert_array_equal(rows["record_id"], 10 + np.arange(10))   # arange over the run, as HipDataFramePlugin
    assert not rows["board"].any()
    with pytest.raises(ValueError, match="basic_features length"):
        df_rows(rec, bf[:3])
    assert DF_EVENT_ROW_DTYPE.itemsize == 64
    assert [DF_EVENT_ROW_DTYPE.fields[n][1] for n in DF_EVENT_ROW_DTYPE.names] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60, 62]


def test_horizons_of_an_unsorted_run():
    run = S.run("ragged")
    rec = run.records[:40].copy()
    rec["timestamp"][20] = rec["timestamp"][3] + 1          # a late chunk begins with an early record
    chunks = S.records_to_chunks(rec, 10)
    assert chunk_horizons_ts(chunks) == [int(rec["timestamp"][3]) + 1] * 2 + [int(rec["timestamp"][30]), HORIZON_END]
    chunks.insert(1, S.empty_chunk_between(chunks[0], chunks[1]))   # an empty chunk takes the next one's horizon
    hs = chunk_horizons_ts(chunks)
    assert hs[0] == hs[1] and hs[-1] == HORIZON_END and all(a <= b for a, b in zip(hs, hs[1:]))
    assert chunk_horizons_ts([]) == []


# ---- the plugins on a device double -----------------------------------------------------------------------------------
def _static_features(run):
    bf = D.oracle_features(run.records)
    return bf


@pytest.mark.parametrize("name", ("ragged", "mixed", "shuffled"))
@pytest.mark.parametrize("chunk_size", (1, 7, 1000))
@pytest.mark.parametrize("workers", (1, 4))
def test_features_stream_rows_and_event_index(name, chunk_size, workers):
    """event_index counts through the run, across the time segments of `mixed` (first_record restarts in each)."""
    run = S.run(name)
    pool = D.df_event_pool()
    plugin = HipBasicFeaturesStream(device_pool=pool)
    outs = list(plugin.compute(_ctx(run), "run", streaming_config={"chunk_size": chunk_size, "max_workers": workers}))
    got = np.concatenate([o.data for o in outs])
    assert got.dtype == BASIC_FEATURES_DTYPE and got.tobytes() == _static_features(run).tobytes()
    np.testing.assert_array_equal(got["event_index"], np.arange(len(run.records)))
    if name == "mixed":
        assert any(o.metadata["first_record"] == 0 and o.metadata["record_base"] > 0 for o in outs)


def test_features_stream_cuts_the_pool_and_passes_the_fixed_baseline():
    run = S.run("shuffled")
    pool = D.df_event_pool()
    config = {"channel_config": {"0:1": {"fixed_baseline": 8001.5}, "0:3": {"fixed_baseline": 7999.0}}}
    plugin = HipBasicFeaturesStream(device_pool=pool, height_range=(3, 30), area_range=(2, 35), **config)
    chunk = run.chunks(50)[2]
    out = plugin.compute_chunk(chunk, _ctx(run), "run")
    kinds = [c[0] for c in pool.calls]
    assert kinds == ["upload_pool", "upload_records", "basic_features"]
    rec = chunk.data
    lo, hi = int(rec["wave_offset"].min()), int((rec["wave_offset"] + rec["event_length"]).max())
    assert pool.calls[0][1] == hi - lo
    call = pool.calls[2]
    assert call[2:4] == ((3, 30), (2, 35))
    want_fixed = np.where(rec["channel"] == 1, 8001.5, np.where(rec["channel"] == 3, 7999.0, np.nan))
    np.testing.assert_array_equal(call[4], want_fixed)
    np.testing.assert_array_equal(out.data["event_index"], np.arange(len(rec)) + 100)


@pytest.mark.parametrize("name", ("ragged", "mixed", "shuffled"))
@pytest.mark.parametrize("chunk_size", (1, 7, 1000))
@pytest.mark.parametrize("workers", (1, 4))
def test_events_stream_rows_equal_the_static_rule(name, chunk_size, workers):
    run = S.run(name)
    pool = D.df_event_pool()
    plugin = HipGroupedEventsStream(device_pool=pool, time_window_ns=600.0)
    plugin.chunk_size = chunk_size
    outs = list(plugin.run_chunks(run.chunks(chunk_size), _ctx(run), "run", max_workers=workers))
    want = D.static_rows(df_rows(run.records, _static_features(run)), 600.0)
    got = np.concatenate([o.data for o in outs])
    assert got.dtype == DF_EVENT_ROW_DTYPE and got.tobytes() == want.tobytes()
    assert int(want["n_hits"].max()) > 1                                   # (600 ns joins neighbouring records)
    first = 0
    for o in outs:
        assert len(o.data) and (o.start, o.end) == (int(o.data["t_min"].min()), int(o.data["t_max"].max()) + 1)
        assert o.data_type == "df_events_stream" and o.time_field == "t_min"
        assert o.metadata["first_event"] == first == int(o.data["event_id"][0]) and o.metadata["n_carry"] >= 0
        first = int(o.data["event_id"][-1]) + 1
    assert plugin.stats["rows_in"] == plugin.stats["rows_out"] == len(want)
    assert plugin.stats["events"] == int(want["event_id"][-1]) + 1


def test_run_chunks_numbers_the_chunks_it_is_given():
    """A record_base left in the metadata by another cut does not win (the records here have no record_id column, so
    record_id is the run index that event_index gives)."""
    run = S.run("mixed")
    bare = run.records[[n for n in run.records.dtype.names if n != "record_id"]]
    chunks = S.records_to_chunks(bare, 100)
    for c in chunks:
        c.metadata["record_base"] = 12345
    ctx = SimpleContext({"wave_source": "records"}, {"wave_pool": run.pool, "records": bare})
    plugin = HipGroupedEventsStream(device_pool=D.df_event_pool())
    rows = np.concatenate([o.data for o in plugin.run_chunks(chunks, ctx, "run", max_workers=1)])
    assert sorted(rows["record_id"].tolist()) == list(range(len(bare)))
    assert [c.metadata["record_base"] for c in chunks] == [12345] * len(chunks)     # the caller's chunks are untouched


def test_events_stream_call_sequence_with_an_empty_chunk():
    run = S.run("sparse")
    chunks, k_empty = S.sparse_chunks_with_empty()
    pool = D.df_event_pool()
    plugin = HipGroupedEventsStream(device_pool=pool)
    list(plugin.run_chunks(chunks, _ctx(run), "run", max_workers=4))
    stream_calls = [c for c in pool.calls if c[0] in ("begin", "push", "end")]
    assert stream_calls[0][:2] == ("begin", 100.0) and stream_calls[-1][0] == "end"
    pushes = stream_calls[1:-1]
    assert [c[0] for c in pushes] == ["push"] * len(chunks)               # no flush: the last chunk is final
    assert [c[1] for c in pushes] == [len(c.data) for c in chunks] and pushes[k_empty][1] == 0
    assert [c[2] for c in pushes] == chunk_horizons_ts(chunks)
    assert [c[3] for c in pushes] == [False] * (len(chunks) - 1) + [True]
    assert len({id(c[-1]) for c in stream_calls}) == 1                    # one session for the whole run
    assert stream_calls[0][-1] not in {c[-1] for c in pool.calls if c[0] == "basic_features"}


def test_compute_chunks_the_records_of_the_context_and_a_run_without_records_gives_nothing():
    run = S.run("mixed")
    pool = D.df_event_pool()
    ctx = _ctx(run, {"time_window_ns": 5000.0}, pool)
    outs = list(HipGroupedEventsStream().compute(ctx, "run", streaming_config={"chunk_size": 100}))
    want = D.static_rows(df_rows(run.records, _static_features(run)), 5000.0)
    assert np.concatenate([o.data for o in outs]).tobytes() == want.tobytes()
    empty = SimpleContext({"wave_source": "records"}, {"wave_pool": run.pool, "records": run.records[:0]})
    pool = D.df_event_pool()
    empty.wfa_device_pool = pool
    assert list(HipGroupedEventsStream().compute(empty, "run")) == []
    assert list(HipBasicFeaturesStream().compute(empty, "run")) == []
    assert [c[0] for c in pool.calls] == ["begin", "end"] and pool.uploads == []


def test_every_host_refusal_fires_before_any_session_call():
    run = S.run("ragged")
    refused = (({"use_filtered": True}, "use_filtered"), ({"fixed_baseline": {"0:1": 8000.0}}, "fixed_baseline"),
               ({"wave_source": "st_waveforms"}, "wave_source must be 'records'"),
               ({"wave_source": "auto"}, "wave_source must be 'records'"))
    for cls in (HipBasicFeaturesStream, HipGroupedEventsStream):
        for config, match in refused:
            with pytest.raises(ValueError, match=match):
                cls(**config)
            pool = D.df_event_pool()
            with pytest.raises(ValueError, match=match):
                list(cls(device_pool=pool).compute(_ctx(run, config), "run"))
            assert pool.calls == [] and pool.uploads == [], (cls, config)
    pool = D.df_event_pool()
    with pytest.raises(ValueError, match="time_window_ns must be >= 0"):
        list(HipGroupedEventsStream(device_pool=pool).compute(_ctx(run, {"time_window_ns": -5.0}), "run"))
    with pytest.raises(ValueError, match="time_window_ns must be >= 0"):
        HipGroupedEventsStream(time_window_ns=float("nan"))
    small = D.df_event_pool(max_sessions=2)
    with pytest.raises(ValueError, match="max_sessions >= 3"):
        list(HipGroupedEventsStream(device_pool=small).compute(_ctx(run), "run"))
    assert pool.calls == [] and small.calls == [] and small.uploads == []
    with pytest.raises(ValueError, match="two for the features"):
        HipGroupedEventsStream(device_pool=small)._check_pool(small)
    for bogus in ("bogus", "max_len"):   # (no padded width here)
        with pytest.raises(TypeError, match="unknown options"):
            HipGroupedEventsStream(**{bogus: 1})
    with pytest.raises(TypeError, match="unknown options"):
        HipBasicFeaturesStream(time_window_ns=1.0)
    with pytest.raises(NotImplementedError):
        HipGroupedEventsStream().compute_chunk(run.chunks(50)[0], _ctx(run), "run")


@pytest.mark.parametrize("workers", (1, 4))
def test_end_is_called_and_the_sessions_come_back_when_a_chunk_raises(workers, monkeypatch):
    run = S.run("ragged")
    pool = D.df_event_pool()
    chunks = run.chunks(50)
    third = int(chunks[2].data["record_id"][0])
    plain = D.DfEventOracleSession.basic_features

    def failing(self, *a, **k):
        # the chunk decides, not the order in which worker threads get here: results are delivered in chunk order, so
        # the first two chunks are pushed whatever the workers do
        if int(self._rec["record_id"][0]) == third:
            raise _lib.WfaError(_lib.WFA_E_HIP, "injected")
        return plain(self, *a, **k)

    monkeypatch.setattr(D.DfEventOracleSession, "basic_features", failing)
    with pytest.raises(_lib.WfaError, match="injected"):
        list(HipGroupedEventsStream(device_pool=pool).run_chunks(chunks, _ctx(run), "run", max_workers=workers))
    assert [c[0] for c in pool.calls if c[0] in ("begin", "push", "end")] == ["begin", "push", "push", "end"]
    assert len(pool._free) == pool._borrowable                        # every session is back in the pool


def test_option_precedence_and_pass_through():
    run = S.run("ragged")
    pool = D.df_event_pool()
    ctx = _ctx(run, {"height_range": (1, 2), "time_window_ns": 7.0, "df_events_stream": {"area_range": (5, 9)}}, pool)
    plugin = HipGroupedEventsStream(height_range=(3, 4))
    cfg = plugin._configure(ctx)
    assert (cfg["height_range"], cfg["area_range"], cfg["time_window_ns"]) == ((3, 4), (5, 9), 7.0)
    inner = plugin._inner(cfg, pool)
    assert inner._configure(ctx)["height_range"] == (3, 4) and inner.cfg["area_range"] == (5, 9)
    assert (inner.chunk_size, inner.break_threshold_ps) == (plugin.chunk_size, plugin.break_threshold_ps)
    assert HipGroupedEventsStream().cfg["time_window_ns"] == 100.0
    assert HipBasicFeaturesStream().cfg == {"height_range": (40, 90), "area_range": (0, None), "channel_config": None}


def test_plugin_contracts_and_profile():
    p, f = HipGroupedEventsStream(), HipBasicFeaturesStream()
    assert p.provides == "df_events_stream" and f.provides == "basic_features_stream"
    assert p.depends_on == f.depends_on == ["records", "wave_pool"]
    assert p.is_stateful is True and p.reset_on_break is False and p.save_when == f.save_when == "never"
    assert f.is_stateful is False and p.output_dtype == DF_EVENT_ROW_DTYPE and f.output_dtype == BASIC_FEATURES_DTYPE
    assert {"height_range", "area_range", "channel_config"} <= set(f.options) < set(p.options)
    assert p.options["time_window_ns"].default == 100.0 and f.options["height_range"].default == (40, 90)
    assert [q.provides for q in plugins.hip_streaming_df_events()] == \
        [q.provides for q in plugins.hip_streaming()] + ["basic_features_stream", "df_events_stream"]
    assert "hip_streaming_df_events" in plugins.__all__


# ---- the frame helpers ---------------------------------------------------------------------------------------------------
def _frames_equal(a: pd.DataFrame, b: pd.DataFrame):
    assert list(a.columns) == list(b.columns) and [str(t) for t in a.dtypes] == [str(t) for t in b.dtypes]
    scalar = [c for c in a.columns if a[c].dtype != object]
    pd.testing.assert_frame_equal(a[scalar].reset_index(drop=True), b[scalar].reset_index(drop=True))
    for c in a.columns:
        if a[c].dtype == object:
            off_a, flat_a = E.ragged_flat(a[c])
            off_b, flat_b = E.ragged_flat(b[c])
            np.testing.assert_array_equal(off_a, off_b, err_msg=c)
            assert flat_a.dtype == flat_b.dtype, c
            np.testing.assert_array_equal(flat_a, flat_b, err_msg=c)


@pytest.mark.parametrize("window_ns", (0.0, 100.0, 5000.0))
def test_frame_helpers_equal_build_events_frame_and_pair_events(window_ns):
    rows, _ = D.fixture_rows(Z, "records_plain")
    order, bounds = D.events_of(rows, window_ns)
    want, _flat = build_events_frame(order, bounds, rows["timestamp"], rows["channel"], rows["area"], rows["height"])
    out = D.static_rows(rows, window_ns)
    got = grouped_events_frame(out)
    assert list(got.columns) == MULTI_CHANNEL_COLUMNS
    _frames_equal(got, want)
    for args in ({}, {"time_window_ns": 60.0, "n_channels": 3, "start_channel_slice": 2}, {"time_window_ns": -1.0}):
        _frames_equal(paired_events_frame(out, **args), pair_events(want, args.get("time_window_ns", 100.0),
                      n_channels=args.get("n_channels", 2), start_channel_slice=args.get("start_channel_slice", 6)))
    # pairing commutes with chunking: the frames of two halves, cut at an event border, add up
    cut = int(np.flatnonzero(np.diff(out["event_id"]))[len(got) // 2]) + 1
    halves = pd.concat([paired_events_frame(out[:cut]), paired_events_frame(out[cut:])])
    assert len(halves) == len(paired_events_frame(out))
    np.testing.assert_array_equal(halves["event_id"].to_numpy(), paired_events_frame(out)["event_id"].to_numpy())
    assert list(grouped_events_frame(out[:0]).columns) == MULTI_CHANNEL_COLUMNS


# ---- the C boundary ----------------------------------------------------------------------------------------------------
def test_declared_symbols_and_abi_version():
    header = open(os.path.join(REPO, "include", "wfa_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES, name
    assert int(re.search(r"#define WFA_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 11
    assert _lib.load().wfa_abi_version() == _lib.ABI_VERSION


def test_entry_points_refuse_a_null_context():
    lib = _lib.load()
    n = C.c_int64(0)
    rows = np.zeros(1, dtype=DF_ROW_DTYPE)
    assert lib.wfa_df_event_stream_begin(None, 100.0) == _lib.WFA_E_INVALID
    assert "ctx is null" in _lib.last_error()
    assert lib.wfa_df_event_stream_push(None, rows.ctypes.data_as(C.c_void_p), 1, 0, 0, C.byref(n), C.byref(n),
                                        C.byref(n)) == _lib.WFA_E_INVALID
    assert lib.wfa_df_event_stream_fill(None, None, 0) == _lib.WFA_E_INVALID
    assert lib.wfa_df_event_stream_end(None) == _lib.WFA_E_INVALID
