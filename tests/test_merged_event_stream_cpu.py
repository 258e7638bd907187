"""The merged-event stream without a GPU: the two-step rule (numpy restatement, tests/merged_event_stream_util.py) against
the events of merged hits the reference recorded, HipHitMergedGroupedStream's frames, call sequence, option precedence and
refusals on a device double, the lowering of open_start, merged_events_frame, the profile and the declared C symbols."""

import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from tests import merged_event_stream_util as U
from tests import stream_hits_util as S
from waveformanalysis_amd import _lib, plugins
from waveformanalysis_amd.dtypes import EVENT_MERGED_HIT_DTYPE, HIT_MERGED_DTYPE
from waveformanalysis_amd.event_grouping import EVENT_COLUMNS
from waveformanalysis_amd.event_stream import chunk_horizons, horizon_margin, run_margin
from waveformanalysis_amd.merged_event_stream import (
    HipHitMergedGroupedStream,
    group_horizon,
    lowered_open_start,
    merged_events_frame,
    open_start_margin,
)
from waveformanalysis_amd.plugin_api import SimpleContext

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("wfa_merged_event_stream_begin", "wfa_merged_event_stream_push", "wfa_merged_event_stream_fill",
                "wfa_merged_event_stream_end")
WIDTH = 10000.0


def _ctx(run, config=None, pool=None):
    ctx = SimpleContext({"wave_source": "records", **(config or {})}, {"wave_pool": run.pool, "records": run.records})
    if pool is not None:
        ctx.wfa_device_pool = pool
    return ctx


@functools.cache
def _static_oracle(name, use_filtered, gap, width, window):
    """The static chain of the oracle over a fixture run: hit_merged, its components, and hit_grouped of them as rows."""
    from oracle import wfa_oracle as O
    from waveformanalysis_amd.hit_merge import compute_component_rows

    hits = S.run(name).want(use_filtered)
    clusters = O.hit_merge_clusters(hits, gap, width)
    merged = O.hit_merged_rows(hits, clusters).astype(HIT_MERGED_DTYPE)
    components = compute_component_rows(merged, O.hit_merge_cluster_rows(clusters))
    rows = U.static_rows(merged, components, hits, window)
    rows.setflags(write=False)
    return hits, merged, components, rows


_assert_frames_equal, _assert_components = U.assert_frames_equal, U.assert_components


# ---- the rule against the reference's recorded tables -------------------------------------------------------------------
@pytest.mark.parametrize("chunk_size", U.CPU_CHUNK_SIZES)
@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("name", U.FIXTURES)
def test_rule_gives_the_recorded_events_of_merged_hits(name, k, chunk_size):
    case = U.fixture(name)
    hits, cfg = case["hits"], case["configs"][k]
    size = U.chunk_size_of(chunk_size, len(hits))
    margin = U.fixture_margin(hits)
    horizons = U.fixture_horizons(hits, size, margin)
    assert len(case["windows"]) == 3
    for tw in case["windows"]:
        tag = f"g{k}_w{int(tw)}"
        stream = U.NumpyMergedEventStream(time_window_ns=float(tw), horizon_margin_ps=margin, **cfg)
        rows, hit_index = U.stream_all(stream.push, hits, size, horizons)
        U.assert_recorded(rows, case, tag)
        assert sorted(hit_index.tolist()) == list(range(len(hits)))
        # ... and the static grouping of the recorded merged table gives the same rows but for component_offset
        want = U.static_rows(case[f"merged_{k}"], case[f"components_{k}"], hits, float(tw))
        for field in EVENT_MERGED_HIT_DTYPE.names:
            if field != "component_offset":
                assert np.array_equal(rows[field], want[field]), (tag, field)
        if chunk_size == 1 and tw == 100.0:
            assert 0 < stream.max_carry < len(hits)               # events leave before the end, and some wait
    if k >= 2:
        assert (case[f"merged_{k}"]["sample_start"] < 0).any()    # clusters that span records: windows from the members


def test_rule_holds_an_event_back_while_a_cluster_is_open():
    # gap 100 ns, H = 1 us: channel 0's cluster [1000, 951000] ends within the gap of H and stays open; channel 1's single
    # hit [2000, 6000] closes at once, but G = open_start = 1000 holds its event: the open cluster will become a row that
    # starts at 1000 and joins it
    hits = U.make_hits([(1000, 950_000, 0, 0), (2000, 4000, 0, 1)])
    s = U.NumpyMergedEventStream(100.0, 1e6, 1.0)
    out, idx, n_hits, n_rows, g = s.push(hits, 1_000_000.0)
    assert (len(out), idx.tolist(), n_hits, n_rows, g) == (0, [1], 1, 1, 1000.0)
    out, idx, n_hits, n_rows, g = s.push(None, 2_000_000.0)
    assert (out["event_id"].tolist(), out["channel"].tolist(), idx.tolist(), n_hits, n_rows, g) == ([0, 0], [0, 1], [0], 0, 0, 2_000_000.0)
    assert out["component_offset"].tolist() == [1, 0] and out["t_min"].tolist() == [1000, 1000]
    # the strict boundary: max(abs_end) + window == G holds the event, one ps more releases it
    s = U.NumpyMergedEventStream(0.0, WIDTH, 1.0)
    one = U.make_hits([(1000, 4000, 0, 0)])
    assert len(s.push(one, 6000.0)[0]) == 0 and len(s.push(None, 6001.0)[0]) == 1


@pytest.mark.parametrize("same_channel", (False, True))
def test_rule_at_2_to_60_gives_the_static_events(same_channel):
    from oracle import wfa_oracle as O
    from waveformanalysis_amd.hit_merge import compute_component_rows

    pushes, margin = U.late_pushes(same_channel)
    hits = np.concatenate([rows for rows, _h in pushes])
    assert margin == 512.0
    for gap in (30.0, 900.0):
        stream = U.NumpyMergedEventStream(gap, 1e9, 100.0, margin)
        parts = [stream.push(rows, h) for rows, h in pushes] + [stream.push(None, math.inf)]     # (asserts the row bound)
        rows = np.concatenate([p[0] for p in parts])
        clusters = O.hit_merge_clusters(hits, gap, 1e9)
        merged = O.hit_merged_rows(hits, clusters).astype(HIT_MERGED_DTYPE)
        components = compute_component_rows(merged, O.hit_merge_cluster_rows(clusters))
        want = U.static_rows(merged, components, hits, 100.0)
        for field in EVENT_MERGED_HIT_DTYPE.names:
            assert field == "component_offset" or np.array_equal(rows[field], want[field]), (gap, field)
        assert all(a[4] <= b[4] for a, b in zip(parts[:-1], parts[1:])) and sum(len(p[0]) for p in parts[:-2]) > 0
    # as given every cluster of several hits spans records (member windows); in one channel they lie inside a record (anchor)
    assert (rows["sample_start"] < 0).any() == (not same_channel)
    assert (rows["component_count"][rows["sample_start"] >= 0] > 1).any() == same_channel


# ---- the lowering of open_start --------------------------------------------------------------------------------------------
def test_open_start_is_lowered_beyond_2_to_53_only():
    assert open_start_margin(0.0) == 0.0 and open_start_margin(horizon_margin(2**60)) == 768.0     # three ulps of 256 ps
    assert lowered_open_start(12345.0, 0.0) == 12345.0 and lowered_open_start(float(2**53 - 1), horizon_margin(2**53 - 1)) == 2.0**53 - 1
    assert lowered_open_start(math.inf, 512.0) == math.inf
    at = lowered_open_start(float(2**53), horizon_margin(2**53))
    assert at == float(2**53) - 6.0 - 1.0                     # 3 ulps of 2 ps, then one step (1 ps below 2^53)
    x = float(2**60 + 10_240)
    assert lowered_open_start(x, 512.0) == x - 768.0 - 256.0 == U.lowered(x, 512.0)
    assert group_horizon(5000.0, 1000.0) == 1000.0 and group_horizon(5000.0, math.inf) == 5000.0
    assert group_horizon(5000.0, 1000.0, 0.0, previous=2000.0) == 2000.0
    assert group_horizon(x + 4096.0, x, 512.0) == x - 1024.0
    # brute force at 2^60 and just below 2^62, dt = 3 ns: the anchor window of a one-record cluster never starts below the
    # lowered smallest member window, while the unlowered one does
    rng = np.random.default_rng(21)
    for base in (2**60, 2**62 - 10**9):
        n = 4000
        rec_ts = base + rng.integers(0, 10**8, n)
        pos = rng.integers(0, 500, (n, 2))
        start = np.minimum(rng.integers(0, 500, (n, 2)), pos)
        ts = rec_ts[:, None] + pos * 3000
        member = ts.astype(np.float64) + (start.astype(np.float64) - pos.astype(np.float64)) * (3.0 * 1e3)
        smin = start.min(axis=1).astype(np.float64)
        anchors = ts.astype(np.float64) + (smin[:, None] - pos.astype(np.float64)) * (3.0 * 1e3)      # either member as anchor
        margin = horizon_margin(int(base) + 10**8 + 3000 * 500)
        lowest = np.array([lowered_open_start(v, margin) for v in member.min(axis=1)])
        assert (anchors.min(axis=1) >= lowest).all()
        assert (anchors.min(axis=1) < member.min(axis=1)).any()


# ---- the plugin on a device double --------------------------------------------------------------------------------------
@pytest.mark.parametrize("workers", (1, 4), ids=("serial", "ring"))
@pytest.mark.parametrize("chunk_size", (1, 7, 1000))
@pytest.mark.parametrize("name", ("ragged", "mixed", "shuffled"))
def test_plugin_frame_equals_the_static_chain(name, chunk_size, workers):
    run = S.run(name)
    gap, window = 400.0, 100.0
    pool = U.merged_event_pool()
    plugin = HipHitMergedGroupedStream(device_pool=pool, merge_gap_ns=gap, time_window_ns=window)
    plugin.chunk_size = chunk_size
    chunks = run.chunks(chunk_size)
    outs = list(plugin.run_chunks(chunks, _ctx(run), "run", max_workers=workers))
    hits, merged, components, want = _static_oracle(name, False, gap, WIDTH, window)
    rows = np.concatenate([o.data for o in outs])
    assert rows.dtype == EVENT_MERGED_HIT_DTYPE and len(merged) < len(hits)
    _assert_frames_equal(merged_events_frame(rows), merged_events_frame(want))
    _assert_components(outs, rows, merged, components)
    previous = -math.inf
    for o in outs:
        assert len(o.data) and (o.start, o.end) == (int(o.data["t_min"].min()), int(o.data["t_max"].max()) + 1)
        assert o.data_type == "hit_merged_grouped_stream" and o.time_field == "t_min"
        assert o.metadata["first_event"] == int(o.data["event_id"][0]) and o.metadata["group_horizon"] >= previous
        assert o.metadata["n_merge_carry"] >= 0 and o.metadata["n_event_carry"] >= 0
        previous = o.metadata["group_horizon"]
    assert outs[-1].metadata["n_merge_carry"] == outs[-1].metadata["n_event_carry"] == 0
    assert plugin.stats["pushes"] == len(chunks) + 1                            # one push per chunk plus the flush
    assert [c[0] for c in pool.calls] == ["begin"] + ["push"] * (len(chunks) + 1) + ["end"]
    assert plugin.stats["rows_in"] == plugin.stats["components"] == len(hits) and plugin.stats["rows_out"] == len(merged)
    assert plugin.stats["events"] == int(want["event_id"][-1]) + 1
    assert [c[2] for c in pool.calls[1:-2]] == chunk_horizons(chunks) and pool.calls[-2][2] == math.inf
    assert pool.calls[0][4] == run_margin(chunks) == 0.0                        # the run's margin reaches _begin


def test_the_margin_of_a_late_run_reaches_begin():
    from types import SimpleNamespace

    rec = S.run("ragged").records.copy()
    rec["timestamp"] += 2**60
    chunks = [SimpleNamespace(data=rec[lo : lo + 100]) for lo in range(0, len(rec), 100)]
    assert run_margin(chunks) == 512.0 and chunk_horizons(chunks) == chunk_horizons(chunks, 512.0)
    plugin = HipHitMergedGroupedStream()
    plugin._run_margin(run_margin(chunks))
    calls = []
    plugin._begin(U.MergedEventOracleSession(calls=calls), plugin.cfg)
    assert calls[0][:5] == ("begin", 0.0, WIDTH, 100.0, 512.0)


@pytest.mark.parametrize("workers", (1, 4))
def test_end_is_called_when_a_chunk_raises(workers, monkeypatch):
    run = S.run("ragged")
    pool = U.merged_event_pool()
    seen = []

    def failing_wait(self):
        seen.append(1)
        if len(seen) == 3:
            raise _lib.WfaError(_lib.WFA_E_HIP, "injected")
        return len(self._rows)

    monkeypatch.setattr(U.MergedEventOracleSession, "hits_wait", failing_wait)
    plugin = HipHitMergedGroupedStream(device_pool=pool)
    with pytest.raises(_lib.WfaError, match="injected"):
        list(plugin.run_chunks(run.chunks(50), _ctx(run), "run", max_workers=workers))
    assert [c[0] for c in pool.calls] == ["begin", "push", "push", "end"]
    assert len(pool._free) == pool._borrowable                        # every session is back in the pool


def test_option_precedence_and_pass_through():
    run = S.run("ragged")
    pool = U.merged_event_pool()
    ctx = _ctx(run, {"threshold": 250.0, "merge_gap_ns": 7.0, "max_total_width_ns": 900.0, "time_window_ns": 33.0,
                     "hit_merged_grouped_stream": {"right_extension": 1}}, pool)
    plugin = HipHitMergedGroupedStream(threshold=S.THRESHOLD, left_extension=S.LE, max_total_width_ns=50.0)
    cfg = plugin._configure(ctx)
    assert (cfg["threshold"], cfg["left_extension"], cfg["right_extension"]) == (S.THRESHOLD, S.LE, 1)
    assert (cfg["merge_gap_ns"], cfg["max_total_width_ns"], cfg["time_window_ns"]) == (7.0, 50.0, 33.0)
    inner = plugin._inner(cfg, pool)
    inner._configure(ctx)       # the Context cannot win over what the outer stream resolved
    assert (inner.threshold, inner.le, inner.re) == (S.THRESHOLD, S.LE, 1)
    assert HipHitMergedGroupedStream(time_window_ns=3.0)._configure(ctx)["time_window_ns"] == 3.0
    default = HipHitMergedGroupedStream().cfg
    assert (default["merge_gap_ns"], default["max_total_width_ns"], default["time_window_ns"], default["dt"]) == \
        (0.0, WIDTH, 100.0, None)                                                   # the static plugins' defaults
    list(HipHitMergedGroupedStream().compute(ctx, "run", streaming_config={"chunk_size": 200}))
    assert pool.calls[0][:5] == ("begin", 7.0, 900.0, 33.0, 0.0)                    # the Context's values reach the device


def test_refusals_before_any_upload():
    run = S.run("ragged")
    small = U.merged_event_pool(max_sessions=2)
    with pytest.raises(ValueError, match="max_sessions >= 3"):
        list(HipHitMergedGroupedStream(device_pool=small).compute(_ctx(run), "run"))
    assert small.uploads == [] and small.calls == []
    for bad in ({"merge_gap_ns": -1.0}, {"max_total_width_ns": -5.0}, {"time_window_ns": -0.5}, {"merge_gap_ns": math.nan}):
        name = next(iter(bad))
        with pytest.raises(ValueError, match=f"{name} must be >= 0"):
            HipHitMergedGroupedStream(**bad)
        pool = U.merged_event_pool()
        with pytest.raises(ValueError, match=f"{name} must be >= 0"):
            list(HipHitMergedGroupedStream(device_pool=pool).compute(_ctx(run, bad), "run"))
        assert pool.uploads == [] and pool.calls == []
    with pytest.raises(TypeError, match="unknown options"):
        HipHitMergedGroupedStream(bogus=1)
    with pytest.raises(NotImplementedError):
        HipHitMergedGroupedStream().compute_chunk(run.chunks(50)[0], _ctx(run), "run")


def test_a_pool_of_three_sessions_suffices():
    run = S.run("ragged")
    pool = U.merged_event_pool(max_sessions=3)
    plugin = HipHitMergedGroupedStream(device_pool=pool, merge_gap_ns=20.0)
    outs = list(plugin.run_chunks(run.chunks(50), _ctx(run), "run", max_workers=4))
    want = _static_oracle("ragged", False, 20.0, WIDTH, 100.0)[3]
    _assert_frames_equal(merged_events_frame(np.concatenate([o.data for o in outs])), merged_events_frame(want))
    assert pool._borrowable == 3
    assert len({id(c[-1]) for c in pool.calls}) == 1 and pool.calls[0][-1] not in [e["session"] for e in pool.log]


def test_run_without_hits_gives_no_chunks():
    rec = S.run("sparse").records[:120].copy()
    wave_pool = np.full(int((rec["wave_offset"] + rec["event_length"]).max()), S.BASELINE, dtype=np.uint16)
    ctx = SimpleContext({"wave_source": "records", "merge_gap_ns": 20.0}, {"records": rec, "wave_pool": wave_pool})
    ctx.wfa_device_pool = pool = U.merged_event_pool()
    plugin = HipHitMergedGroupedStream()
    assert list(plugin.compute(ctx, "run", streaming_config={"chunk_size": 50})) == []
    assert plugin.stats["pushes"] == 4 and plugin.stats["rows_in"] == 0 and [c[1] for c in pool.calls[1:-1]] == [0] * 4


def test_existing_streams_do_not_see_the_margin_hook():
    from tests import event_stream_util as E
    from tests import merge_stream_util as M
    from waveformanalysis_amd.event_stream import HipHitGroupedStream
    from waveformanalysis_amd.merge_stream import HipHitMergedStream

    run = S.run("ragged")
    pool = E.event_pool()
    list(HipHitGroupedStream(device_pool=pool).run_chunks(run.chunks(150), _ctx(run), "run"))
    assert pool.calls[0][:2] == ("begin", 100.0) and len(pool.calls[0]) == 3
    pool = M.merge_pool()
    list(HipHitMergedStream(device_pool=pool).run_chunks(run.chunks(150), _ctx(run), "run"))
    assert pool.calls[0][:3] == ("begin", 0.0, WIDTH) and len(pool.calls[0]) == 4
    with pytest.raises(ValueError, match="merge_gap_ns"):               # and hit_grouped_stream keeps its refusal
        list(HipHitGroupedStream(device_pool=E.event_pool()).compute(_ctx(run, {"merge_gap_ns": 20.0}), "run"))


# ---- host-side functions ---------------------------------------------------------------------------------------------------
def test_merged_events_frame():
    hits = U.make_hits([(0, 4000, 0, 0), (6000, 4000, 0, 0), (8000, 2000, 0, 1), (900_000, 4000, 0, 1)])
    s = U.NumpyMergedEventStream(20.0, WIDTH, 100.0)
    rows, _idx = U.stream_all(s.push, hits, 2)
    frame = merged_events_frame(rows)
    assert list(frame.columns) == EVENT_COLUMNS and frame["event_id"].tolist() == [0, 1]
    assert frame["n_hits"].tolist() == [2, 1] and frame["t_min"].tolist() == [0, 900_000]
    first = frame.iloc[0]
    assert first["channels"].tolist() == [0, 1] and first["sample_starts"].tolist() == [-1, 10]     # the cluster spans records
    assert first["sample_ends"].tolist() == [-1, 11] and first["sample_starts"].dtype == np.int32
    assert first["t_max"] == 10_000 and first["dt/ns"] == 10.0
    empty = merged_events_frame(rows[:0])
    assert list(empty.columns) == EVENT_COLUMNS and len(empty) == 0


def test_plugin_contract_and_profiles():
    p = HipHitMergedGroupedStream()
    assert p.provides == "hit_merged_grouped_stream" and p.depends_on == ["records", "wave_pool"]
    assert p.is_stateful is True and p.reset_on_break is False and p.save_when == "never"
    assert p.output_dtype == EVENT_MERGED_HIT_DTYPE and EVENT_MERGED_HIT_DTYPE.itemsize == 96
    assert [EVENT_MERGED_HIT_DTYPE.fields[n][1] for n in ("event_id", "t_min", "t_max", "position", "sample_start",
                                                          "component_offset", "component_count")] == [0, 8, 16, 24, 40, 84, 92]
    assert EVENT_MERGED_HIT_DTYPE.names[3:] == HIT_MERGED_DTYPE.names
    assert {"merge_gap_ns", "max_total_width_ns", "time_window_ns", "dt", "threshold", "channel_config"} <= set(p.options)
    merged = [q.provides for q in plugins.hip_streaming_merged()]
    assert merged == ["hit_threshold_stream", "signal_peaks_stream", "s1_s2_stream", "hit_grouped_stream", "hit_merged_stream"]
    assert [q.provides for q in plugins.hip_streaming_merged_events()] == merged + ["hit_merged_grouped_stream"]
    assert "hip_streaming_merged_events" in plugins.__all__


# ---- the C boundary ----------------------------------------------------------------------------------------------------
def test_declared_symbols_and_abi_version():
    header = open(os.path.join(REPO, "include", "wfa_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES, name
    assert int(re.search(r"#define WFA_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 9
    assert _lib.load().wfa_abi_version() == _lib.ABI_VERSION


def test_entry_points_refuse_a_null_context():
    lib = _lib.load()
    n, f = C.c_int64(0), C.c_double(0.0)
    rows = np.zeros(1, dtype=U.THRESHOLD_HIT_DTYPE)
    assert lib.wfa_merged_event_stream_begin(None, 20.0, 100.0, 100.0, 0.0) == _lib.WFA_E_INVALID
    assert "ctx is null" in _lib.last_error()
    assert lib.wfa_merged_event_stream_push(None, rows.ctypes.data_as(C.c_void_p), 1, 0.0, *([C.byref(n)] * 6),
                                            C.byref(f)) == _lib.WFA_E_INVALID
    assert lib.wfa_merged_event_stream_fill(None, None, None, 0, 0) == _lib.WFA_E_INVALID
    assert lib.wfa_merged_event_stream_end(None) == _lib.WFA_E_INVALID
