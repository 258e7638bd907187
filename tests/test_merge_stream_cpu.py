"""The merge stream without a GPU: the closed-cluster rule (numpy restatement, tests/merge_stream_util.py) through
`static_tables` against the tables the reference recorded, HipHitMergedStream's call sequence, option precedence and
refusals on a device double, the profile and the declared C symbols."""

import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import merge_stream_util as M
from tests import stream_hits_util as S
from waveformanalysis_amd import _lib, plugins
from waveformanalysis_amd.dtypes import HIT_MERGED_DTYPE
from waveformanalysis_amd.event_stream import chunk_horizons
from waveformanalysis_amd.merge_stream import HipHitMergedStream, merged_bounds, static_tables
from waveformanalysis_amd.plugin_api import SimpleContext

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("wfa_merge_stream_begin", "wfa_merge_stream_push", "wfa_merge_stream_fill", "wfa_merge_stream_end")


def _ctx(run, config=None, pool=None):
    ctx = SimpleContext({"wave_source": "records", **(config or {})}, {"wave_pool": run.pool, "records": run.records})
    if pool is not None:
        ctx.wfa_device_pool = pool
    return ctx


def _static_oracle(hits, gap, width):
    """The static tables of the oracle's literal chain over the whole table."""
    from oracle import wfa_oracle as O
    from waveformanalysis_amd.hit_merge import compute_component_rows

    clusters = O.hit_merge_clusters(hits, gap, width)
    merged = O.hit_merged_rows(hits, clusters).astype(HIT_MERGED_DTYPE)
    rows = O.hit_merge_cluster_rows(clusters)
    return merged, rows, compute_component_rows(merged, rows)


# ---- the rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_size", M.CPU_CHUNK_SIZES)
@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("name", M.FIXTURES)
def test_rule_and_static_tables_give_the_recorded_tables(name, k, chunk_size):
    case = M.fixture(name)
    hits, configs = case["hits"], case["configs"]
    assert len(configs) == 4
    stream = M.NumpyMergeStream(**configs[k])
    merged, hit_index = M.stream_all(stream.push, hits, M.chunk_size_of(chunk_size, len(hits)))
    got = static_tables(merged, hit_index)
    for table, tag in zip(got, ("merged", "clusters", "components")):
        want = case[f"{tag}_{k}"]
        assert table.dtype == want.dtype and table.tobytes() == want.tobytes(), (name, k, chunk_size, tag)
    if chunk_size == 1:
        assert 0 < stream.max_carry < len(hits)      # clusters leave before the end, and some wait


def test_rule_holds_and_releases_clusters_as_stated():
    # one channel, gap 10 ns: [0, 4000] and [9000, 13000] chain; H = 23000 holds the cluster (H - end == gap), 24000 closes it
    hits = M.make_hits([(0, 4000, 0, 0), (9000, 4000, 0, 0)])
    s = M.NumpyMergeStream(10.0, 10000.0)
    merged, idx, carry, open_start = s.push(hits, 23_000.0)
    assert (len(merged), len(idx), carry, open_start) == (0, 0, 2, 0.0)
    merged, idx, carry, open_start = s.push(None, 24_000.0)
    assert (len(merged), idx.tolist(), carry, open_start) == (1, [0, 1], 0, math.inf)
    assert merged["component_count"].tolist() == [2] and merged["height"].tolist() == [1.0]
    # a row with abs_start == H is not final: the cluster before it stays although the chain broke there
    s = M.NumpyMergeStream(1.0, 10000.0)
    far = M.make_hits([(0, 4000, 0, 0), (50_000, 4000, 0, 0)])
    merged, idx, carry, open_start = s.push(far, 50_000.0)
    assert (len(merged), carry, open_start) == (1, 1, 50_000.0)      # (H - 4000 > gap closes the first by rule 3)
    far = M.make_hits([(0, 4000, 0, 0, 2), (50_000, 4000, 0, 0, 4)])   # (another dt: the chain breaks whatever the gap)
    s = M.NumpyMergeStream(100.0, 10000.0)
    merged, idx, carry, open_start = s.push(far, 50_000.0)           # gap 100 ns: rule 3 fails, rule 1 needs b < F
    assert (len(merged), carry, open_start) == (0, 2, 0.0)
    merged, idx, carry, open_start = s.push(None, 50_001.0)          # the breaking hit is final now: rule 1
    assert (idx.tolist(), carry, open_start) == ([0], 1, 50_000.0)


def test_static_tables_reorders_and_checks():
    hits = M.make_hits([(0, 4000, 0, 1), (1000, 4000, 0, 0), (900_000, 4000, 0, 1), (901_000, 4000, 0, 1)])
    s = M.NumpyMergeStream(20.0, 10000.0)
    merged, hit_index = M.stream_all(s.push, hits, 2)
    assert merged["channel"].tolist() == [0, 1, 1] and hit_index.tolist() == [1, 0, 2, 3]
    got = static_tables(merged, hit_index)
    for table, want in zip(got, _static_oracle(hits, 20.0, 10000.0)):
        assert table.tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="component rows"):
        static_tables(merged, hit_index[:-1])
    empty = static_tables(merged[:0], hit_index[:0])
    assert [len(t) for t in empty] == [0, 0, 0] and empty[0].dtype == HIT_MERGED_DTYPE


# ---- the plugin on a device double ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("workers", (1, 4))
@pytest.mark.parametrize("gap", (0.0, 400.0))
@pytest.mark.parametrize("name,chunk_size", (("ragged", 50), ("mixed", 100), ("shuffled", 7)))
def test_plugin_tables_equal_the_static_rule(name, chunk_size, gap, workers):
    run = S.run(name)
    pool = M.merge_pool()
    plugin = HipHitMergedStream(device_pool=pool, merge_gap_ns=gap)
    plugin.chunk_size = chunk_size
    outs = list(plugin.run_chunks(run.chunks(chunk_size), _ctx(run), "run", max_workers=workers))
    hits = run.want(False)
    merged = np.concatenate([o.data for o in outs])
    hit_index = np.concatenate([o.metadata["hit_index"] for o in outs])
    for table, want in zip(static_tables(merged, hit_index), _static_oracle(hits, gap, 10000.0)):
        assert table.dtype == want.dtype and table.tobytes() == want.tobytes()
    first = 0
    for o in outs:
        assert len(o.data) and o.data.dtype == HIT_MERGED_DTYPE and (o.start, o.end) == merged_bounds(o.data)
        assert o.data_type == "hit_merged_stream" and o.time_field == "timestamp"
        assert o.metadata["first_component"] == first == int(o.data["component_offset"][0])
        assert len(o.metadata["hit_index"]) == int(o.data["component_count"].sum())
        assert o.metadata["n_carry"] >= 0 and o.metadata["open_start"] > 0
        first += len(o.metadata["hit_index"])
    assert plugin.stats["rows_in"] == plugin.stats["components"] == len(hits) and plugin.stats["rows_out"] == len(merged)
    assert (len(merged) < len(hits)) == (gap > 0)


def test_call_sequence_with_hitless_and_empty_chunks():
    run = S.run("sparse")
    chunks, k_empty = S.sparse_chunks_with_empty()
    pool = M.merge_pool()
    plugin = HipHitMergedStream(device_pool=pool, merge_gap_ns=20.0, max_total_width_ns=500.0)
    list(plugin.run_chunks(chunks, _ctx(run), "run", max_workers=4))
    calls = pool.calls
    assert calls[0][:3] == ("begin", 20.0, 500.0) and calls[-1][0] == "end"
    pushes = calls[1:-1]
    assert [c[0] for c in pushes] == ["push"] * (len(chunks) + 1)
    assert len({id(c[-1]) for c in calls}) == 1                       # one session for the whole run
    want = run.want(False)
    per_chunk = [int(np.isin(want["record_id"], c.data["record_id"]).sum()) for c in chunks]
    assert [c[1] for c in pushes] == per_chunk + [0]                  # one push per chunk, in order, then the flush
    assert per_chunk[k_empty] == 0 and 0 in [n for k, n in enumerate(per_chunk) if k != k_empty]   # hitless chunks too
    assert [c[2] for c in pushes[:-1]] == chunk_horizons(chunks) and pushes[-1][2] == math.inf
    assert calls[0][-1] not in [e["session"] for e in pool.log]       # the ring's sessions are others
    assert plugin.stats["pushes"] == len(chunks) + 1


@pytest.mark.parametrize("workers", (1, 4))
def test_end_is_called_when_a_chunk_raises(workers, monkeypatch):
    run = S.run("ragged")
    pool = M.merge_pool()
    seen = []

    def failing_wait(self):
        seen.append(1)
        if len(seen) == 3:
            raise _lib.WfaError(_lib.WFA_E_HIP, "injected")
        return len(self._rows)

    monkeypatch.setattr(M.MergeOracleSession, "hits_wait", failing_wait)
    plugin = HipHitMergedStream(device_pool=pool)
    with pytest.raises(_lib.WfaError, match="injected"):
        list(plugin.run_chunks(run.chunks(50), _ctx(run), "run", max_workers=workers))
    assert [c[0] for c in pool.calls] == ["begin", "push", "push", "end"]
    assert len(pool._free) == pool._borrowable                        # every session is back in the pool


def test_option_precedence_and_pass_through():
    run = S.run("ragged")
    pool = M.merge_pool()
    ctx = _ctx(run, {"threshold": 250.0, "merge_gap_ns": 7.0, "max_total_width_ns": 900.0,
                     "hit_merged_stream": {"right_extension": 1}}, pool)
    plugin = HipHitMergedStream(threshold=S.THRESHOLD, left_extension=S.LE, max_total_width_ns=50.0)
    cfg = plugin._configure(ctx)
    assert (cfg["threshold"], cfg["left_extension"], cfg["right_extension"]) == (S.THRESHOLD, S.LE, 1)
    assert (cfg["merge_gap_ns"], cfg["max_total_width_ns"]) == (7.0, 50.0)         # Context > default, constructor > Context
    inner = plugin._inner(cfg, pool)
    inner._configure(ctx)       # the Context cannot win over what the outer stream resolved
    assert (inner.threshold, inner.le, inner.re) == (S.THRESHOLD, S.LE, 1)
    assert HipHitMergedStream(merge_gap_ns=3.0)._configure(ctx)["merge_gap_ns"] == 3.0
    default = HipHitMergedStream().cfg
    assert (default["merge_gap_ns"], default["max_total_width_ns"], default["dt"]) == (0.0, 10000.0, None)
    list(HipHitMergedStream().compute(ctx, "run", streaming_config={"chunk_size": 200}))
    assert pool.calls[0][:3] == ("begin", 7.0, 900.0)                               # the Context's values reach the device


def test_refusals_before_any_upload():
    run = S.run("ragged")
    small = M.merge_pool(max_sessions=2)
    with pytest.raises(ValueError, match="max_sessions >= 3"):
        list(HipHitMergedStream(device_pool=small).compute(_ctx(run), "run"))
    assert small.uploads == [] and small.calls == []
    for bad in ({"merge_gap_ns": -1.0}, {"max_total_width_ns": -5.0}, {"merge_gap_ns": math.nan}):
        name = next(iter(bad))
        with pytest.raises(ValueError, match=f"{name} must be >= 0"):
            HipHitMergedStream(**bad)
        pool = M.merge_pool()
        with pytest.raises(ValueError, match=f"{name} must be >= 0"):
            list(HipHitMergedStream(device_pool=pool).compute(_ctx(run, bad), "run"))
        assert pool.uploads == [] and pool.calls == []
    with pytest.raises(TypeError, match="unknown options"):
        HipHitMergedStream(bogus=1)
    with pytest.raises(NotImplementedError):
        HipHitMergedStream().compute_chunk(run.chunks(50)[0], _ctx(run), "run")
    three = M.merge_pool(max_sessions=3)                              # three sessions suffice
    outs = list(HipHitMergedStream(device_pool=three).run_chunks(run.chunks(150), _ctx(run), "run", max_workers=4))
    assert sum(len(o.data) for o in outs) == len(run.want(False))


def test_plugin_contract_and_profiles():
    p = HipHitMergedStream()
    assert p.provides == "hit_merged_stream" and p.depends_on == ["records", "wave_pool"]
    assert p.is_stateful is True and p.reset_on_break is False and p.save_when == "never"
    assert p.output_dtype == HIT_MERGED_DTYPE and HIT_MERGED_DTYPE.itemsize == 72
    assert [HIT_MERGED_DTYPE.fields[n][1] for n in ("sample_start", "timestamp", "component_offset", "component_count")] == \
        [16, 40, 60, 68]
    assert {"merge_gap_ns", "max_total_width_ns", "dt", "threshold", "channel_config", "filter_source"} <= set(p.options)
    events = [q.provides for q in plugins.hip_streaming_events()]
    assert events == ["hit_threshold_stream", "signal_peaks_stream", "s1_s2_stream", "hit_grouped_stream"]   # unchanged
    assert [q.provides for q in plugins.hip_streaming_merged()] == events + ["hit_merged_stream"]
    assert "hip_streaming_merged" in plugins.__all__


# ---- the C boundary ----------------------------------------------------------------------------------------------------
def test_declared_symbols_and_abi_version():
    header = open(os.path.join(REPO, "include", "wfa_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, header, flags=re.M) and name in _lib.SIGNATURES, name
    assert int(re.search(r"#define WFA_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 8
    assert _lib.load().wfa_abi_version() == _lib.ABI_VERSION


def test_entry_points_refuse_a_null_context():
    lib = _lib.load()
    n, f = C.c_int64(0), C.c_double(0.0)
    rows = np.zeros(1, dtype=M.THRESHOLD_HIT_DTYPE)
    assert lib.wfa_merge_stream_begin(None, 20.0, 100.0) == _lib.WFA_E_INVALID
    assert "ctx is null" in _lib.last_error()
    assert lib.wfa_merge_stream_push(None, rows.ctypes.data_as(C.c_void_p), 1, 0.0, C.byref(n), C.byref(n), C.byref(n),
                                     C.byref(f)) == _lib.WFA_E_INVALID
    assert lib.wfa_merge_stream_fill(None, None, None, 0, 0) == _lib.WFA_E_INVALID
    assert lib.wfa_merge_stream_end(None) == _lib.WFA_E_INVALID
