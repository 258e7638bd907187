"""The inputs of tests/test_hip_stream_hits.py hold what that file is about (no vacuous pass), and the host logic of
HipThresholdHitStream -- the padded width that reaches every chunk's pass, option precedence, the staged slice of the
pool, the ring, empty chunks -- on a device double that answers with the oracle's rows (stream_hits_util.OracleSession).
No GPU."""

import numpy as np
import pytest

from tests import stream_hits_util as S
from waveformanalysis_amd import _lib
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.streaming import HipThresholdHitStream

BOTH = (False, True)


def _ctx(run, config=None, records=True):
    data = {"wave_pool": run.pool}
    if records:
        data["records"] = run.records
    return SimpleContext({"wave_source": "records", **(config or {})}, data)


# ---- conditions on the inputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_filtered", BOTH)
def test_ragged_chunks_narrower_than_the_run_change_rows(use_filtered):
    run = S.run("ragged")
    want = run.want(use_filtered)
    counts = {}
    for c in (50, 100, 150):
        diff = S.differing_rows(run.per_chunk_oracle(c, use_filtered), want)
        counts[c] = len(set(np.concatenate(list(diff.values())).tolist())) if diff else 0
        if c == 50:
            assert len(diff.get("position", ())) >= 1
            assert set(diff) <= {"position", "height", "integral", "rise_time", "fall_time", "timestamp"}
    assert counts[50] >= 5 and counts[100] >= 1 and counts[150] == 0, counts


@pytest.mark.parametrize("use_filtered", BOTH)
def test_mixed_windows_reach_the_padding(use_filtered):
    run = S.run("mixed")
    want = run.want(use_filtered)
    assert run.width == 88
    short = run.row_lengths(want) < 88
    assert int((run.in_padding(want) & short).sum()) >= 10
    lengths = [np.unique(seg["event_length"]) for seg in run.segments()]
    assert [len(seg) for seg in run.segments()] == [n for _name, n in S.MIXED_SEGMENTS]
    assert lengths[0].tolist() == [64] and lengths[1].tolist() == [88] and lengths[3].tolist() == [24]
    assert lengths[2].min() >= 40 and lengths[2].max() == 64 and len(lengths[2]) > 10
    # consecutive chunks of one session of a ring of 2 or 3 differ in record count or in layout
    chunks = run.chunks(100)
    shape = [(len(c.data), c.metadata["segment_id"]) for c in chunks]
    assert [n for n, _s in shape] == [100, 50, 100, 30, 100, 70, 100, 20]
    for ring in (2, 3):
        for a, b in zip(shape, shape[ring:]):
            assert a != b, (ring, shape)
    assert {s for _n, s in shape} == {0, 1, 2, 3}


@pytest.mark.parametrize("use_filtered", BOTH)
@pytest.mark.parametrize("name", S.RUN_NAMES)
def test_every_run_has_rows_at_both_record_ends(name, use_filtered):
    run = S.run(name)
    want = run.want(use_filtered)
    assert len(run.records) < 1500 and run.pool.size < 150_000
    assert len(want) > 150
    assert int((want["edge_start"] == 0).sum()) >= 20
    assert int((want["edge_end"] == run.row_lengths(want)).sum()) >= 20
    assert np.all(np.diff(run.records["timestamp"]) > 0)     # time-sorted


def test_ragged_layout():
    run = S.run("ragged")
    rec = run.records
    assert run.pool.size % 8 != 0
    assert set((rec["wave_offset"] % 8).tolist()) == set(range(8))
    for L in (0, 1, 7):
        assert int((rec["event_length"] == L).sum()) >= 3
    assert np.flatnonzero(rec["event_length"] == 200).tolist() == [0, 150, 300, 450]
    for c in run.chunk_sizes:
        assert all(int(ch.data["event_length"].max()) > 0 for ch in run.chunks(c))


def test_shuffled_slices_hold_other_chunks_samples():
    run, base = S.run("shuffled"), S.run("ragged")
    rec = run.records
    assert np.any(np.diff(rec["wave_offset"]) < 0)
    for r in (0, 1, 77, 599):   # the same samples as the ragged run's records
        o, b, L = int(rec["wave_offset"][r]), int(base.records["wave_offset"][r]), int(rec["event_length"][r])
        np.testing.assert_array_equal(run.pool[o : o + L], base.pool[b : b + L])
        assert np.all(run.pool[o - 5 : o] == S.GARBAGE)
    for f in BOTH:
        assert run.want(f).tobytes() == base.want(f).tobytes()
    wide = 0
    for ch in run.chunks(50):
        lo = int(ch.data["wave_offset"].min())
        hi = int((ch.data["wave_offset"] + ch.data["event_length"]).max())
        wide += hi - lo >= 2 * int(ch.data["event_length"].sum())
    assert wide >= 1


def test_sparse_blocks():
    run = S.run("sparse")
    want = run.want(False)
    chunks = run.chunks(S.SPARSE_BLOCK)
    per_chunk = [int(np.isin(want["record_id"], c.data["record_id"]).sum()) for c in chunks]
    assert [n > 0 for n in per_chunk] == list(S.SPARSE_PATTERN)
    assert all(n == 2 * S.SPARSE_BLOCK for n in per_chunk if n)
    with_empty, k = S.sparse_chunks_with_empty()
    assert len(with_empty) == len(chunks) + 1 and len(with_empty[k].data) == 0 and 0 < k < len(chunks)


# ---- the padded width ---------------------------------------------------------------------------------------------
def _drive(plugin, run, ctx, driver, c):
    """-> (input chunks, results) of one driver."""
    chunks = run.chunks(c)
    if driver == "compute_serial":
        return chunks, list(plugin.compute(ctx, "run", streaming_config={"chunk_size": c, "parallel": False}))
    if driver == "compute_parallel":
        return chunks, list(plugin.compute(ctx, "run", streaming_config={"chunk_size": c, "max_workers": 3}))
    if driver == "run_chunks_serial":
        return chunks, plugin.run_chunks(chunks, ctx, "run", max_workers=1)
    if driver == "run_chunks_parallel":
        return chunks, plugin.run_chunks(chunks, ctx, "run", max_workers=3)
    assert driver == "compute_chunk"
    return chunks, [plugin.compute_chunk(ch, ctx, "run") for ch in chunks]


DRIVERS = ("compute_serial", "compute_parallel", "run_chunks_serial", "run_chunks_parallel", "compute_chunk")


def test_data_to_chunks_is_what_the_util_builds():
    for name in S.RUN_NAMES:
        run = S.run(name)
        plugin = HipThresholdHitStream()
        for c in run.chunk_sizes:
            plugin.chunk_size = c
            got = list(plugin._data_to_chunks(run.records, "run"))
            mine = run.chunks(c)
            assert [(g.start, g.end, g.metadata["segment_id"], g.data["record_id"].tolist()) for g in got] == \
                   [(m.start, m.end, m.metadata["segment_id"], m.data["record_id"].tolist()) for m in mine]


@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("name", S.RUN_NAMES)
def test_every_chunk_is_passed_the_runs_width(name, driver):
    run = S.run(name)
    ctx = _ctx(run)
    for use_filtered in BOTH:
        want = run.want(use_filtered)
        for c in run.chunk_sizes:
            dp = S.oracle_pool()
            plugin = HipThresholdHitStream(use_filtered=use_filtered, device_pool=dp)
            chunks, outs = _drive(plugin, run, ctx, driver, c)
            what = f"{name} {driver} chunk_size={c} filtered={use_filtered}"
            assert [e["max_len"] for e in dp.log] == [run.width] * len(chunks), what
            assert {e["source"] for e in dp.log} == {_lib.SRC_SG_FUSED if use_filtered else _lib.SRC_RAW}
            got = S.check_bookkeeping(run, chunks, outs, want, what)
            # the double answers with the oracle's rows of the chunk at the width it was given: the whole run's rows
            assert got.tobytes() == want.tobytes(), what
            dp.close()


def test_constructor_width_wins_and_a_smaller_one_is_refused_before_any_upload():
    run = S.run("ragged")
    ctx = _ctx(run)
    for driver in DRIVERS:
        dp = S.oracle_pool()
        plugin = HipThresholdHitStream(max_len=256, device_pool=dp)
        chunks, _outs = _drive(plugin, run, ctx, driver, 100)
        assert [e["max_len"] for e in dp.log] == [256] * len(chunks), driver
        dp = S.oracle_pool()
        plugin = HipThresholdHitStream(max_len=run.width, device_pool=dp)
        _drive(plugin, run, ctx, driver, 100)
        assert {e["max_len"] for e in dp.log} == {run.width}
        # chunk 2 of 100 records (200..299) holds no 200-sample record: a width of 199 passes the library's check
        # for it, and only the host can refuse it for the run
        dp = S.oracle_pool()
        plugin = HipThresholdHitStream(max_len=199, device_pool=dp)
        with pytest.raises(ValueError, match=r"max_len \(199\) is below the longest record of the run \(200\)"):
            if driver == "compute_chunk":
                plugin.compute_chunk(run.chunks(100)[2], ctx, "run")
            else:
                _drive(plugin, run, ctx, driver, 100)
        assert dp.uploads == [] and dp.log == [], driver


def test_width_without_records_in_the_context():
    """Ready-made chunks and a Context with nothing but the wave_pool: run_chunks pads to the longest record of the list
    it was given, compute_chunk to the chunk's own (the one caller for whom max_len=0 still means that)."""
    run = S.run("ragged")
    ctx = _ctx(run, records=False)
    chunks = run.chunks(100)
    for workers in (1, 3):
        dp = S.oracle_pool()
        outs = HipThresholdHitStream(device_pool=dp).run_chunks(chunks, ctx, "run", max_workers=workers)
        assert [e["max_len"] for e in dp.log] == [200] * len(chunks)
        assert np.concatenate([o.data for o in outs]).tobytes() == run.want(False).tobytes()
    dp = S.oracle_pool()
    plugin = HipThresholdHitStream(device_pool=dp)
    for ch in chunks:
        plugin.compute_chunk(ch, ctx, "run")
    assert [e["max_len"] for e in dp.log] == [0] * len(chunks)
    sub = [chunks[2], chunks[5]]   # a list whose longest record (120) is below the constructor's width: taken as given
    dp = S.oracle_pool()
    HipThresholdHitStream(max_len=150, device_pool=dp).run_chunks(sub, ctx, "run", max_workers=3)
    assert [e["max_len"] for e in dp.log] == [150, 150]
    with pytest.raises(ValueError, match="below the longest record"):
        HipThresholdHitStream(max_len=150, device_pool=S.oracle_pool()).run_chunks(chunks, ctx, "run", max_workers=3)


def test_width_follows_the_context_the_call_was_given():
    """One plugin, two runs: the width is resolved per call from that call's records, never kept from the last run."""
    a, b = S.run("ragged"), S.run("mixed")
    dp = S.oracle_pool()
    plugin = HipThresholdHitStream(device_pool=dp)
    for run in (a, b, a):
        dp.log.clear()
        plugin.run_chunks(run.chunks(100), _ctx(run), "run", max_workers=2)
        assert {e["max_len"] for e in dp.log} == {run.width}


# ---- options --------------------------------------------------------------------------------------------------------
def test_option_precedence():
    run = S.run("sparse")
    plugin = HipThresholdHitStream(threshold=33.0, right_extension=7)
    assert (plugin.threshold, plugin.le, plugin.re, plugin.use_filtered, plugin.sg) == (33.0, 2, 7, False, (11, 2))
    ctx = _ctx(run, {"hit_threshold_stream": {"threshold": 25.0, "left_extension": 5, "use_filtered": True},
                     "right_extension": 1, "sg_window_size": 7, "left_extension": 9})
    plugin._configure(ctx)
    # constructor > Context (plugin block > global key) > option default
    assert (plugin.threshold, plugin.le, plugin.re, plugin.use_filtered, plugin.sg) == (33.0, 5, 7, True, (7, 2))
    plugin._configure(_ctx(run))
    assert (plugin.threshold, plugin.le, plugin.re, plugin.use_filtered, plugin.sg) == (33.0, 2, 7, False, (11, 2))
    assert HipThresholdHitStream(left_extension=-3, right_extension=-1).le == 0
    # the Context's options reach the pass: a threshold no sample reaches gives no row, through every driver
    dp = S.oracle_pool()
    plugin = HipThresholdHitStream(device_pool=dp)
    ctx = _ctx(run, {"threshold": 1e9})
    for driver in DRIVERS:
        chunks, outs = _drive(plugin, run, ctx, driver, S.SPARSE_BLOCK)
        assert len(outs) == len(chunks) and all(len(o.data) == 0 for o in outs), driver


# ---- the staged slice -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "shuffled", "mixed"])
def test_staged_slice_and_rebased_offsets(name):
    run = S.run(name)
    c = run.chunk_sizes[0]
    dp = S.oracle_pool()
    chunks = run.chunks(c)
    HipThresholdHitStream(device_pool=dp).run_chunks(chunks, _ctx(run), "run", max_workers=3)
    assert len(dp.log) == len(chunks)
    for ch, entry in zip(chunks, dp.log):
        rec = ch.data
        lo = int(rec["wave_offset"].min())
        hi = int((rec["wave_offset"].astype(np.int64) + rec["event_length"]).max())
        np.testing.assert_array_equal(entry["pool"], run.pool[lo:hi])
        staged = entry["records"]
        assert staged["record_id"].tolist() == rec["record_id"].tolist()
        off = staged["wave_offset"].astype(np.int64)
        assert off.min() == 0 and np.all(off >= 0) and np.all(off <= hi - lo)
        assert np.all(off + staged["event_length"] <= hi - lo)
        np.testing.assert_array_equal(off, rec["wave_offset"] - lo)
        for f in ("event_length", "timestamp", "baseline", "polarity", "dt", "channel"):
            np.testing.assert_array_equal(staged[f], rec[f])
    assert run.records.flags.writeable is False      # (the driver rebases a copy)


# ---- the ring -------------------------------------------------------------------------------------------------------
def test_ring_order_sessions_and_empty_chunks():
    run = S.run("sparse")
    ctx = _ctx(run)
    chunks, k_empty = S.sparse_chunks_with_empty()
    staged_chunks = [c for c in chunks if len(c.data)]
    want = run.want(False)
    # two sessions per device of the pool, capped by max_workers, never fewer than two
    for devices, workers, ring in (((0,), 2, 2), ((0,), 3, 2), ((0,), 8, 2), ((0, 1), 3, 3), ((0, 1), 8, 4)):
        dp = S.oracle_pool(devices)
        plugin = HipThresholdHitStream(device_pool=dp)
        timeline = []
        outs = plugin.run_chunks(chunks, ctx, "run", max_workers=workers, timeline=timeline)
        got = S.check_bookkeeping(run, chunks, outs, want, f"workers={workers}")
        assert got.tobytes() == want.tobytes()
        assert len(outs[k_empty].data) == 0 and (outs[k_empty].start, outs[k_empty].end) == (chunks[k_empty].start,
                                                                                             chunks[k_empty].end)
        # input order; the zero-record chunk is never staged, and the ring is drained before its result is given
        assert [t[0] for t in timeline] == [k for k in range(len(chunks)) if k != k_empty]
        sessions = [e["session"] for e in dp.log]
        assert len(set(map(id, sessions))) == ring and dp.live_sessions == ring
        assert all(sessions[i] is sessions[i % ring] for i in range(len(sessions)))
        assert [e["n_records"] for e in dp.log] == [len(c.data) for c in staged_chunks]
        stamps = {t[0]: t for t in timeline}
        for k in range(len(chunks) - 1):
            if k == k_empty or k + 1 == k_empty:
                continue
            (_k, _b, queued, collected), (_k1, begin1, queued1, _c1) = stamps[k], stamps[k + 1]
            assert queued <= begin1 <= queued1 <= collected, (workers, k)
        assert stamps[k_empty - 1][3] <= stamps[k_empty + 1][1]     # drained before the chunk behind the empty one
        for _again in range(2):
            plugin.run_chunks(chunks, ctx, "run", max_workers=workers)
        assert dp.live_sessions == ring
    # the generator entry points give the empty chunk's result in place as well
    dp = S.oracle_pool()
    plugin = HipThresholdHitStream(device_pool=dp)
    outs = plugin.run_chunks(chunks, ctx, "run", max_workers=1)
    assert [len(o.data) for o in outs] == [2 * S.SPARSE_BLOCK if len(c.data) and p else 0
                                           for c, p in zip(chunks, _pattern_with_empty(k_empty))]


def _pattern_with_empty(k_empty):
    pattern = list(S.SPARSE_PATTERN)
    return pattern[:k_empty] + [False] + pattern[k_empty:]
