"""The event stream on the device: wfa_event_stream_* through DeviceSession against the static grouping pass of the same
library (group_hit_windows_flat, pinned to the reference's frames by tests/test_event_grouping.py), push by push against
the numpy rule (tests/event_stream_util.py), and HipHitGroupedStream end to end against HipHitGroupedPlugin on
HipThresholdHitPlugin's rows."""

import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import event_stream_util as E
from tests import stream_hits_util as S
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DevicePool, DeviceSession
from waveformanalysis_amd.dtypes import EVENT_HIT_DTYPE, THRESHOLD_HIT_DTYPE
from waveformanalysis_amd.event_grouping import EVENT_COLUMNS, group_hit_windows_flat
from waveformanalysis_amd.event_stream import (
    HipHitGroupedStream,
    event_rows,
    events_frame,
    horizon_margin,
    horizon_of,
)
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipHitGroupedPlugin, HipThresholdHitPlugin

pytestmark = pytest.mark.gpu
WINDOWS = (0.0, 100.0, 5000.0, 2000000.0)


@pytest.fixture(scope="module")
def sess():
    with DeviceSession(0) as s:
        yield s


@pytest.fixture(scope="module")
def static_sess():
    with DeviceSession(0) as s:
        yield s


@pytest.fixture(scope="module")
def dp():
    pool = DevicePool([0])
    yield pool
    pool.close()


STATIC: dict = {}


def _static(static_sess, key, hits, window):
    """Rows of the static pass over the whole table, computed once per (table, window)."""
    if key not in STATIC:
        rows = event_rows(hits, group_hit_windows_flat(hits, window, session=static_sess))
        rows.setflags(write=False)
        STATIC[key] = rows
    return STATIC[key]


def _stream(sess, window, hits, chunk_size, horizons=None):
    sess.event_stream_begin(window)
    try:
        return E.stream_rows(sess.event_stream_push, hits, chunk_size, horizons)
    finally:
        sess.event_stream_end()


# ---- the two golden hit tables ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_size", (1, 3, 7, 64, "n+1"))
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", E.GOLDEN_TABLES)
def test_golden_tables_equal_the_static_pass(name, window, chunk_size, sess, static_sess):
    hits, windows, _z = E.golden(name)
    assert window in windows
    want = _static(static_sess, (name, window), hits, window)
    c = len(hits) + 1 if chunk_size == "n+1" else chunk_size
    got = _stream(sess, window, hits, c)
    assert got.dtype == EVENT_HIT_DTYPE and len(got) == len(hits)
    assert got.tobytes() == want.tobytes()
    ids = got["event_id"]
    assert ids[0] == 0 and set(np.diff(ids).tolist()) <= {0, 1}      # 0 .. n_events - 1 without a gap
    assert want.tobytes() == E.static_rows(hits, window).tobytes()   # (and the numpy rule agrees with the static pass)


# ---- hand-made tables ---------------------------------------------------------------------------------------------------
def _push_by_push(sess, static_sess, window, pushes, hits_all=None):
    """Each (rows, horizon) push against the numpy rule, all rows against the static pass over all pushed rows."""
    rule = E.NumpyStream(window)
    parts = []
    sess.event_stream_begin(window)
    try:
        for k, (rows, horizon) in enumerate(pushes):
            got, carry = sess.event_stream_push(rows, horizon)
            want, want_carry = rule.push(rows, horizon)
            assert (got.tobytes(), carry) == (want.tobytes(), want_carry), (k, len(got), len(want), carry, want_carry)
            parts.append(got)
    finally:
        sess.event_stream_end()
    table = np.concatenate([r for r, _h in pushes if r is not None and len(r)]) if hits_all is None else hits_all
    rows = np.concatenate(parts)
    assert rows.tobytes() == event_rows(table, group_hit_windows_flat(table, window, session=static_sess)).tobytes()
    return parts


def test_event_open_across_three_pushes(sess, static_sess):
    # one hit of 300 ns keeps its event open while short hits of the next two pushes fall into it
    a = E.make_hits([(1_000_000, 300_000, 0, 0), (1_002_000, 4000, 0, 1)])
    b = E.make_hits([(1_100_000, 4000, 0, 2), (1_150_000, 4000, 0, 1)])
    c = E.make_hits([(1_290_000, 4000, 0, 3), (2_000_000, 4000, 0, 0)])
    for t, base in ((b, 2), (c, 4)):
        t["record_id"] += base
    parts = _push_by_push(sess, static_sess, 10.0, [(a, 1_100_000.0), (b, 1_290_000.0), (c, 2_000_000.0), (None, math.inf)])
    assert [len(p) for p in parts] == [0, 0, 5, 1]
    assert parts[2]["event_id"].tolist() == [0] * 5 and parts[3]["event_id"].tolist() == [1]


def test_push_without_rows_in_the_middle(sess, static_sess):
    a = E.make_hits([(1000, 4000, 0, 0), (500_000, 4000, 0, 1)])
    b = E.make_hits([(900_000, 4000, 0, 0)])
    b["record_id"] += 2
    empty = np.zeros(0, dtype=THRESHOLD_HIT_DTYPE)
    parts = _push_by_push(sess, static_sess, 100.0, [(a, 500_000.0), (empty, 700_000.0), (None, 900_000.0), (b, 900_000.0),
                                                     (None, math.inf)])
    assert [len(p) for p in parts] == [1, 1, 0, 0, 1]


def test_horizon_boundary_is_strict(sess, static_sess):
    # event [0, 4000], window 1 ns: max + gap = 5000 == H and a later hit at abs_start == H joins the event
    a = E.make_hits([(0, 4000, 0, 0)])
    b = E.make_hits([(5000, 2000, 0, 1), (50_000, 2000, 0, 0)])
    b["record_id"] += 1
    parts = _push_by_push(sess, static_sess, 1.0, [(a, 5000.0), (b, math.inf)])
    assert [len(p) for p in parts] == [0, 3] and parts[1]["event_id"].tolist() == [0, 0, 1]
    # H one ps larger: the event closes (and the later hit, now at 5001, opens the next)
    b2 = b.copy()
    b2["timestamp"][0] = 5001
    parts = _push_by_push(sess, static_sess, 1.0, [(a, 5001.0), (b2, math.inf)])
    assert [len(p) for p in parts] == [1, 2] and parts[1]["event_id"].tolist() == [1, 2]


def test_window_zero_one_event_two_dt_and_ties(sess, static_sess):
    # window 0: touching hits chain, a gap of 1 ps splits
    hits = E.make_hits([(0, 4000, 0, 0), (4000, 4000, 0, 1), (8001, 4000, 0, 0), (12_001, 2000, 0, 2)])
    parts = _push_by_push(sess, static_sess, 0.0, [(hits[:2], 4000.0), (hits[2:], math.inf)])
    assert np.concatenate(parts)["event_id"].tolist() == [0, 0, 1, 1]
    # all hits in one event, pushed in four parts: nothing comes out before the flush
    rng = np.random.default_rng(3)
    one = E.make_hits([(int(t), 6000, 0, int(c)) for t, c in zip(np.sort(rng.integers(0, 40_000, 32)), rng.integers(0, 4, 32))])
    horizons = E.row_horizons(one, 8)
    parts = _push_by_push(sess, static_sess, 100.0, [(one[lo : lo + 8], horizons[k]) for k, lo in enumerate(range(0, 32, 8))]
                          + [(None, math.inf)])
    assert [len(p) for p in parts] == [0, 0, 0, 32, 0]
    # two channels with different dt; equal abs_start on two channels (the order inside the event is by channel, then dt)
    mix = E.make_hits([(10_000, 8000, 0, 1, 4), (10_000, 8000, 0, 0, 2), (10_000, 4000, 0, 1, 2), (12_000, 8000, 1, 0, 4),
                       (900_000, 8000, 0, 0, 4), (900_000, 8000, 0, 0, 2)])
    parts = _push_by_push(sess, static_sess, 100.0, [(mix[:3], 12_000.0), (mix[3:], math.inf)])
    rows = np.concatenate(parts)
    assert rows["record_id"].tolist() == [1, 2, 0, 3, 5, 4]
    assert rows["t_max"].tolist() == [20_000] * 4 + [908_000] * 2


def test_timestamps_at_2_to_60_with_rounding_windows(sess, static_sess):
    # one ulp is 256 ps; dt = 3 ns and odd record timestamps make float(ts), the product and the sum all round
    rng = np.random.default_rng(11)
    n_rec = 16
    rec_ts = 2**60 + np.arange(n_rec, dtype=np.int64) * 1_000_003 + rng.integers(0, 255, n_rec)
    hits = np.zeros(2 * n_rec, dtype=THRESHOLD_HIT_DTYPE)
    def computed_start(ts, pos, start):
        return float(ts) + (float(start) - float(pos)) * (3.0 * 1e3)

    for i in range(2 * n_rec):
        r = i // 2
        pos = int(rng.integers(3, 60))
        start = int(rng.integers(0, pos + 1))
        if i % 2 == 0:   # a hit on the record's first sample, at a position where the roundings put it below float(record ts)
            start = 0
            pos = next((p for p in range(3, 60) if computed_start(int(rec_ts[r]) + p * 3000, p, 0) < float(rec_ts[r])), pos)
        hits[i] = (pos, float(i), 1.0, start, pos + int(rng.integers(1, 9)), 0.0, 3, 0.0, 0.0, int(rec_ts[r]) + pos * 3000,
                   0, i % 3, r)
    a0, _ = E.windows_of(hits)
    margin = horizon_margin(int(rec_ts.max()) + 3 * 1000 * 80)
    assert margin == 512.0
    assert np.any(a0 < rec_ts[hits["record_id"]].astype(np.float64))       # float(minimum) alone is no horizon here
    pushes = []
    for lo in range(0, n_rec, 4):                                          # four records (eight hits) per push
        later = int(rec_ts[lo + 4:].min()) if lo + 4 < n_rec else None
        pushes.append((hits[2 * lo : 2 * lo + 8], horizon_of(later, margin)))
    parts = _push_by_push(sess, static_sess, 30.0, pushes + [(None, math.inf)])
    assert sum(len(p) for p in parts[:-2]) > 0                             # events did close before the last records


def _assert_invalid(call, match):
    with pytest.raises(ValueError, match=match):
        call()


def test_refusals_leave_the_stream_untouched(sess, static_sess):
    a = E.make_hits([(1000, 4000, 0, 0), (400_000, 4000, 0, 1), (402_000, 4000, 0, 2)])
    b = E.make_hits([(404_000, 4000, 0, 0), (900_000, 4000, 0, 1)])
    b["record_id"] += 3
    window = 100.0
    rule = E.NumpyStream(window)
    with pytest.raises(ValueError, match="time_window_ns must be >= 0"):
        sess.event_stream_begin(-1.0)
    n = C.c_int64(0)
    lib = _lib.load()
    assert lib.wfa_event_stream_push(sess._h, None, 0, 0.0, C.byref(n), C.byref(n), C.byref(n)) == _lib.WFA_E_STATE
    sess.event_stream_begin(window)
    try:
        out = np.zeros(4, dtype=EVENT_HIT_DTYPE)
        assert lib.wfa_event_stream_fill(sess._h, out.ctypes.data_as(C.c_void_p), 0) == _lib.WFA_E_STATE   # before a push
        got, carry = sess.event_stream_push(a, 400_000.0)
        want, want_carry = rule.push(a, 400_000.0)
        assert (got.tobytes(), carry) == (want.tobytes(), want_carry) and carry == 2
        assert lib.wfa_event_stream_fill(sess._h, out.ctypes.data_as(C.c_void_p), 4) == _lib.WFA_E_INVALID  # another count
        accepted = len(got)
        assert 0 < accepted <= len(out)

        def nothing_to_fill():      # after a refused push: not with the last accepted push's count, not with 0
            return all(lib.wfa_event_stream_fill(sess._h, out.ctypes.data_as(C.c_void_p), count) == _lib.WFA_E_STATE
                       for count in (accepted, 0))

        bad = b.copy()
        bad["dt"][1] = 0
        _assert_invalid(lambda: sess.event_stream_push(bad, 900_000.0), "dt must be positive")
        assert nothing_to_fill()
        for field in ("edge_start", "edge_end"):
            bad = b.copy()
            bad[field][0] = -1
            _assert_invalid(lambda: sess.event_stream_push(bad, 900_000.0), "negative edge_start / edge_end")
            assert nothing_to_fill()
        bad = b.copy()
        bad["timestamp"][0] = 399_999                                        # starts below the previous horizon
        _assert_invalid(lambda: sess.event_stream_push(bad, 900_000.0), "below the previous push's horizon")
        assert nothing_to_fill()
        _assert_invalid(lambda: sess.event_stream_push(b, 399_999.0), "lies below the previous push's")
        assert nothing_to_fill()
        _assert_invalid(lambda: sess.event_stream_push(b, math.nan), "NaN")
        assert nothing_to_fill()
        rc = lib.wfa_event_stream_push(sess._h, b.ctypes.data_as(C.c_void_p), 2**31 - 2, 900_000.0, C.byref(n), C.byref(n),
                                       C.byref(n))                           # carry (2) + rows = 2^31: refused unread
        assert rc == _lib.WFA_E_INVALID and "table limit" in _lib.last_error()
        assert nothing_to_fill()
        # the carry is intact: the valid push gives what the rule gives without the refused ones
        got, carry = sess.event_stream_push(b, 900_000.0)
        want, want_carry = rule.push(b, 900_000.0)
        assert (got.tobytes(), carry) == (want.tobytes(), want_carry) and len(got) == 3 and carry == 1
        got, carry = sess.event_stream_push(None, math.inf)
        assert got.tobytes() == rule.push(None, math.inf)[0].tobytes() and carry == 0
    finally:
        sess.event_stream_end()
    assert lib.wfa_event_stream_push(sess._h, None, 0, 0.0, C.byref(n), C.byref(n), C.byref(n)) == _lib.WFA_E_STATE


def test_release_scratch_between_pushes_changes_nothing(sess, static_sess):
    hits, _w, _z = E.golden("grouping_v1725")
    want = _static(static_sess, ("grouping_v1725", 100.0), hits, 100.0)
    horizons = E.row_horizons(hits, 500)
    parts, carried = [], []
    sess.event_stream_begin(100.0)
    try:
        for k, lo in enumerate(range(0, len(hits), 500)):
            got, carry = sess.event_stream_push(hits[lo : lo + 500], horizons[k])
            parts.append(got)
            carried.append(carry)
            before = sess.scratch_bytes()
            assert before > 0 and sess.release_scratch() == before and sess.scratch_bytes() == 0   # the carry is not scratch
        parts.append(sess.event_stream_push(None, math.inf)[0])
    finally:
        sess.event_stream_end()
    assert max(carried) > 0
    assert np.concatenate(parts).tobytes() == want.tobytes()


# ---- the plugin end to end ----------------------------------------------------------------------------------------------
CONFIG = {"threshold": S.THRESHOLD, "left_extension": S.LE, "right_extension": S.RE, "time_window_ns": 100.0}


@functools.cache
def _static_frame(name):
    run = S.run(name)
    ctx = SimpleContext({"wave_source": "records", **CONFIG}, {"records": run.records, "wave_pool": run.pool},
                        plugins=[HipThresholdHitPlugin(), HipHitGroupedPlugin()])
    return ctx.get_data("run", "hit_grouped")


def _assert_frames_equal(got, want):
    assert list(got.columns) == list(want.columns) == EVENT_COLUMNS and len(got) == len(want)
    for column in EVENT_COLUMNS:
        assert got[column].dtype == want[column].dtype, column
        if got[column].dtype != object:
            np.testing.assert_array_equal(got[column].to_numpy(), want[column].to_numpy(), err_msg=column)
            continue
        for k, (a, b) in enumerate(zip(got[column], want[column])):
            assert a.dtype == b.dtype and np.array_equal(a, b), (column, k)


@pytest.mark.parametrize("workers", (1, 4), ids=("serial", "ring"))
@pytest.mark.parametrize("chunk_size", (1, 7, 1000))
@pytest.mark.parametrize("name", ("ragged", "mixed", "shuffled"))
def test_plugin_equals_the_static_chain(name, chunk_size, workers, dp):
    run = S.run(name)
    ctx = SimpleContext({"wave_source": "records", **CONFIG}, {"records": run.records, "wave_pool": run.pool})
    plugin = HipHitGroupedStream(device_pool=dp)
    cfg = {"chunk_size": chunk_size, "parallel": workers > 1, "max_workers": workers}
    outs = list(plugin.compute(ctx, "run", streaming_config=cfg))
    for o in outs:
        assert o.data.dtype == EVENT_HIT_DTYPE and len(o.data)
        assert (o.start, o.end) == (int(o.data["t_min"].min()), int(o.data["t_max"].max()) + 1)
    rows = np.concatenate([o.data for o in outs])
    want = _static_frame(name)
    assert len(want) > 10
    _assert_frames_equal(events_frame(rows), want)
    assert plugin.stats["pushes"] == len(run.chunks(chunk_size)) + 1 and plugin.stats["rows_out"] == len(rows)
    if chunk_size == 1:
        assert len(outs) > 10 and plugin.stats["max_carry"] < len(rows) // 4    # events leave as they close


def test_run_without_hits_gives_no_chunks(dp):
    rec = S.run("sparse").records[:120].copy()
    pool = np.full(int((rec["wave_offset"] + rec["event_length"]).max()), S.BASELINE, dtype=np.uint16)
    ctx = SimpleContext({"wave_source": "records", **CONFIG}, {"records": rec, "wave_pool": pool})
    plugin = HipHitGroupedStream(device_pool=dp)
    assert list(plugin.compute(ctx, "run", streaming_config={"chunk_size": 50})) == []
    assert plugin.stats["pushes"] == 4 and plugin.stats["rows_in"] == 0
