"""The merged-event stream on the device: wfa_merged_event_stream_* through DeviceSession, push by push against the numpy
rule (tests/merged_event_stream_util.py), against the static device pass over all pushed rows (static merge, then
group_hit_windows with components), against the events of merged hits the reference recorded, and
HipHitMergedGroupedStream end to end against the static plugin chain."""

import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import event_stream_util as E
from tests import merged_event_stream_util as U
from tests import stream_hits_util as S
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DevicePool, DeviceSession
from waveformanalysis_amd.dtypes import EVENT_MERGED_HIT_DTYPE, HIT_MERGED_DTYPE, THRESHOLD_HIT_DTYPE
from waveformanalysis_amd.event_grouping import group_hit_windows_flat
from waveformanalysis_amd.hit_merge import compute_cluster_rows, compute_component_rows, compute_merged_rows
from waveformanalysis_amd.merged_event_stream import HipHitMergedGroupedStream, merged_events_frame
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import (
    HipHitGroupedPlugin,
    HipHitMergeClustersPlugin,
    HipHitMergedComponentsPlugin,
    HipHitMergePlugin,
    HipThresholdHitPlugin,
)

pytestmark = pytest.mark.gpu
WIDTH = 10000.0


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


def _static_pass(static_sess, hits, gap, width, window):
    """(event rows, hit_merged, hit_merged_components) of the static device pass over the whole table: static merge, then
    group_hit_windows with components."""
    clusters = compute_cluster_rows(static_sess, hits, gap, width, None, "hit_merge_clusters")
    merged = compute_merged_rows(static_sess, hits, clusters, None, "hit_merged")
    components = compute_component_rows(merged, clusters)
    flat = group_hit_windows_flat(merged, window, component_rows=components, component_hits=hits, session=static_sess)
    ev = {k: np.asarray(flat[k], dtype=np.int64) for k in ("order", "event_start", "t_min", "t_max")}
    return U.rows_of(merged, ev), merged, components


def _assert_equals_static(rows, hit_index, want, what=None):
    """Stream rows against the static pass's, row by row: every field but component_offset, and the members the offsets
    address."""
    want_rows, _merged, components = want
    assert rows.dtype == EVENT_MERGED_HIT_DTYPE and len(rows) == len(want_rows), (what, len(rows), len(want_rows))
    for field in EVENT_MERGED_HIT_DTYPE.names:
        if field != "component_offset":
            assert np.array_equal(rows[field], want_rows[field]), (what, field)
    assert len(hit_index) == len(components)
    static_index = np.asarray(components["hit_index"], dtype=np.int64)
    counts = rows["component_count"].astype(np.int64)
    take = np.repeat(rows["component_offset"] - np.cumsum(counts) + counts, counts) + np.arange(int(counts.sum()))
    take_static = np.repeat(want_rows["component_offset"] - np.cumsum(counts) + counts, counts) + np.arange(int(counts.sum()))
    assert np.array_equal(hit_index[take], static_index[take_static]), what


def _stream(sess, gap, width, window, hits, chunk_size, horizons=None, margin=0.0):
    sess.merged_event_stream_begin(gap, width, window, margin)
    try:
        return U.stream_all(sess.merged_event_stream_push, hits, chunk_size, horizons)
    finally:
        sess.merged_event_stream_end()


def _same(got, want):
    return (got[0].tobytes(), got[1].tolist(), got[2:]) == (want[0].tobytes(), want[1].tolist(), want[2:])


def _push_by_push(sess, static_sess, gap, width, window, pushes, margin=0.0):
    """Each (rows, horizon) push against the numpy rule on every returned value -- rows, hit_index, both carry sizes and
    G -- and all of them against the static device pass over all pushed rows."""
    rule = U.NumpyMergedEventStream(gap, width, window, margin)
    parts = []
    sess.merged_event_stream_begin(gap, width, window, margin)
    try:
        for k, (rows, horizon) in enumerate(pushes):
            got = sess.merged_event_stream_push(rows, horizon)
            want = rule.push(rows, horizon)
            assert got[0].dtype == EVENT_MERGED_HIT_DTYPE and got[1].dtype == np.int64
            assert _same(got, want), (k, got, want)
            parts.append(got)
    finally:
        sess.merged_event_stream_end()
    assert parts[-1][2:4] == (0, 0)
    table = np.concatenate([r for r, _h in pushes if r is not None and len(r)])
    _assert_equals_static(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                          _static_pass(static_sess, table, gap, width, window))
    return parts


# ---- the two recorded hit tables ----------------------------------------------------------------------------------------
STATIC: dict = {}


@pytest.mark.parametrize("chunk_size", (1, 3, 7, 64, "n+1"))
@pytest.mark.parametrize("tw", (0, 100, 5000))
@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("name", U.FIXTURES)
def test_recorded_events_of_merged_hits(name, k, tw, chunk_size, sess, static_sess):
    case = U.fixture(name)
    hits = case["hits"]
    cfg = {"merge_gap_ns": 0.0, "max_total_width_ns": WIDTH, **case["configs"][k]}
    assert float(tw) in [float(w) for w in case["windows"]]
    if (name, k, tw) not in STATIC:
        STATIC[name, k, tw] = _static_pass(static_sess, hits, cfg["merge_gap_ns"], cfg["max_total_width_ns"], float(tw))
        for table in STATIC[name, k, tw]:
            table.setflags(write=False)
        U.assert_recorded(STATIC[name, k, tw][0], case, f"g{k}_w{tw}")        # (and the static pass gives the recorded columns)
    rows, hit_index = _stream(sess, cfg["merge_gap_ns"], cfg["max_total_width_ns"], float(tw), hits,
                              U.chunk_size_of(chunk_size, len(hits)))
    U.assert_recorded(rows, case, f"g{k}_w{tw}")
    _assert_equals_static(rows, hit_index, STATIC[name, k, tw], (name, k, tw, chunk_size))


# ---- hand-made tables ---------------------------------------------------------------------------------------------------
def test_a_cluster_spanning_two_records_takes_its_member_window(sess, static_sess):
    # gap 20 ns: [0, 4000] of record 0 and [6000, 10000] of record 1 merge into a row with edges -1, -1, anchored on the
    # second hit.  Its member window [0, 10000] reaches channel 1's hit at 12000 under a 3 ns window: one event.  The anchor
    # formula on -1 would put the row at -16000 and the hit at 12000 into an event of its own.
    hits = E.make_hits([(0, 4000, 0, 0), (6000, 4000, 0, 0), (12_000, 2000, 0, 1)])
    parts = _push_by_push(sess, static_sess, 20.0, WIDTH, 3.0, [(hits[:2], 12_000.0), (hits[2:], math.inf)])
    rows = np.concatenate([p[0] for p in parts])
    assert rows["event_id"].tolist() == [0, 0] and rows["channel"].tolist() == [0, 1]
    assert (rows["sample_start"].tolist(), rows["sample_end"].tolist()) == ([-1, 10], [-1, 11])
    assert (rows["t_min"].tolist(), rows["t_max"].tolist()) == ([0, 0], [14_000, 14_000])
    assert rows["component_count"].tolist() == [2, 1] and int(rows["timestamp"][0]) == 6000
    # the same two hits in ONE record: the row has a sample window and the anchor formula gives the same extent
    one = hits.copy()
    one["record_id"][:2] = 4
    one["position"][1], one["edge_start"][1], one["edge_end"][1] = 13, 13, 15          # (timestamp - position * dt = -20000 for both)
    rows = np.concatenate([p[0] for p in _push_by_push(sess, static_sess, 20.0, WIDTH, 3.0, [(one, math.inf)])])
    assert (rows["sample_start"].tolist(), rows["t_min"].tolist(), rows["t_max"].tolist()) == ([10, 10], [0, 0], [14_000, 14_000])


def test_open_start_holds_the_grouping_horizon_back(sess, static_sess):
    # gap 100 ns, H = 1 us: channel 0's cluster [1000, 951000] ends within the gap of H and stays open; channel 1's single hit
    # [2000, 6000] closes at once, but its event waits: G = open_start = 1000, whatever H
    hits = E.make_hits([(1000, 950_000, 0, 0), (2000, 4000, 0, 1)])
    parts = _push_by_push(sess, static_sess, 100.0, 1e6, 1.0, [(hits, 1_000_000.0), (None, 2_000_000.0), (None, math.inf)])
    assert [len(p[0]) for p in parts] == [0, 2, 0]
    assert parts[0][1].tolist() == [1] and parts[0][2:] == (1, 1, 1000.0)         # nothing delivered, group_horizon == 1000.0
    assert parts[1][0]["event_id"].tolist() == [0, 0] and parts[1][0]["channel"].tolist() == [0, 1]
    assert parts[1][0]["component_offset"].tolist() == [1, 0] and parts[1][1].tolist() == [0] and parts[1][4] == 2_000_000.0


def test_an_event_carried_over_two_buffer_flips(sess, static_sess):
    # gap 0, window 100 ns.  Push 1: E leaves, X stays (flip).  Push 2: Y joins X's event, nothing leaves (the table is the
    # carry, grown in place).  Push 3: the event of X and Y leaves, W stays (flip back).  X closed as a cluster in push 1.
    a = E.make_hits([(0, 4000, 0, 0), (200_000, 4000, 0, 1)])
    b = E.make_hits([(300_000, 4000, 0, 0)])
    c = E.make_hits([(900_000, 4000, 0, 1)])
    b["record_id"] += 2
    c["record_id"] += 3
    parts = _push_by_push(sess, static_sess, 0.0, WIDTH, 100.0, [(a, 300_000.0), (b, 304_000.0), (c, 1_000_000.0),
                                                                 (None, math.inf)])
    assert [len(p[0]) for p in parts] == [1, 0, 2, 1] and [p[3] for p in parts] == [1, 2, 1, 0]
    assert [p[1].tolist() for p in parts] == [[0, 1], [2], [3], []]
    assert parts[2][0]["event_id"].tolist() == [1, 1] and parts[2][0]["component_offset"].tolist() == [2, 1]
    assert parts[3][0]["event_id"].tolist() == [2]


def test_the_event_boundary_is_strict(sess, static_sess):
    # [1000, 5000], window 1 ns: max(abs_end) + window == G = 6000 holds the event, one ps more releases it
    hit = E.make_hits([(1000, 4000, 0, 0)])
    parts = _push_by_push(sess, static_sess, 0.0, WIDTH, 1.0, [(hit, 6000.0), (None, 6001.0), (None, math.inf)])
    assert [len(p[0]) for p in parts] == [0, 1, 0] and parts[0][2:] == (0, 1, 6000.0)
    # and a later row at abs_start == max(abs_end) + window does join
    late = E.make_hits([(6000, 2000, 0, 3)])
    late["record_id"] += 1
    parts = _push_by_push(sess, static_sess, 0.0, WIDTH, 1.0, [(hit, 6000.0), (late, math.inf)])
    assert [len(p[0]) for p in parts] == [0, 2] and parts[1][0]["event_id"].tolist() == [0, 0]


def test_a_tie_inside_one_channel_keeps_chain_order(sess, static_sess):
    # width cap 6 ns: [0, 8000] and [0, 2000] of one channel cannot merge (8 ns), so two clusters start at 0 with equal dt,
    # timestamp and record_id: every sort key ties, and chain order -- the first row first -- must survive both sorts
    hits = E.make_hits([(0, 8000, 0, 2), (0, 2000, 0, 2), (4000, 2000, 0, 1)])
    hits["record_id"] = 5
    for pushes in ([(hits, math.inf)], [(hits[:2], 4000.0), (hits[2:], math.inf)]):
        parts = _push_by_push(sess, static_sess, 50.0, 6.0, 10.0, pushes)
        rows = np.concatenate([p[0] for p in parts])
        assert rows["event_id"].tolist() == [0, 0, 0] and rows["channel"].tolist() == [1, 2, 2]
        assert rows["height"].tolist() == [2.0, 0.0, 1.0] and rows["sample_end"].tolist() == [11, 14, 11]


def test_gap_zero_equals_the_plain_event_stream(sess, static_sess):
    rng = np.random.default_rng(5)
    hits = E.make_hits([(int(t), 4000, 0, int(c)) for t, c in zip(np.sort(rng.integers(0, 600_000, 40)), rng.integers(0, 3, 40))])
    hits["width"] = rng.random(40).astype(np.float32)
    horizons = E.row_horizons(hits, 8)
    pushes = [(hits[lo : lo + 8], horizons[k]) for k, lo in enumerate(range(0, 40, 8))] + [(None, math.inf)]
    parts = _push_by_push(sess, static_sess, 0.0, WIDTH, 20.0, pushes)
    sess.event_stream_begin(20.0)
    try:
        plain = [sess.event_stream_push(rows, horizon) for rows, horizon in pushes]
    finally:
        sess.event_stream_end()
    assert sum(len(p[0]) for p in parts[:-2]) > 0 and max(p[3] for p in parts) > 0
    for got, (want, n_carry) in zip(parts, plain):                  # every hit is its own row: the same events, push by push
        assert len(got[0]) == len(want) and got[3] == n_carry and set(got[0]["component_count"].tolist()) <= {1}
        for field in ("event_id", "t_min", "t_max") + THRESHOLD_HIT_DTYPE.names:
            merged_field = {"edge_start": "sample_start", "edge_end": "sample_end"}.get(field, field)
            assert np.array_equal(got[0][merged_field], want[field]), field


@pytest.mark.parametrize("same_channel", (False, True))
def test_timestamps_at_2_to_60_with_rounding_windows(same_channel, sess, static_sess):
    # the construction of the merge stream's test (U.late_pushes): one ulp is 256 ps; dt = 3 ns and odd record timestamps
    # make float(ts), the product and the sum all round
    pushes, margin = U.late_pushes(same_channel)
    assert margin == 512.0
    for gap in (30.0, 900.0):                                              # (900 ns reaches into the next record)
        parts = _push_by_push(sess, static_sess, gap, 1e9, 100.0, pushes + [(None, math.inf)], margin)   # (no refusal)
        assert sum(len(p[0]) for p in parts[:-2]) > 0                      # events did leave before the last records
        assert all(a[4] <= b[4] for a, b in zip(parts[:-1], parts[1:]))
    assert any(c > 1 for c in np.concatenate([p[0] for p in parts])["component_count"])
    rows = np.concatenate([p[0] for p in parts])        # member windows as given, anchor windows of clusters in one channel
    assert (rows["sample_start"] < 0).any() == (not same_channel)
    assert (rows["component_count"][rows["sample_start"] >= 0] > 1).any() == same_channel


# ---- sizes at block edges -----------------------------------------------------------------------------------------------
def test_257_single_hit_clusters_in_257_events(sess, static_sess):
    # 257 rows in 257 events: a last thread block of one row; 257 * 24 dwords end inside a block
    hits = E.make_hits([(1_000_000 * i, 4000, 0, i % 5) for i in range(257)])
    parts = _push_by_push(sess, static_sess, 20.0, WIDTH, 100.0, [(hits, math.inf)])
    assert parts[0][0]["event_id"].tolist() == list(range(257)) and sorted(parts[0][1].tolist()) == list(range(257))
    # gap 2 us, hits of a channel 5 us apart: nothing merges, the two hits that end within the gap of the horizon wait and
    # hold G at the first of them
    parts = _push_by_push(sess, static_sess, 2000.0, WIDTH, 100.0, [(hits[:256], float(1_000_000 * 256)), (hits[256:], math.inf)])
    assert [len(p[0]) for p in parts] == [254, 3] and parts[0][2:] == (2, 0, 254_000_000.0)


def _consistent_hits(n, seed):
    """n hits, three per record, the hits of a record sharing channel, dt and timestamp - position * dt; records overlap
    in time inside a channel, so clusters form inside records and across them."""
    rng = np.random.default_rng(seed)
    n_rec = (n + 2) // 3
    rec_ts = np.sort(rng.integers(0, 18 * n, n_rec)) * 2000
    rid = np.arange(n) // 3
    hits = np.zeros(n, dtype=THRESHOLD_HIT_DTYPE)
    hits["position"] = rng.integers(4, 400, n)
    hits["edge_start"] = hits["position"] - rng.integers(0, 4, n)
    hits["edge_end"] = hits["position"] + rng.integers(1, 6, n)
    hits["dt"] = 2
    hits["timestamp"] = rec_ts[rid] + hits["position"] * 2000
    hits["channel"] = rng.integers(0, 16, n_rec)[rid]
    hits["board"] = rng.integers(0, 2, n_rec)[rid]
    hits["record_id"] = rid
    hits["height"] = rng.integers(1, 50, n)
    hits["integral"] = rng.random(n)
    hits["width"] = rng.random(n)
    return hits


def test_65537_hits_in_three_pushes(sess, static_sess):
    n = 65_537
    hits = _consistent_hits(n, 17)
    gap, width, window = 600.0, 5000.0, 50.0
    want = _static_pass(static_sess, hits, gap, width, window)
    assert 1.5 < n / len(want[1]) < 20 and (want[1]["sample_start"] < 0).any() and (want[1]["component_count"][want[1]["sample_start"] >= 0] > 1).any()
    assert 100 < int(want[0]["event_id"][-1]) < len(want[1])
    sess.merged_event_stream_begin(gap, width, window)
    try:
        rows, members, carried = [], [], []
        horizons = E.row_horizons(hits, 30_000)
        for k, lo in enumerate(range(0, n, 30_000)):
            out = sess.merged_event_stream_push(hits[lo : lo + 30_000], horizons[k])
            rows.append(out[0]), members.append(out[1]), carried.append(out[2:4])
        assert carried[-1] == (0, 0) and min(sum(c) for c in carried[:-1]) > 0 and len(rows) == 3
    finally:
        sess.merged_event_stream_end()
    _assert_equals_static(np.concatenate(rows), np.concatenate(members), want)


# ---- refusals, scratch, shared sessions ---------------------------------------------------------------------------------
def _assert_invalid(call, match):
    with pytest.raises(ValueError, match=match):
        call()


def test_refusals_leave_the_stream_untouched(sess):
    a = E.make_hits([(1000, 4000, 0, 0), (400_000, 4000, 0, 1), (402_000, 4000, 0, 2)])
    b = E.make_hits([(404_000, 4000, 0, 1), (900_000, 4000, 0, 1)])
    b["record_id"] += 3
    gap, window = 100.0, 1.0
    rule = U.NumpyMergedEventStream(gap, WIDTH, window)
    for bad in ((-1.0, WIDTH, window, 0.0), (gap, -1.0, window, 0.0), (gap, WIDTH, -1.0, 0.0), (math.nan, WIDTH, window, 0.0),
                (gap, WIDTH, math.nan, 0.0)):
        with pytest.raises(ValueError, match="must be >= 0"):
            sess.merged_event_stream_begin(*bad)
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="horizon_margin_ps"):
            sess.merged_event_stream_begin(gap, WIDTH, window, bad)
    n, f = C.c_int64(0), C.c_double(0.0)
    counts = (*([C.byref(n)] * 6), C.byref(f))
    lib = _lib.load()
    assert lib.wfa_merged_event_stream_push(sess._h, None, 0, 0.0, *counts) == _lib.WFA_E_STATE    # a push before _begin
    assert "wfa_merged_event_stream_begin first" in _lib.last_error()
    sess.merged_event_stream_begin(gap, WIDTH, window)
    try:
        out = np.zeros(4, dtype=EVENT_MERGED_HIT_DTYPE)
        idx = np.zeros(4, dtype=np.int64)
        ptrs = (out.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p))
        assert lib.wfa_merged_event_stream_fill(sess._h, *ptrs, 0, 0) == _lib.WFA_E_STATE          # before a push
        got = sess.merged_event_stream_push(a, 400_000.0)
        assert _same(got, rule.push(a, 400_000.0))
        assert lib.wfa_merged_event_stream_fill(sess._h, *ptrs, 2, 1) == _lib.WFA_E_INVALID         # other counts
        assert lib.wfa_merged_event_stream_fill(sess._h, *ptrs, 1, 2) == _lib.WFA_E_INVALID
        accepted = (len(got[0]), len(got[1]))
        assert accepted[0] <= len(out) and 0 < accepted[1] <= len(idx)
        bad = b.copy()
        bad["dt"][1] = 0                                                     # (refused by the MERGE step)
        _assert_invalid(lambda: sess.merged_event_stream_push(bad, 900_000.0), "dt must be positive")
        for c in (accepted, (0, 0)):                                         # nothing to fill after a refused push
            assert lib.wfa_merged_event_stream_fill(sess._h, *ptrs, *c) == _lib.WFA_E_STATE
        for field in ("edge_start", "edge_end"):
            bad = b.copy()
            bad[field][0] = -1
            _assert_invalid(lambda: sess.merged_event_stream_push(bad, 900_000.0), "negative edge_start / edge_end")
        bad = b.copy()
        bad["timestamp"][0] = 399_999                                        # starts below the previous horizon
        _assert_invalid(lambda: sess.merged_event_stream_push(bad, 900_000.0), "below the previous push's horizon")
        _assert_invalid(lambda: sess.merged_event_stream_push(b, 399_999.0), "lies below the previous push's")
        _assert_invalid(lambda: sess.merged_event_stream_push(b, math.nan), "NaN")
        rc = lib.wfa_merged_event_stream_push(sess._h, b.ctypes.data_as(C.c_void_p), 2**31 - 2, 900_000.0, *counts)
        assert rc == _lib.WFA_E_INVALID and "table limit" in _lib.last_error()   # carry (2) + rows = 2^31: refused unread
        # both carries and all three counters are intact: the valid pushes give what the rule gives without the refused ones
        got, want = sess.merged_event_stream_push(b, 900_000.0), rule.push(b, 900_000.0)
        assert _same(got, want) and len(got[0]) > 0 and got[1].tolist() == [1, 3, 2]
        got, want = sess.merged_event_stream_push(None, math.inf), rule.push(None, math.inf)
        assert _same(got, want) and got[2:] == (0, 0, math.inf) and got[0]["event_id"][-1] == rule.next_event - 1
    finally:
        sess.merged_event_stream_end()
    assert lib.wfa_merged_event_stream_push(sess._h, None, 0, 0.0, *counts) == _lib.WFA_E_STATE


def test_a_merged_row_below_the_previous_grouping_horizon_is_refused(sess):
    # two hits of ONE record that do not share timestamp - position * dt (no threshold hit table has such rows): the anchor
    # window of their cluster starts at 2000, below the G = 10000 the first push reported: the push is refused, not grouped
    first = E.make_hits([(0, 2000, 1, 7)])
    pair = E.make_hits([(10_000, 4000, 0, 0), (16_000, 4000, 0, 0)])
    pair["record_id"] = 9
    pair["edge_start"][0], pair["timestamp"][0] = 3, 10_000 + 7 * 2000            # abs_start still 10000, sample 3
    rule = U.NumpyMergedEventStream(2.0, WIDTH, 1.0)
    sess.merged_event_stream_begin(2.0, WIDTH, 1.0)
    try:
        got = sess.merged_event_stream_push(first, 10_000.0)
        assert _same(got, rule.push(first, 10_000.0)) and len(got[0]) == 1 and got[4] == 10_000.0
        _assert_invalid(lambda: sess.merged_event_stream_push(pair, math.inf), "below the previous push's horizon")
        lib = _lib.load()
        assert lib.wfa_merged_event_stream_fill(sess._h, None, None, 0, 0) == _lib.WFA_E_STATE      # nothing to fill
        ok = E.make_hits([(10_000, 4000, 0, 0), (16_000, 4000, 0, 0)])
        ok["record_id"] = 9
        ok["position"][1], ok["edge_start"][1], ok["edge_end"][1] = 13, 13, 15        # (timestamp - position * dt = -10000 for both)
        got, want = sess.merged_event_stream_push(ok, math.inf), rule.push(ok, math.inf)
        assert _same(got, want) and got[1].tolist() == [1, 2] and got[0]["event_id"].tolist() == [1]
    finally:
        sess.merged_event_stream_end()


def test_release_scratch_between_pushes_changes_nothing(sess, static_sess):
    case = U.fixture("merge_v1725")
    hits, cfg = case["hits"], case["configs"][2]
    horizons = E.row_horizons(hits, 500)
    rows, members, carried = [], [], []
    sess.merged_event_stream_begin(cfg["merge_gap_ns"], cfg["max_total_width_ns"], 100.0)
    try:
        for k, lo in enumerate(range(0, len(hits), 500)):
            out = sess.merged_event_stream_push(hits[lo : lo + 500], horizons[k])
            rows.append(out[0]), members.append(out[1]), carried.append(out[2:4])
            before = sess.scratch_bytes()
            assert before > 0 and sess.release_scratch() == before and sess.scratch_bytes() == 0   # the carries are not scratch
        out = sess.merged_event_stream_push(None, math.inf)
        rows.append(out[0]), members.append(out[1])
    finally:
        sess.merged_event_stream_end()
    assert max(c[0] for c in carried) > 0 and max(c[1] for c in carried) > 0
    U.assert_recorded(np.concatenate(rows), case, "g2_w100")
    assert sorted(np.concatenate(members).tolist()) == list(range(len(hits)))


def test_interleaved_with_the_merge_stream_on_one_session(sess):
    hits, _windows, _z = E.golden("grouping_v1725")
    step = 300
    horizons = E.row_horizons(hits, step)
    pushes = [(hits[lo : lo + step], horizons[k]) for k, lo in enumerate(range(0, len(hits), step))] + [(None, math.inf)]
    sess.merged_event_stream_begin(400.0, 1500.0, 100.0)
    try:
        alone_events = [sess.merged_event_stream_push(*p) for p in pushes]
    finally:
        sess.merged_event_stream_end()
    sess.merge_stream_begin(400.0, 1500.0)
    try:
        alone_merged = [sess.merge_stream_push(*p) for p in pushes]
    finally:
        sess.merge_stream_end()
    assert max(p[2] for p in alone_events) > 0 and max(p[3] for p in alone_events) > 0 and max(p[2] for p in alone_merged) > 0
    # the stream's hit_index is the component sequence hit_merged_stream delivers
    assert np.concatenate([p[1] for p in alone_events]).tolist() == np.concatenate([p[1] for p in alone_merged]).tolist()
    sess.merge_stream_begin(400.0, 1500.0)
    sess.merged_event_stream_begin(400.0, 1500.0, 100.0)
    sess.event_stream_begin(100.0)
    try:
        for k, p in enumerate(pushes):
            mg = sess.merge_stream_push(*p)
            ev = sess.merged_event_stream_push(*p)
            sess.event_stream_push(*p)
            assert _same(ev, alone_events[k]), k
            assert (mg[0].tobytes(), mg[1].tolist(), mg[2:]) == (alone_merged[k][0].tobytes(), alone_merged[k][1].tolist(),
                                                                 alone_merged[k][2:]), k
    finally:
        sess.event_stream_end()
        sess.merged_event_stream_end()
        sess.merge_stream_end()


# ---- the plugin end to end ----------------------------------------------------------------------------------------------
CONFIG = {"threshold": S.THRESHOLD, "left_extension": S.LE, "right_extension": S.RE}


@functools.cache
def _static_chain(name, gap):
    run = S.run(name)
    ctx = SimpleContext({"wave_source": "records", **CONFIG, "merge_gap_ns": gap}, {"records": run.records, "wave_pool": run.pool},
                        plugins=[HipThresholdHitPlugin(), HipHitMergeClustersPlugin(), HipHitMergePlugin(),
                                 HipHitMergedComponentsPlugin(), HipHitGroupedPlugin()])
    frame = ctx.get_data("run", "hit_grouped")
    merged, components = (ctx.get_data("run", t) for t in ("hit_merged", "hit_merged_components"))
    for t in (merged, components):
        t.setflags(write=False)
    return frame, merged, components, len(ctx.get_data("run", "hit_threshold"))


@pytest.mark.parametrize("gap", (0.0, 20.0, 400.0))
@pytest.mark.parametrize("workers", (1, 4), ids=("serial", "ring"))
@pytest.mark.parametrize("chunk_size", (1, 7, 1000))
@pytest.mark.parametrize("name", ("ragged", "mixed", "shuffled"))
def test_plugin_equals_the_static_chain(name, chunk_size, workers, gap, dp):
    run = S.run(name)
    ctx = SimpleContext({"wave_source": "records", **CONFIG, "merge_gap_ns": gap}, {"records": run.records, "wave_pool": run.pool})
    plugin = HipHitMergedGroupedStream(device_pool=dp)
    cfg = {"chunk_size": chunk_size, "parallel": workers > 1, "max_workers": workers}
    outs = list(plugin.compute(ctx, "run", streaming_config=cfg))
    frame, merged, components, n_hits = _static_chain(name, gap)
    assert len(merged) > 10 and (len(merged) < n_hits) == (gap > 0) and len(frame) > 5
    previous = -math.inf
    for o in outs:
        assert o.data.dtype == EVENT_MERGED_HIT_DTYPE and len(o.data)
        assert (o.start, o.end) == (int(o.data["t_min"].min()), int(o.data["t_max"].max()) + 1)
        assert o.metadata["first_event"] == int(o.data["event_id"][0]) and o.metadata["group_horizon"] >= previous
        previous = o.metadata["group_horizon"]
    rows = np.concatenate([o.data for o in outs])
    U.assert_frames_equal(merged_events_frame(rows), frame)
    hit_index_all = U.assert_components(outs, rows, merged, components)
    assert sorted(hit_index_all.tolist()) == list(range(n_hits))
    assert plugin.stats["pushes"] == len(run.chunks(chunk_size)) + 1 and plugin.stats["components"] == n_hits
    assert plugin.stats["rows_out"] == len(merged) and plugin.stats["events"] == len(frame)
    assert outs[-1].metadata["n_merge_carry"] == outs[-1].metadata["n_event_carry"] == 0
    if chunk_size == 1:
        assert len(outs) > 5 and plugin.stats["max_carry"] < n_hits // 4          # events leave before the end


def test_run_without_hits_gives_no_chunks(dp):
    rec = S.run("sparse").records[:120].copy()
    pool = np.full(int((rec["wave_offset"] + rec["event_length"]).max()), S.BASELINE, dtype=np.uint16)
    ctx = SimpleContext({"wave_source": "records", **CONFIG, "merge_gap_ns": 20.0}, {"records": rec, "wave_pool": pool})
    plugin = HipHitMergedGroupedStream(device_pool=dp)
    assert list(plugin.compute(ctx, "run", streaming_config={"chunk_size": 50})) == []
    assert plugin.stats["pushes"] == 4 and plugin.stats["rows_in"] == 0
