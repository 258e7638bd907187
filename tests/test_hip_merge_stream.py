"""The merge stream on the device: wfa_merge_stream_* through DeviceSession, via `static_tables`, against the static merge
pass of the same library (compute_cluster_rows / compute_merged_rows / compute_component_rows, pinned to the reference's
tables by tests/test_hip_hits.py), push by push against the numpy rule (tests/merge_stream_util.py), and
HipHitMergedStream end to end against the three static merge plugins on HipThresholdHitPlugin's rows."""

import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import event_stream_util as E
from tests import merge_stream_util as M
from tests import stream_hits_util as S
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DevicePool, DeviceSession
from waveformanalysis_amd.dtypes import HIT_MERGED_DTYPE, THRESHOLD_HIT_DTYPE
from waveformanalysis_amd.event_stream import horizon_margin, horizon_of
from waveformanalysis_amd.hit_merge import compute_cluster_rows, compute_component_rows, compute_merged_rows
from waveformanalysis_amd.merge_stream import HipHitMergedStream, merged_bounds, static_tables
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import (
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


def _static_pass(static_sess, hits, gap, width):
    """(hit_merged, hit_merge_clusters, hit_merged_components) of the static device pass over the whole table."""
    clusters = compute_cluster_rows(static_sess, hits, gap, width, None, "hit_merge_clusters")
    merged = compute_merged_rows(static_sess, hits, clusters, None, "hit_merged")
    return merged, clusters, compute_component_rows(merged, clusters)


def _assert_tables(got, want, what=None):
    for table, ref, tag in zip(got, want, ("merged", "clusters", "components")):
        assert table.dtype == ref.dtype and len(table) == len(ref), (what, tag, len(table), len(ref))
        assert table.tobytes() == ref.tobytes(), (what, tag)


def _stream(sess, gap, width, hits, chunk_size, horizons=None):
    sess.merge_stream_begin(gap, width)
    try:
        return M.stream_all(sess.merge_stream_push, hits, chunk_size, horizons)
    finally:
        sess.merge_stream_end()


# ---- the two recorded hit tables ----------------------------------------------------------------------------------------
STATIC: dict = {}


@pytest.mark.parametrize("chunk_size", (1, 3, 7, 64, "n+1"))
@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("name", M.FIXTURES)
def test_recorded_tables_equal_the_static_pass(name, k, chunk_size, sess, static_sess):
    case = M.fixture(name)
    hits = case["hits"]
    cfg = {"merge_gap_ns": 0.0, "max_total_width_ns": WIDTH, **case["configs"][k]}
    if (name, k) not in STATIC:
        STATIC[name, k] = _static_pass(static_sess, hits, cfg["merge_gap_ns"], cfg["max_total_width_ns"])
        for table, tag in zip(STATIC[name, k], ("merged", "clusters", "components")):
            table.setflags(write=False)
            assert table.tobytes() == case[f"{tag}_{k}"].tobytes()       # (and the static pass gives the recorded tables)
    merged, hit_index = _stream(sess, cfg["merge_gap_ns"], cfg["max_total_width_ns"], hits, M.chunk_size_of(chunk_size, len(hits)))
    assert merged.dtype == HIT_MERGED_DTYPE and hit_index.dtype == np.int64 and len(hit_index) == len(hits)
    _assert_tables(static_tables(merged, hit_index), STATIC[name, k], (name, k, chunk_size))


# ---- hand-made tables ---------------------------------------------------------------------------------------------------
def _push_by_push(sess, static_sess, gap, width, pushes):
    """Each (rows, horizon) push against the numpy rule -- rows, hit_index, n_carry and open_start -- and all of them,
    through static_tables, against the static pass over all pushed rows."""
    rule = M.NumpyMergeStream(gap, width)
    parts = []
    sess.merge_stream_begin(gap, width)
    try:
        for k, (rows, horizon) in enumerate(pushes):
            got = sess.merge_stream_push(rows, horizon)
            want = rule.push(rows, horizon)
            assert got[0].tobytes() == want[0].tobytes(), (k, got[0], want[0])
            assert got[1].tolist() == want[1].tolist() and got[2:] == want[2:], (k, got[1:], want[1:])
            parts.append(got)
    finally:
        sess.merge_stream_end()
    assert parts[-1][2] == 0
    table = np.concatenate([r for r, _h in pushes if r is not None and len(r)])
    got = static_tables(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    _assert_tables(got, _static_pass(static_sess, table, gap, width))
    return parts


def test_cluster_open_across_three_pushes(sess, static_sess):
    a = E.make_hits([(1_000_000, 4000, 0, 0), (1_001_000, 4000, 0, 1)])
    b = E.make_hits([(1_050_000, 4000, 0, 0), (1_300_000, 4000, 0, 1)])
    c = E.make_hits([(1_120_000, 4000, 0, 0), (2_000_000, 4000, 0, 0)])
    for t, base in ((b, 2), (c, 4)):
        t["record_id"] += base
    parts = _push_by_push(sess, static_sess, 100.0, WIDTH, [(a, 1_050_000.0), (b, 1_120_000.0), (c, 2_000_000.0),
                                                            (None, math.inf)])
    # channel 0's cluster takes a hit of every push and leaves with the third; channel 1's first hit leaves with the second
    assert [len(p[0]) for p in parts] == [0, 1, 2, 1] and [p[2] for p in parts] == [2, 3, 1, 0]
    assert parts[2][0]["component_count"].tolist() == [3, 1] and parts[2][1].tolist() == [0, 2, 4, 3]
    assert [p[3] for p in parts] == [1_000_000.0, 1_000_000.0, 2_000_000.0, math.inf]


def test_push_without_rows_in_the_middle(sess, static_sess):
    a = E.make_hits([(1000, 4000, 0, 0), (500_000, 4000, 0, 1)])
    b = E.make_hits([(900_000, 4000, 0, 0)])
    b["record_id"] += 2
    empty = np.zeros(0, dtype=THRESHOLD_HIT_DTYPE)
    parts = _push_by_push(sess, static_sess, 100.0, WIDTH, [(a, 500_000.0), (empty, 700_000.0), (None, 900_000.0),
                                                            (b, 900_000.0), (None, math.inf)])
    assert [len(p[0]) for p in parts] == [1, 1, 0, 0, 1]


def test_horizon_boundary_is_strict(sess, static_sess):
    # gap 10 ns: [0, 4000] and [9000, 13000] chain; H - cluster_end == gap_ps holds the cluster, 1000 ps more closes it
    hits = E.make_hits([(0, 4000, 0, 0), (9000, 4000, 0, 0)])
    parts = _push_by_push(sess, static_sess, 10.0, WIDTH, [(hits, 23_000.0), (None, 24_000.0), (None, math.inf)])
    assert [len(p[0]) for p in parts] == [0, 1, 0] and parts[0][2:] == (2, 0.0) and parts[1][1].tolist() == [0, 1]
    # and a later hit at abs_start == H == cluster_end + gap does join
    late = E.make_hits([(23_000, 2000, 0, 0)])
    late["record_id"] += 2
    parts = _push_by_push(sess, static_sess, 10.0, WIDTH, [(hits, 23_000.0), (late, math.inf)])
    assert [len(p[0]) for p in parts] == [0, 1] and parts[1][0]["component_count"].tolist() == [3]


def test_a_row_at_the_horizon_is_not_final(sess, static_sess):
    # gap 100 ns: the chain breaks at the second hit (another dt), but that hit starts AT the horizon: rule 1 needs b < F,
    # and rule 3 fails because H - cluster_end = 46 ns is within the gap
    far = E.make_hits([(0, 4000, 0, 0, 2), (50_000, 4000, 0, 0, 4)])
    parts = _push_by_push(sess, static_sess, 100.0, WIDTH, [(far, 50_000.0), (None, math.inf)])
    assert [len(p[0]) for p in parts] == [0, 2] and parts[0][2:] == (2, 0.0)
    # one ps more and the second hit is final: the first cluster closes by rule 1, the second waits
    parts = _push_by_push(sess, static_sess, 100.0, WIDTH, [(far, 50_001.0), (None, math.inf)])
    assert [len(p[0]) for p in parts] == [1, 1] and parts[0][2:] == (1, 50_000.0)


def test_width_cap_dt_change_and_two_boards(sess, static_sess):
    # within the gap (100 ns) but over the cap (10 ns): [0, 4000] + [8000, 12000] would be 12 ns wide
    capped = E.make_hits([(0, 4000, 0, 0), (8000, 4000, 0, 0), (10_000, 2000, 0, 0), (900_000, 4000, 0, 0)])
    parts = _push_by_push(sess, static_sess, 100.0, 10.0, [(capped[:2], 10_000.0), (capped[2:], math.inf)])
    assert np.concatenate([p[0] for p in parts])["component_count"].tolist() == [1, 2, 1]
    assert [len(p[0]) for p in parts] == [1, 3 - 1]           # the cap closes the first cluster by rule 1 at once
    # a dt change inside a channel breaks the chain, whatever the gap
    mixed = E.make_hits([(0, 4000, 0, 0, 2), (6000, 4000, 0, 0, 4), (12_000, 4000, 0, 0, 4), (20_000, 4000, 0, 0, 2)])
    parts = _push_by_push(sess, static_sess, 100.0, WIDTH, [(mixed[:3], 20_000.0), (mixed[3:], math.inf)])
    assert np.concatenate([p[0] for p in parts])["component_count"].tolist() == [1, 2, 1]
    assert np.concatenate([p[0] for p in parts])["dt"].tolist() == [2, 4, 2]
    # the same channel number on two boards: two channels, ordered by board first
    boards = E.make_hits([(0, 4000, 1, 3), (2000, 4000, 0, 3), (5000, 4000, 1, 3), (7000, 4000, 0, 3), (9000, 4000, 0, 2)])
    parts = _push_by_push(sess, static_sess, 20.0, WIDTH, [(boards[:2], 5000.0), (boards[2:], math.inf)])
    rows = parts[1][0]
    assert (rows["board"].tolist(), rows["channel"].tolist()) == ([0, 0, 1], [2, 3, 3])
    assert rows["component_count"].tolist() == [1, 2, 2] and parts[1][1].tolist() == [4, 1, 3, 0, 2]


def test_record_span_height_tie_and_single_hit_rows(sess, static_sess):
    # two hits of one record: window = (min start, max end), width from it; two records: -1, -1 and width -1
    hits = E.make_hits([(0, 4000, 0, 0), (6000, 8000, 0, 0), (500_000, 4000, 0, 0), (506_000, 4000, 0, 0),
                        (900_000, 6000, 0, 0)])
    hits["record_id"] = [7, 7, 8, 9, 9]
    hits["edge_start"][1] = 4      # (and abs_start with it: 6000 -> ts + (4 - 10) * 2000)
    hits["timestamp"][1] += 12_000
    hits["width"] = [1.5, 2.5, 3.5, 4.5, 5.5]
    hits["integral"] = [0.1, 0.2, 0.3, 0.4, 0.5]
    parts = _push_by_push(sess, static_sess, 20.0, WIDTH, [(hits[:3], 506_000.0), (hits[3:], math.inf)])
    rows = np.concatenate([p[0] for p in parts])
    assert rows["component_count"].tolist() == [2, 2, 1]
    assert (rows["sample_start"].tolist(), rows["sample_end"].tolist()) == ([4, -1, 10], [14, -1, 13])
    assert rows["width"].tolist() == [10.0, -1.0, 5.5]          # the single hit keeps its own width, not end - start
    assert rows["integral"].tolist() == [np.float32(np.float64(np.float32(0.1)) + np.float64(np.float32(0.2))),
                                         np.float32(np.float64(np.float32(0.3)) + np.float64(np.float32(0.4))),
                                         np.float32(0.5)]
    # equal heights: the anchor is the member with the smaller timestamp, here the LATER one in chain order
    tie = E.make_hits([(100_000, 4000, 0, 0), (106_000, 4000, 0, 0), (112_000, 4000, 0, 0)])
    tie["height"] = [5.0, 9.0, 9.0]
    tie["position"][2], tie["timestamp"][2] = 80, 112_000 - (10 - 80) * 2000      # same abs_start, another anchor sample
    tie["timestamp"][1] += 1_000_000                                               # ... and the second member's is larger
    tie["position"][1] = 10 + 500
    assert E.windows_of(tie)[0].tolist() == [100_000.0, 106_000.0, 112_000.0]
    parts = _push_by_push(sess, static_sess, 20.0, WIDTH, [(tie[:2], 112_000.0), (tie[2:], math.inf)])
    row = parts[1][0]
    assert len(row) == 1 and row["component_count"][0] == 3 and row["height"][0] == 9.0
    assert (int(row["timestamp"][0]), int(row["position"][0]), int(row["record_id"][0])) == (int(tie["timestamp"][2]), 80, 2)


def test_gap_zero_every_hit_is_its_own_row(sess, static_sess):
    rng = np.random.default_rng(5)
    hits = E.make_hits([(int(t), 4000, 0, int(c)) for t, c in zip(np.sort(rng.integers(0, 60_000, 40)), rng.integers(0, 3, 40))])
    hits["width"] = rng.random(40).astype(np.float32)
    horizons = E.row_horizons(hits, 8)
    parts = _push_by_push(sess, static_sess, 0.0, WIDTH, [(hits[lo : lo + 8], horizons[k]) for k, lo in enumerate(range(0, 40, 8))]
                          + [(None, math.inf)])
    rows = np.concatenate([p[0] for p in parts])
    assert len(rows) == 40 and set(rows["component_count"].tolist()) == {1}
    assert sum(len(p[0]) for p in parts[:-2]) > 0                # rows leave as soon as they are final


def test_timestamps_at_2_to_60_with_rounding_windows(sess, static_sess):
    # one ulp is 256 ps; dt = 3 ns and odd record timestamps make float(ts), the product and the sum all round
    rng = np.random.default_rng(11)
    n_rec = 16
    rec_ts = 2**60 + np.arange(n_rec, dtype=np.int64) * 1_000_003 + rng.integers(0, 255, n_rec)
    hits = np.zeros(2 * n_rec, dtype=THRESHOLD_HIT_DTYPE)
    for i in range(2 * n_rec):
        r = i // 2
        pos = int(rng.integers(3, 60))
        start = 0 if i % 2 == 0 else int(rng.integers(0, pos + 1))
        hits[i] = (pos, float(i), 1.0, start, pos + int(rng.integers(1, 9)), 0.0, 3, 0.0, 0.0, int(rec_ts[r]) + pos * 3000,
                   0, i % 3, r)
    margin = horizon_margin(int(rec_ts.max()) + 3 * 1000 * 80)
    assert margin == 512.0
    pushes = []
    for lo in range(0, n_rec, 4):                                          # four records (eight hits) per push
        later = int(rec_ts[lo + 4:].min()) if lo + 4 < n_rec else None
        pushes.append((hits[2 * lo : 2 * lo + 8], horizon_of(later, margin)))
    for gap in (30.0, 900.0):                                              # (900 ns reaches into the next record)
        parts = _push_by_push(sess, static_sess, gap, 1e9, pushes + [(None, math.inf)])
        assert sum(len(p[0]) for p in parts[:-2]) > 0                      # clusters did close before the last records
        assert max(p[2] for p in parts) > 0 or gap == 30.0                 # ... and with the wide gap some waited
    assert any(c > 1 for c in np.concatenate([p[0] for p in parts])["component_count"])


# ---- sizes at block edges -----------------------------------------------------------------------------------------------
def test_257_single_hit_clusters(sess, static_sess):
    # 257 clusters / 257 rows: a last thread block of one cluster and one row; 257 * 18 dwords end inside a block
    hits = E.make_hits([(1_000_000 * i, 4000, 0, i % 5) for i in range(257)])
    parts = _push_by_push(sess, static_sess, 20.0, WIDTH, [(hits, math.inf)])
    assert len(parts[0][0]) == 257 and sorted(parts[0][1].tolist()) == list(range(257))
    # gap 2 us, hits of a channel 5 us apart: nothing merges, the hits that end within the gap of the horizon wait
    parts = _push_by_push(sess, static_sess, 2000.0, WIDTH, [(hits[:256], float(1_000_000 * 256)), (hits[256:], math.inf)])
    assert [len(p[0]) for p in parts] == [254, 3] and parts[0][2:] == (2, 254_000_000.0)


def test_65537_rows_in_three_pushes(sess, static_sess):
    rng = np.random.default_rng(17)
    n = 65_537
    start = np.sort(rng.integers(0, 6 * n, n)) * 2000
    hits = np.zeros(n, dtype=THRESHOLD_HIT_DTYPE)
    hits["position"] = rng.integers(4, 40, n)
    hits["edge_start"] = hits["position"] - rng.integers(0, 4, n)
    hits["edge_end"] = hits["position"] + rng.integers(1, 6, n)
    hits["dt"] = 2
    hits["timestamp"] = start + (hits["position"] - hits["edge_start"]) * 2000
    hits["channel"] = rng.integers(0, 16, n)
    hits["board"] = rng.integers(0, 2, n)
    hits["record_id"] = np.arange(n) // 3
    hits["height"] = rng.integers(1, 50, n)
    hits["integral"] = rng.random(n)
    hits["width"] = rng.random(n)
    gap = 600.0
    want = _static_pass(static_sess, hits, gap, 5000.0)
    assert 2 < len(hits) / len(want[0]) < 20 and want[0]["component_count"].max() > 8
    sess.merge_stream_begin(gap, 5000.0)
    try:
        rows, members, carried = [], [], []
        horizons = E.row_horizons(hits, 30_000)
        for k, lo in enumerate(range(0, n, 30_000)):
            out = sess.merge_stream_push(hits[lo : lo + 30_000], horizons[k])
            rows.append(out[0]), members.append(out[1]), carried.append(out[2])
        assert carried[-1] == 0 and min(carried[:-1]) > 0 and len(rows) == 3
    finally:
        sess.merge_stream_end()
    _assert_tables(static_tables(np.concatenate(rows), np.concatenate(members)), want)


# ---- refusals, scratch, two streams on one session ----------------------------------------------------------------------
def _assert_invalid(call, match):
    with pytest.raises(ValueError, match=match):
        call()


def test_refusals_leave_the_stream_untouched(sess):
    a = E.make_hits([(1000, 4000, 0, 0), (400_000, 4000, 0, 1), (402_000, 4000, 0, 2)])
    b = E.make_hits([(404_000, 4000, 0, 1), (900_000, 4000, 0, 1)])
    b["record_id"] += 3
    gap = 100.0
    rule = M.NumpyMergeStream(gap, WIDTH)
    for bad in ((-1.0, WIDTH), (gap, -1.0), (math.nan, WIDTH), (gap, math.nan)):
        with pytest.raises(ValueError, match="must be >= 0"):
            sess.merge_stream_begin(*bad)
    n, f = C.c_int64(0), C.c_double(0.0)
    counts = (C.byref(n), C.byref(n), C.byref(n), C.byref(f))
    lib = _lib.load()
    assert lib.wfa_merge_stream_push(sess._h, None, 0, 0.0, *counts) == _lib.WFA_E_STATE       # (a refused _begin opens nothing)
    sess.merge_stream_begin(gap, WIDTH)
    try:
        out = np.zeros(4, dtype=HIT_MERGED_DTYPE)
        idx = np.zeros(4, dtype=np.int64)
        ptrs = (out.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p))
        assert lib.wfa_merge_stream_fill(sess._h, *ptrs, 0, 0) == _lib.WFA_E_STATE             # before a push
        got, want = sess.merge_stream_push(a, 400_000.0), rule.push(a, 400_000.0)
        assert (got[0].tobytes(), got[1].tolist(), got[2:]) == (want[0].tobytes(), want[1].tolist(), want[2:])
        assert got[2:] == (2, 400_000.0)
        assert lib.wfa_merge_stream_fill(sess._h, *ptrs, 2, 1) == _lib.WFA_E_INVALID            # other counts
        accepted = (len(got[0]), len(got[1]))
        assert 0 < accepted[0] <= len(out) and 0 < accepted[1] <= len(idx)

        def nothing_to_fill():      # after a refused push: not with the last accepted push's counts, not with 0
            return all(lib.wfa_merge_stream_fill(sess._h, *ptrs, *c) == _lib.WFA_E_STATE for c in (accepted, (0, 0)))

        bad = b.copy()
        bad["dt"][1] = 0
        _assert_invalid(lambda: sess.merge_stream_push(bad, 900_000.0), "dt must be positive")
        assert nothing_to_fill()
        for field in ("edge_start", "edge_end"):
            bad = b.copy()
            bad[field][0] = -1
            _assert_invalid(lambda: sess.merge_stream_push(bad, 900_000.0), "negative edge_start / edge_end")
            assert nothing_to_fill()
        bad = b.copy()
        bad["timestamp"][0] = 399_999                                        # starts below the previous horizon
        _assert_invalid(lambda: sess.merge_stream_push(bad, 900_000.0), "below the previous push's horizon")
        assert nothing_to_fill()
        _assert_invalid(lambda: sess.merge_stream_push(b, 399_999.0), "lies below the previous push's")
        assert nothing_to_fill()
        _assert_invalid(lambda: sess.merge_stream_push(b, math.nan), "NaN")
        assert nothing_to_fill()
        rc = lib.wfa_merge_stream_push(sess._h, b.ctypes.data_as(C.c_void_p), 2**31 - 2, 900_000.0, *counts)
        assert rc == _lib.WFA_E_INVALID and "table limit" in _lib.last_error()   # carry (2) + rows = 2^31: refused unread
        assert nothing_to_fill()
        # carry, hit and component counters are intact: the valid push gives what the rule gives without the refused ones
        got, want = sess.merge_stream_push(b, 900_000.0), rule.push(b, 900_000.0)
        assert (got[0].tobytes(), got[1].tolist(), got[2:]) == (want[0].tobytes(), want[1].tolist(), want[2:])
        assert got[1].tolist() == [1, 3, 2] and got[0]["component_offset"].tolist() == [1, 3] and got[2:] == (1, 900_000.0)
        got, want = sess.merge_stream_push(None, math.inf), rule.push(None, math.inf)
        assert (got[0].tobytes(), got[1].tolist(), got[2:]) == (want[0].tobytes(), [4], (0, math.inf))
    finally:
        sess.merge_stream_end()
    assert lib.wfa_merge_stream_push(sess._h, None, 0, 0.0, *counts) == _lib.WFA_E_STATE


def test_release_scratch_between_pushes_changes_nothing(sess, static_sess):
    case = M.fixture("merge_v1725")
    hits, cfg = case["hits"], case["configs"][2]
    horizons = E.row_horizons(hits, 500)
    rows, members, carried = [], [], []
    sess.merge_stream_begin(cfg["merge_gap_ns"], cfg["max_total_width_ns"])
    try:
        for k, lo in enumerate(range(0, len(hits), 500)):
            out = sess.merge_stream_push(hits[lo : lo + 500], horizons[k])
            rows.append(out[0]), members.append(out[1]), carried.append(out[2])
            before = sess.scratch_bytes()
            assert before > 0 and sess.release_scratch() == before and sess.scratch_bytes() == 0   # the carry is not scratch
        out = sess.merge_stream_push(None, math.inf)
        rows.append(out[0]), members.append(out[1])
    finally:
        sess.merge_stream_end()
    assert max(carried) > 0
    got = static_tables(np.concatenate(rows), np.concatenate(members))
    for table, tag in zip(got, ("merged", "clusters", "components")):
        assert table.tobytes() == case[f"{tag}_2"].tobytes()


def test_event_stream_and_merge_stream_interleaved_on_one_session(sess):
    hits, _windows, _z = E.golden("grouping_v1725")
    step = 300
    horizons = E.row_horizons(hits, step)
    alone_events = []
    sess.event_stream_begin(100.0)
    try:
        alone_events = [sess.event_stream_push(hits[lo : lo + step], horizons[k]) for k, lo in enumerate(range(0, len(hits), step))]
        alone_events.append(sess.event_stream_push(None, math.inf))
    finally:
        sess.event_stream_end()
    alone_merged = []
    sess.merge_stream_begin(400.0, 1500.0)
    try:
        alone_merged = [sess.merge_stream_push(hits[lo : lo + step], horizons[k]) for k, lo in enumerate(range(0, len(hits), step))]
        alone_merged.append(sess.merge_stream_push(None, math.inf))
    finally:
        sess.merge_stream_end()
    assert max(p[1] for p in alone_events) > 0 and max(p[2] for p in alone_merged) > 0     # both carry between pushes
    sess.event_stream_begin(100.0)
    sess.merge_stream_begin(400.0, 1500.0)
    try:
        for k, lo in enumerate(list(range(0, len(hits), step)) + [None]):
            rows, horizon = (None, math.inf) if lo is None else (hits[lo : lo + step], horizons[k])
            ev = sess.event_stream_push(rows, horizon)
            mg = sess.merge_stream_push(rows, horizon)
            assert (ev[0].tobytes(), ev[1]) == (alone_events[k][0].tobytes(), alone_events[k][1]), k
            assert (mg[0].tobytes(), mg[1].tolist(), mg[2:]) == (alone_merged[k][0].tobytes(), alone_merged[k][1].tolist(),
                                                                 alone_merged[k][2:]), k
    finally:
        sess.merge_stream_end()
        sess.event_stream_end()


# ---- the plugin end to end ----------------------------------------------------------------------------------------------
CONFIG = {"threshold": S.THRESHOLD, "left_extension": S.LE, "right_extension": S.RE}


@functools.cache
def _static_chain(name, gap):
    run = S.run(name)
    ctx = SimpleContext({"wave_source": "records", **CONFIG, "merge_gap_ns": gap}, {"records": run.records, "wave_pool": run.pool},
                        plugins=[HipThresholdHitPlugin(), HipHitMergeClustersPlugin(), HipHitMergePlugin(),
                                 HipHitMergedComponentsPlugin()])
    tables = tuple(ctx.get_data("run", name) for name in ("hit_merged", "hit_merge_clusters", "hit_merged_components"))
    for t in tables:
        t.setflags(write=False)
    return tables


@pytest.mark.parametrize("gap", (0.0, 20.0, 400.0))
@pytest.mark.parametrize("workers", (1, 4), ids=("serial", "ring"))
@pytest.mark.parametrize("chunk_size", (1, 7, 1000))
@pytest.mark.parametrize("name", ("ragged", "mixed", "shuffled"))
def test_plugin_equals_the_static_chain(name, chunk_size, workers, gap, dp):
    run = S.run(name)
    ctx = SimpleContext({"wave_source": "records", **CONFIG, "merge_gap_ns": gap}, {"records": run.records, "wave_pool": run.pool})
    plugin = HipHitMergedStream(device_pool=dp)
    cfg = {"chunk_size": chunk_size, "parallel": workers > 1, "max_workers": workers}
    outs = list(plugin.compute(ctx, "run", streaming_config=cfg))
    first = 0
    for o in outs:
        assert o.data.dtype == HIT_MERGED_DTYPE and len(o.data) and (o.start, o.end) == merged_bounds(o.data)
        assert o.metadata["first_component"] == first and o.metadata["hit_index"].dtype == np.int64
        first += len(o.metadata["hit_index"])
    merged = np.concatenate([o.data for o in outs])
    hit_index = np.concatenate([o.metadata["hit_index"] for o in outs])
    want = _static_chain(name, gap)
    assert len(want[0]) > 10 and (len(want[0]) < len(want[1])) == (gap > 0)
    _assert_tables(static_tables(merged, hit_index), want, (name, chunk_size, workers, gap))
    assert plugin.stats["pushes"] == len(run.chunks(chunk_size)) + 1 and plugin.stats["components"] == len(want[1])
    assert outs[-1].metadata["n_carry"] == 0 and outs[-1].metadata["open_start"] == math.inf
    if chunk_size == 1:
        assert len(outs) > 10 and plugin.stats["max_carry"] < len(hit_index) // 4    # rows leave as their clusters close


def test_run_without_hits_gives_no_chunks(dp):
    rec = S.run("sparse").records[:120].copy()
    pool = np.full(int((rec["wave_offset"] + rec["event_length"]).max()), S.BASELINE, dtype=np.uint16)
    ctx = SimpleContext({"wave_source": "records", **CONFIG, "merge_gap_ns": 20.0}, {"records": rec, "wave_pool": pool})
    plugin = HipHitMergedStream(device_pool=dp)
    assert list(plugin.compute(ctx, "run", streaming_config={"chunk_size": 50})) == []
    assert plugin.stats["pushes"] == 4 and plugin.stats["rows_in"] == 0
