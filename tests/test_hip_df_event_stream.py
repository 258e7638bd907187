"""The df_events stream on the device: wfa_df_event_stream_* through DeviceSession against the frames the reference
recorded, the static device pass of the same library (group_multi_channel) and, push by push, the numpy rule
(tests/df_event_stream_util.py); HipBasicFeaturesStream and HipGroupedEventsStream end to end against the static
basic_features / df / df_events / df_paired plugins on the same Context."""

import ctypes as C
import functools

import numpy as np
import pytest

from tests import df_event_stream_util as D
from tests import event_stream_util as ES
from tests import events_util as E
from tests import stream_hits_util as S
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DevicePool, DeviceSession
from waveformanalysis_amd.df_event_stream import HipGroupedEventsStream, grouped_events_frame, paired_events_frame
from waveformanalysis_amd.dtypes import BASIC_FEATURES_DTYPE, DF_EVENT_ROW_DTYPE, DF_ROW_DTYPE
from waveformanalysis_amd.event_grouping import group_hit_windows_flat
from waveformanalysis_amd.event_stream import event_rows
from waveformanalysis_amd.features_stream import HipBasicFeaturesStream
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import (
    HipBasicFeaturesPlugin,
    HipDataFramePlugin,
    HipGroupedEventsPlugin,
    HipPairedEventsPlugin,
)

pytestmark = pytest.mark.gpu
END = D.HORIZON_END
Z = D.fixture()


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


def _static(static_sess, rows, window_ns):
    """Rows of the static device pass over the whole table; the host pass agrees."""
    if len(rows) == 0:
        return np.zeros(0, dtype=DF_EVENT_ROW_DTYPE)
    order, bounds = static_sess.group_multi_channel(rows["timestamp"], rows["channel"], float(window_ns) * 1e3)
    out = D.rows_of(rows, order, bounds)
    assert out.tobytes() == D.static_rows(rows, window_ns).tobytes()
    return out


def _stream(sess, window_ns, rows, chunk_size):
    sess.df_event_stream_begin(window_ns)
    try:
        return D.stream_rows(sess.df_event_stream_push, rows, chunk_size)
    finally:
        sess.df_event_stream_end()


def _push_by_push(sess, static_sess, window_ns, pushes):
    """Each (rows, horizon, final) push against the numpy rule, all rows against the static pass over all pushed rows."""
    rule = D.NumpyDfStream(window_ns)
    parts, carries = [], []
    sess.df_event_stream_begin(window_ns)
    try:
        for k, (rows, horizon, final) in enumerate(pushes):
            got, carry = sess.df_event_stream_push(rows, horizon, final)
            want, want_carry = rule.push(rows, horizon, final)
            assert got.dtype == DF_EVENT_ROW_DTYPE
            assert (got.tobytes(), carry) == (want.tobytes(), want_carry), (k, len(got), len(want), carry, want_carry)
            parts.append(got)
            carries.append(carry)
    finally:
        sess.df_event_stream_end()
    table = np.concatenate([r for r, _h, _f in pushes if r is not None and len(r)])
    assert np.concatenate(parts).tobytes() == _static(static_sess, table, window_ns).tobytes()
    return parts, carries


# ---- the recorded frames ------------------------------------------------------------------------------------------------
@functools.cache
def _fixture_static(case):
    rows, window_ns = D.fixture_rows(Z, case)
    with DeviceSession(0) as s:
        want = _static(s, rows, window_ns)
    want.setflags(write=False)
    return rows, window_ns, want


@pytest.mark.parametrize("chunk_size", (1, 3, 7, 64, "n+1"))
@pytest.mark.parametrize("case", D.FIXTURE_CASES)
def test_fixture_cases_equal_the_recorded_frames_and_the_static_pass(case, chunk_size, sess):
    rows, window_ns, want = _fixture_static(case)
    got = _stream(sess, window_ns, rows, len(rows) + 1 if chunk_size == "n+1" else chunk_size)
    assert got.dtype == DF_EVENT_ROW_DTYPE and len(got) == len(rows)
    assert got.tobytes() == want.tobytes()
    E.assert_frame_matches(grouped_events_frame(got), Z, f"{case}/df_events")
    E.assert_frame_matches(paired_events_frame(got, **D.pairing_args(Z, case)), Z, f"{case}/df_paired")


# ---- crafted tables -----------------------------------------------------------------------------------------------------
def _rows(ts, ch, first_id=0):
    out = D.make_rows(np.asarray(ts, dtype=np.int64), ch)
    out["record_id"] += first_id
    out["area"] += first_id
    return out


def test_event_open_across_three_pushes(sess, static_sess):
    a = _rows([1_000_000, 1_002_000], [3, 1])
    b = _rows([1_050_000, 1_080_000], [2, 1], 2)
    c = _rows([1_100_000, 2_000_000], [0, 0], 4)              # 1_100_000 == anchor + window: still inside
    parts, carries = _push_by_push(sess, static_sess, 100.0, [(a, 1_050_000, False), (b, 1_100_000, False), (c, END, True)])
    assert [len(p) for p in parts] == [0, 0, 6] and carries == [2, 4, 0]
    assert parts[2]["event_id"].tolist() == [0] * 5 + [1] and parts[2]["n_hits"].tolist() == [5] * 5 + [1]


def test_middle_push_without_rows_and_a_push_that_closes_nothing(sess, static_sess):
    a = _rows([1000, 500_000], [0, 1])
    b = _rows([900_000], [0], 2)
    empty = np.zeros(0, dtype=DF_ROW_DTYPE)
    parts, carries = _push_by_push(sess, static_sess, 100.0, [(a, 500_000, False), (empty, 550_000, False),
                                                              (None, 700_000, False), (None, 700_000, False),
                                                              (b, 900_000, False), (None, END, True)])
    assert [len(p) for p in parts] == [1, 0, 1, 0, 0, 1] and carries == [1, 1, 0, 0, 1, 0]


def test_horizon_boundary_is_strict(sess, static_sess):
    a = _rows([900], [0])
    b = _rows([100_900, 300_000], [1, 0], 1)
    # (double)H == (double)a + w: held back, and the later row at H joins the event
    parts, _ = _push_by_push(sess, static_sess, 100.0, [(a, 100_900, False), (b, END, True)])
    assert [len(p) for p in parts] == [0, 3] and parts[1]["event_id"].tolist() == [0, 0, 1]
    # one more (below 2^53 one ps is more than one ulp of the sum): the event closes
    b["timestamp"][0] = 100_901
    parts, _ = _push_by_push(sess, static_sess, 100.0, [(a, 100_901, False), (b, END, True)])
    assert [len(p) for p in parts] == [1, 2] and parts[1]["event_id"].tolist() == [1, 2]
    # at 2^60 one ulp is 256 ps: the next double above a + w closes, everything that rounds to a + w does not
    base = 2**60
    assert float(base) + 1e5 == float(base + 100_096) == float(base + 100_223) < float(base + 100_224)
    a = _rows([base], [0])
    for h, closes in ((base + 100_096, False), (base + 100_223, False), (base + 100_224, True)):
        b = _rows([h, base + 10**7], [1, 0], 1)
        parts, _ = _push_by_push(sess, static_sess, 100.0, [(a, h, False), (b, END, True)])
        assert [len(p) for p in parts] == ([1, 2] if closes else [0, 3]), h


def test_window_zero_with_equal_timestamps_on_both_sides_of_a_push(sess, static_sess):
    a = _rows([5000, 7000, 7000], [2, 3, 1])
    b = _rows([7000, 7000, 9000], [2, 0, 0], 3)
    parts, carries = _push_by_push(sess, static_sess, 0.0, [(a, 7000, False), (b, END, True)])
    assert [len(p) for p in parts] == [1, 5] and carries == [2, 0]
    assert parts[1]["channel"].tolist() == [0, 1, 2, 3, 0] and parts[1]["n_hits"].tolist() == [4] * 4 + [1]


def test_equal_channels_inside_an_event_keep_row_order_across_a_push(sess, static_sess):
    # equal timestamps AND equal channels: only the stable order tells the rows apart (record_id = row index)
    a = _rows([1000, 1000, 1000], [1, 1, 0])
    b = _rows([1000, 1000, 1050, 900_000], [1, 0, 1, 1], 3)
    parts, _ = _push_by_push(sess, static_sess, 100.0, [(a, 1000, False), (b, END, True)])
    assert parts[1]["record_id"].tolist() == [2, 4, 0, 1, 3, 5, 6]
    # the same across three pushes with the carry in front every time
    c = _rows([1000, 2_000_000], [1, 0], 7)
    b2 = b[:3]
    parts, _ = _push_by_push(sess, static_sess, 100.0, [(a, 1000, False), (b2, 1000, False), (c, END, True)])
    assert parts[2]["record_id"].tolist() == [2, 4, 0, 1, 3, 7, 5, 8]


def test_t_min_and_t_max_are_not_the_extremes(sess, static_sess):
    a = _rows([1000, 900, 1100], [3, 5, 1])
    b = _rows([950, 500_000], [4, 0], 3)
    parts, _ = _push_by_push(sess, static_sess, 100.0, [(a, 950, False), (b, END, True)])
    ev = parts[1][:4]
    assert ev["channel"].tolist() == [1, 3, 4, 5] and ev["timestamp"].tolist() == [1100, 1000, 950, 900]
    assert set(ev["t_min"]) == {1100} and set(ev["t_max"]) == {900}          # first / last row after the channel sort


def test_two_timestamps_with_one_double_form_one_event_across_a_push(sess, static_sess):
    base = 2**60
    assert float(base) == float(base + 1)
    a, b = _rows([base], [1]), _rows([base + 1, base + 10**6], [0, 0], 1)
    parts, carries = _push_by_push(sess, static_sess, 0.0, [(a, base + 1, False), (b, END, True)])
    assert [len(p) for p in parts] == [0, 3] and carries == [1, 0]
    assert parts[1]["event_id"].tolist() == [0, 0, 1] and parts[1]["timestamp"].tolist() == [base + 1, base, base + 10**6]


@pytest.mark.parametrize("anchor,rounds", ((2**60, "up"), (2**60 + 100, "down")))
def test_float_rounding_of_the_window_sum(anchor, rounds, sess, static_sess):
    """(double)a + w against the exact integer a + w, 100 ns at 2^60 (one ulp = 256 ps)."""
    w = 100_000
    needle = int(float(anchor) + float(w))
    assert needle == 2**60 + 100_096
    if rounds == "up":       # the float window is wider than the integer one: a row 50 ps past a + w still joins
        assert needle > anchor + w
        late = anchor + w + 50
        assert late > anchor + w and float(late) <= float(anchor) + float(w)
    else:                    # the float sum ends before a + w does, and float(row) rounds down with it: the row joins
        assert needle < anchor + w
        late = anchor + w - 2
        assert needle < late <= anchor + w and float(late) <= float(anchor) + float(w)
    a = _rows([anchor], [1])
    b = _rows([late, 2**60 + 100_224, 2**60 + 10**7], [0, 0, 0], 1)
    assert float(b["timestamp"][1]) > float(anchor) + float(w)         # the next double: outside
    # H = the late row: (double)H == (double)a + w holds the event back, and the row joins it in the next push
    parts, carries = _push_by_push(sess, static_sess, 100.0, [(a, late, False), (b, END, True)])
    assert carries == [1, 0]
    assert parts[1]["event_id"].tolist() == [0, 0, 1, 2] and parts[1]["record_id"].tolist() == [1, 0, 2, 3]


# ---- size edges ---------------------------------------------------------------------------------------------------------
def _random_rows(n, seed):
    rng = np.random.default_rng(seed)
    ts = 10**9 + np.cumsum(rng.choice([0, 1000, 40_000, 300_000], n)).astype(np.int64)
    return D.make_rows(ts, rng.integers(0, 16, n))


@pytest.mark.parametrize("size", (1, 255, 256, 257, 1023, 1024, 1025))
def test_table_sizes_around_the_block(size, sess, static_sess):
    rows = _random_rows(size, size)
    n_carry = size // 3
    first = int(rows["timestamp"].min())
    # a horizon at the table's first timestamp closes nothing: the carry is exactly the first push
    pushes = [(rows[:n_carry], first, False), (rows[n_carry:], END, True)]
    parts, carries = _push_by_push(sess, static_sess, 100.0, pushes)
    assert carries == [n_carry, 0] and [len(p) for p in parts] == [0, size]
    assert _stream(sess, 100.0, rows, 100).tobytes() == np.concatenate(parts).tobytes()


def test_one_event_of_300_rows_straddles_a_block(sess, static_sess):
    rng = np.random.default_rng(5)
    before, after = _random_rows(200, 1), _random_rows(150, 2)
    t0 = int(before["timestamp"].max()) + 10**6
    big = D.make_rows(t0 + np.sort(rng.integers(0, 90_000, 300)), rng.integers(0, 16, 300))
    big["timestamp"][0] = t0
    after["timestamp"] += t0 + 10**6 - int(after["timestamp"].min())
    rows = np.concatenate([before, big, after])
    rows["record_id"] = np.arange(len(rows))
    want = _static(static_sess, rows, 100.0)
    assert int(want["n_hits"].max()) == 300
    at = np.flatnonzero(want["n_hits"] == 300)
    assert at[0] < 256 < at[-1]
    for chunk_size in (64, 256, 1000):
        assert _stream(sess, 100.0, rows, chunk_size).tobytes() == want.tobytes(), chunk_size


def test_a_carry_larger_than_the_push(sess, static_sess):
    rows = _random_rows(705, 9)
    first = int(rows["timestamp"].min())
    parts, carries = _push_by_push(sess, static_sess, 5000.0, [(rows[:700], first, False),
                                                               (rows[700:], int(rows["timestamp"][700:].min()), False),
                                                               (None, END, True)])
    assert carries[0] == 700 and 0 < carries[1] < 700 and len(parts[1]) > 5


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _assert_invalid(call, match):
    with pytest.raises(ValueError, match=match):
        call()


def test_refusals_leave_the_stream_untouched(sess, static_sess):
    a = _rows([1000, 400_000, 402_000], [0, 1, 2])
    b = _rows([404_000, 900_000], [0, 1], 3)
    window = 100.0
    rule = D.NumpyDfStream(window)
    lib = _lib.load()
    n = C.c_int64(0)
    out = np.zeros(4, dtype=DF_EVENT_ROW_DTYPE)

    def raw_push(rows, n_rows, horizon, final=0):
        return lib.wfa_df_event_stream_push(sess._h, None if rows is None else rows.ctypes.data_as(C.c_void_p), n_rows,
                                            horizon, final, C.byref(n), C.byref(n), C.byref(n))

    def fill(count):
        return lib.wfa_df_event_stream_fill(sess._h, out.ctypes.data_as(C.c_void_p), count)

    for bad_window in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="time_window_ps must be >= 0"):
            sess.df_event_stream_begin(bad_window)
    assert raw_push(None, 0, 0) == _lib.WFA_E_STATE                       # no stream is open
    sess.df_event_stream_begin(window)
    try:
        assert fill(0) == _lib.WFA_E_STATE                                # before a push
        got, carry = sess.df_event_stream_push(a, 400_000)
        want, want_carry = rule.push(a, 400_000)
        assert (got.tobytes(), carry) == (want.tobytes(), want_carry) and carry == 2
        assert fill(4) == _lib.WFA_E_INVALID and fill(1) == _lib.WFA_OK  # another count; the right one, again
        bad = b.copy()
        bad["reserved"][1] = 1
        _assert_invalid(lambda: sess.df_event_stream_push(bad, 900_000), "reserved != 0")
        assert fill(0) == _lib.WFA_E_STATE and fill(1) == _lib.WFA_E_STATE      # nothing to fill after a refused push
        bad = b.copy()
        bad["timestamp"][0] = 399_999                                      # below the previous horizon
        _assert_invalid(lambda: sess.df_event_stream_push(bad, 900_000), "below the previous push's horizon")
        _assert_invalid(lambda: sess.df_event_stream_push(b, 399_999), "lies below the previous push's")
        assert raw_push(b, 2**31 - 2, 900_000) == _lib.WFA_E_INVALID and "table limit" in _lib.last_error()  # carry 2 + rows
        assert raw_push(None, 1, 900_000) == _lib.WFA_E_INVALID and raw_push(b, -1, 900_000) == _lib.WFA_E_INVALID
        # the carry, the horizon and the event count are intact: the valid push gives what the rule gives
        got, carry = sess.df_event_stream_push(b, 900_000)
        want, want_carry = rule.push(b, 900_000)
        assert (got.tobytes(), carry) == (want.tobytes(), want_carry) and len(got) == 3 and carry == 1
        assert got["event_id"].tolist() == [1, 1, 1]
        got, carry = sess.df_event_stream_push(None, 900_000, True)
        assert got.tobytes() == rule.push(None, 900_000, True)[0].tobytes() and carry == 0
        # _begin on an open stream starts over: no carry, event 0, no horizon
        sess.df_event_stream_begin(window)
        assert sess.df_event_stream_push(a, 400_000)[1] == 2
        sess.df_event_stream_begin(window)
        got, carry = sess.df_event_stream_push(a[:1], 0, True)
        assert got["event_id"].tolist() == [0] and carry == 0
    finally:
        sess.df_event_stream_end()
    assert raw_push(None, 0, 0) == _lib.WFA_E_STATE
    table = np.concatenate([a, b])
    assert _stream(sess, window, table, 3).tobytes() == _static(static_sess, table, window).tobytes()


# ---- state ----------------------------------------------------------------------------------------------------------------
def test_release_scratch_between_pushes_changes_nothing(sess, static_sess):
    rows = _random_rows(3000, 11)
    want = _static(static_sess, rows, 5000.0)
    horizons = D.row_horizons(rows, 500)
    parts, carried = [], []
    sess.df_event_stream_begin(5000.0)
    try:
        for k, lo in enumerate(range(0, len(rows), 500)):
            got, carry = sess.df_event_stream_push(rows[lo : lo + 500], horizons[k], k == len(horizons) - 1)
            parts.append(got)
            carried.append(carry)
            before = sess.scratch_bytes()
            assert before > 0 and sess.release_scratch() == before and sess.scratch_bytes() == 0   # the carry is not scratch
    finally:
        sess.df_event_stream_end()
    assert max(carried) > 0 and carried[-1] == 0
    assert np.concatenate(parts).tobytes() == want.tobytes()


def test_open_beside_an_event_stream_on_one_context(sess, static_sess):
    rows = _random_rows(600, 12)
    hits, _w, _z = ES.golden("grouping_v1725")
    hits = hits[:600]
    want_hits = event_rows(hits, group_hit_windows_flat(hits, 100.0, session=static_sess))
    h_df, h_ev = D.row_horizons(rows, 100), ES.row_horizons(hits, 100)
    df_parts, ev_parts = [], []
    sess.df_event_stream_begin(100.0)
    sess.event_stream_begin(100.0)
    try:
        for k, lo in enumerate(range(0, 600, 100)):
            df_parts.append(sess.df_event_stream_push(rows[lo : lo + 100], h_df[k], k == 5)[0])
            ev_parts.append(sess.event_stream_push(hits[lo : lo + 100], h_ev[k])[0])
        ev_parts.append(sess.event_stream_push(None, float("inf"))[0])
    finally:
        sess.event_stream_end()
        sess.df_event_stream_end()
    assert np.concatenate(df_parts).tobytes() == _static(static_sess, rows, 100.0).tobytes()
    assert np.concatenate(ev_parts).tobytes() == want_hits.tobytes()


# ---- the plugins end to end -----------------------------------------------------------------------------------------------
CC = {"0:1": {"fixed_baseline": 7990.0}, "0:2": {"fixed_baseline": 8003.5}}
FEATURE_CONFIG = {"ragged": {}, "mixed": {"channel_config": CC, "height_range": (5, 20), "area_range": (2, None)},
                  "shuffled": {}}
WINDOWS = (0.0, 100.0, 5000.0)
PAIR_WINDOW = 3000.0


@functools.cache
def _static_chain(name, window_ns):
    """basic_features, df_events and df_paired of the static plugins under the run's configuration."""
    run = S.run(name)
    config = {"basic_features": {"wave_source": "records", **FEATURE_CONFIG[name]}, "df": {"wave_source": "records"},
              "df_events": {"time_window_ns": window_ns}, "time_window_ns": PAIR_WINDOW, "n_channels": 3}
    ctx = SimpleContext(config, {"records": run.records, "wave_pool": run.pool},
                        plugins=[HipBasicFeaturesPlugin(), HipDataFramePlugin(), HipGroupedEventsPlugin(),
                                 HipPairedEventsPlugin()])
    return ctx.get_data("run", "basic_features"), ctx.get_data("run", "df_events"), ctx.get_data("run", "df_paired")


def _assert_frames_equal(got, want):
    assert list(got.columns) == list(want.columns) and len(got) == len(want)
    for column in want.columns:
        assert got[column].dtype == want[column].dtype, column
        if got[column].dtype != object:
            np.testing.assert_array_equal(got[column].to_numpy(), want[column].to_numpy(), err_msg=column)
            continue
        for k, (a, b) in enumerate(zip(got[column], want[column])):
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), (column, k)


@pytest.mark.parametrize("workers", (1, 4), ids=("serial", "workers"))
@pytest.mark.parametrize("chunk_size", (1, 7, 1000))
@pytest.mark.parametrize("name", ("ragged", "mixed", "shuffled"))
def test_features_stream_equals_static_basic_features(name, chunk_size, workers, dp):
    run = S.run(name)
    ctx = SimpleContext({}, {"records": run.records, "wave_pool": run.pool})
    plugin = HipBasicFeaturesStream(device_pool=dp, **FEATURE_CONFIG[name])
    cfg = {"chunk_size": chunk_size, "parallel": workers > 1, "max_workers": workers}
    outs = list(plugin.compute(ctx, "run", streaming_config=cfg))
    assert len(outs) == len(run.chunks(chunk_size))
    got = np.concatenate([o.data for o in outs])
    want = _static_chain(name, 100.0)[0]
    assert got.dtype == want.dtype == BASIC_FEATURES_DTYPE and len(got) == len(run.records)
    assert got.tobytes() == want.tobytes()
    if name == "mixed" and chunk_size == 1000 and workers == 1:   # the fixed baselines and ranges did reach the pass
        plain = HipBasicFeaturesStream(device_pool=dp).compute_chunk(run.chunks(1000)[0], ctx, "run").data
        assert plain.tobytes() != got[: len(plain)].tobytes()


@pytest.mark.parametrize("workers", (1, 4), ids=("serial", "workers"))
@pytest.mark.parametrize("window_ns", WINDOWS)
@pytest.mark.parametrize("chunk_size", (1, 7, 1000))
@pytest.mark.parametrize("name", ("ragged", "mixed", "shuffled"))
def test_events_stream_equals_static_df_events_and_df_paired(name, chunk_size, window_ns, workers, dp):
    run = S.run(name)
    ctx = SimpleContext({}, {"records": run.records, "wave_pool": run.pool})
    plugin = HipGroupedEventsStream(device_pool=dp, time_window_ns=window_ns, **FEATURE_CONFIG[name])
    cfg = {"chunk_size": chunk_size, "parallel": workers > 1, "max_workers": workers}
    outs = list(plugin.compute(ctx, "run", streaming_config=cfg))
    first = 0
    for o in outs:
        assert o.data.dtype == DF_EVENT_ROW_DTYPE and len(o.data)
        assert (o.start, o.end) == (int(o.data["t_min"].min()), int(o.data["t_max"].max()) + 1)
        assert o.metadata["first_event"] == first
        first = int(o.data["event_id"][-1]) + 1
    rows = np.concatenate([o.data for o in outs])
    _bf, events, paired = _static_chain(name, window_ns)
    assert len(events) > 10 and (window_ns < 5000.0 or int(events["n_hits"].max()) > 1)
    _assert_frames_equal(grouped_events_frame(rows), events)
    got_paired = paired_events_frame(rows, PAIR_WINDOW, n_channels=3)
    np.testing.assert_array_equal(got_paired.index.to_numpy(), paired.index.to_numpy())
    _assert_frames_equal(got_paired, paired)
    assert plugin.stats["pushes"] == len(run.chunks(chunk_size)) and plugin.stats["rows_out"] == len(rows) == len(run.records)
    if chunk_size == 1:
        assert len(outs) > 10 and plugin.stats["max_carry"] < len(rows) // 4    # events leave as they close


def test_run_without_records_gives_no_chunks_and_a_small_pool_is_refused(dp):
    run = S.run("ragged")
    ctx = SimpleContext({}, {"records": run.records[:0], "wave_pool": run.pool})
    plugin = HipGroupedEventsStream(device_pool=dp)
    assert list(plugin.compute(ctx, "run")) == [] and plugin.stats["pushes"] == 0
    assert list(HipBasicFeaturesStream(device_pool=dp).compute(ctx, "run")) == []
    small = DevicePool([0], max_sessions=2)
    try:
        ctx = SimpleContext({}, {"records": run.records, "wave_pool": run.pool})
        with pytest.raises(ValueError, match="max_sessions >= 3"):
            list(HipGroupedEventsStream(device_pool=small).compute(ctx, "run"))
    finally:
        small.close()
