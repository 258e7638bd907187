"""The dense routes (st_waveforms / filtered_waveforms) across several devices, the parts that need no GPU: the row
split, what every worker is handed, the per-shard residency tags, failure handling and waveform_width's hit partition.
An oracle-backed stand-in session plays the device (tests/test_multidevice_cpu.py::OracleSession plus the dense calls)."""

import math
import threading

import numpy as np
import pytest

from tests.test_multidevice_cpu import OnePool, OracleSession
from waveformanalysis_amd import dense, multidevice as MD
from waveformanalysis_amd.dtypes import (BASIC_FEATURES_DTYPE, THRESHOLD_HIT_DTYPE, WAVEFORM_WIDTH_DTYPE,
                                         create_filtered_waveform_dtype, create_record_dtype)
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import (HipBasicFeaturesPlugin, HipFilteredWaveformsPlugin, HipThresholdHitPlugin,
                                          HipWaveformWidthPlugin)
from waveformanalysis_amd.plugins import _common as K

NEGATIVE = "holds negative samples; the HIP backend reads unsigned ADC codes"


class DenseSession(OracleSession):
    """OracleSession with the dense calls: remembers every array it was asked to hold (`asked`), every one it uploaded
    (`dense_seen`) and every one noted as its float32 content (`noted`); refuses negative int16 samples the way
    DeviceSession.upload_dense does."""

    def __init__(self, device_id=0):
        super().__init__(device_id)
        self._res_records = None
        self.asked, self.dense_seen, self.noted = [], [], []

    def ensure_dense(self, data, what="st_waveforms"):
        self.asked.append(data)
        return super().ensure_dense(data, what=what)

    def upload_dense(self, data, batch_bytes=None, what="st_waveforms"):
        self._note()
        assert self._dense_layout(data) is not None
        self.forget_resident()
        wave = data["wave"]
        bad = np.flatnonzero((wave < 0).any(axis=1)) if wave.dtype == np.int16 else []
        self.first_negative_row = int(bad[0]) if len(bad) else -1
        if len(bad):
            raise ValueError(f"{what}['wave'] {NEGATIVE}")
        self.uploads += 1
        self.dense_seen.append(data)
        flat = np.ascontiguousarray(wave).reshape(-1)
        self.pool = flat.view(np.uint16) if wave.dtype == np.int16 else flat
        self.n_samples = flat.size

    def note_dense(self, data):
        self.noted.append(data)
        super().note_dense(data)


def _st(n, L, seed=3, baseline=True):
    """n rows of L samples at pedestal 1000, a distinct negative-going pulse per row."""
    rng = np.random.default_rng(seed)
    dtype = create_record_dtype(L)
    if not baseline:
        dtype = np.dtype([(name, dtype.fields[name][0]) for name in dtype.names if name != "baseline"])
    st = np.zeros(n, dtype=dtype)
    wave = 1000 + rng.integers(-2, 3, (n, L))
    for r in range(n):
        t0 = (3 * r) % max(L - 4, 1)
        wave[r, t0:t0 + 3] -= 40 + 5 * r
    st["wave"] = wave
    if baseline:
        st["baseline"] = 1000.0
    st["timestamp"] = 10**6 * np.arange(n)
    st["record_id"] = np.arange(n)
    st["dt"], st["event_length"], st["channel"] = 2, L, np.arange(n) % 3
    st["polarity"] = "negative"
    return st


def _ctx(st, **config):
    records = np.zeros(len(st), dtype=[("record_id", "i8"), ("event_length", "i4"), ("wave_offset", "i8")])
    records["record_id"], records["event_length"] = st["record_id"], st.dtype["wave"].shape[0]
    ctx = SimpleContext(config, {"st_waveforms": st, "records": records})
    ctx.wfa_device_pool = OnePool()
    ctx.wfa_device_pool.s = DenseSession()
    ctx.wfa_session_factory = DenseSession
    return ctx


# ---- the split rule --------------------------------------------------------------------------------------------------
def test_split_rule_over_lengths_rows_and_shards():
    for L in range(1, 34):
        unit = 8 // math.gcd(L, 8)
        assert MD.dense_unit(L) == unit
        for n in range(0, 41):
            for shards in range(1, 6):
                parts = MD.split_rows(n, L, shards)
                assert len(parts) == shards and parts[0][0] == 0 and parts[-1][1] == n, (L, n, shards)
                for (a0, a1), (b0, _b1) in zip(parts[:-1], parts[1:]):
                    assert a1 == b0 and a0 <= a1                       # contiguous, in order, covering
                for r0, r1 in parts:
                    assert r0 <= r1 and (r0 % unit == 0 or r0 == n) and (r1 % unit == 0 or r1 == n)
                    assert r0 == r1 or (r0 * L) % MD.POOL_ALIGN == 0   # what the rule is for
                sizes = [r1 - r0 for r0, r1 in parts]
                assert max(sizes) - min(sizes) <= unit, (L, n, shards, parts)


def test_split_of_the_shapes_the_gpu_tests_use():
    assert MD.split_rows(21, 13, 3) == [(0, 8), (8, 16), (16, 21)]       # L odd: boundaries on multiples of 8 rows
    assert MD.split_rows(10, 12, 3) == [(0, 2), (2, 6), (6, 10)]         # unit 2
    assert MD.split_rows(2, 800, 3) == [(0, 0), (0, 1), (1, 2)]          # an empty shard
    assert MD.split_rows(0, 800, 3) == [(0, 0)] * 3
    with pytest.raises(ValueError):
        MD.split_rows(4, 8, 0)


# ---- what a worker is handed -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", [(21, 13), (10, 12), (2, 800), (17, 16)])
def test_every_worker_sees_its_rows_and_shifted_records(n, L):
    st = _st(n, L)
    rec = dense.dense_records(st, L)
    per_row = np.arange(n, dtype=np.float64)
    seen = {}

    def task(sess, rec_k, per_k, scalar, out):
        seen[sess.device_id] = (rec_k.copy(), per_k.copy(), scalar, threading.get_ident())
        out["event_index"] = np.arange(len(rec_k))

    with MD.ShardedRun([0, 1, 2], session_factory=DenseSession) as run:
        out = run.run(rec, st, BASIC_FEATURES_DTYPE, task, per_record=(per_row, 7.5), record_index_field="event_index",
                      rows=("st_waveforms", L, n))
        parts = MD.split_rows(n, L, 3)
        for k, (r0, r1) in enumerate(parts):
            sess = run.sessions[k]
            if r0 == r1:
                assert k not in seen and sess.asked == [] and sess.uploads == 0
                continue
            (view,) = sess.asked
            assert view.base is st or view.base is st.base
            assert len(view) == r1 - r0 and np.shares_memory(view, st[r0:r1])
            assert view["wave"].ctypes.data == st["wave"][r0:r1].ctypes.data      # exactly data[r0:r1], no copy
            assert sess.n_samples == (r1 - r0) * L and sess.uploads == 1
            rec_k, per_k, scalar, _thread = seen[k]
            assert np.array_equal(rec_k["wave_offset"], np.arange(r1 - r0) * L)   # starts at 0, inside the shard
            assert np.array_equal(rec_k["record_id"], np.arange(r0, r1)) and np.array_equal(per_k, per_row[r0:r1])
            assert scalar == 7.5
        assert sum(s.n_samples for s in run.sessions) == n * L
        threads = [seen[k][3] for k in seen]
        assert len(set(threads)) == len(threads) and threading.get_ident() not in threads
    assert np.array_equal(out["event_index"], np.arange(n))                       # r0 added per shard


def test_fetch_kind_gets_the_row_length_as_width():
    st = _st(10, 12)
    rec = dense.dense_records(st, 12)
    rec["event_length"][3] = 5                                                    # hit's truncated rows: width stays L
    widths = []

    def task(sess, rec_k, out, max_len):
        widths.append(max_len)
        sess.rows = np.zeros(len(rec_k), dtype=THRESHOLD_HIT_DTYPE)
        sess.rows["record_id"] = rec_k["record_id"]
        return len(rec_k)

    with MD.ShardedRun([0, 0, 0], session_factory=DenseSession) as run:
        out = run.run(rec, st, THRESHOLD_HIT_DTYPE, task, fetch=lambda s, o: s.download_hits(o), width_arg="max_len",
                      rows=("st_waveforms", 12, 10))
    assert widths == [12, 12, 12] and np.array_equal(out["record_id"], np.arange(10))


# ---- the plugins through the stand-in --------------------------------------------------------------------------------
def test_plugins_shard_the_default_route_and_equal_one_device():
    st = _st(21, 13)
    for cls in (HipThresholdHitPlugin, HipBasicFeaturesPlugin):
        one = cls().compute(_ctx(st), "run")
        ctx = _ctx(st, devices=[0, 1, 2])
        got = cls().compute(ctx, "run")
        assert len(one) and got.dtype == one.dtype and got.tobytes() == one.tobytes(), cls.provides
        (run,) = MD.peek_sharded_runs(ctx)                                        # wave_source="auto" took the devices
        assert [s.n_samples for s in run.sessions] == [8 * 13, 8 * 13, 5 * 13]
        assert [s.uploads for s in run.sessions] == [1, 1, 1] and ctx.wfa_device_pool.s.uploads == 0
        MD.close_sharded_runs(ctx)


def test_devices_option_on_all_six_plugins():
    from waveformanalysis_amd.plugins import HipHitFinderPlugin, HipWaveformWidthIntegralPlugin

    for cls in (HipThresholdHitPlugin, HipBasicFeaturesPlugin, HipWaveformWidthIntegralPlugin, HipHitFinderPlugin,
                HipFilteredWaveformsPlugin, HipWaveformWidthPlugin):
        opt = cls.options["devices"]
        assert opt.default is None and opt.track is False and opt.help is K.DEVICES_HELP
    assert "stay on one" not in K.DEVICES_HELP and "row range" in K.DEVICES_HELP


def test_errors_that_need_no_device_come_before_any_worker():
    st = _st(9, 12)
    ctx = _ctx(st, devices=[0, 0, 0])
    ctx._data["records"] = ctx._data["records"][:-2]
    with pytest.raises(ValueError, match="could not resolve record_id"):
        HipThresholdHitPlugin().compute(ctx, "run")
    assert MD.peek_sharded_runs(ctx) == []
    ctx = _ctx(st, devices=[0, 0, 0])
    ctx._data["st_waveforms"] = np.zeros(4, dtype=[("wave", "<i4", (4,)), ("channel", "i2")])
    with pytest.raises(ValueError, match="must be int16 or float32, got int32"):                  # dense_pool's check
        HipBasicFeaturesPlugin().compute(ctx, "run")
    assert MD.peek_sharded_runs(ctx) == []


# ---- residency tags --------------------------------------------------------------------------------------------------
def _count(sess, rec_k, out):
    out["event_index"] = 0


def test_same_object_uploads_once_a_copy_again_and_the_routes_evict_each_other():
    st, L = _st(17, 16), 16
    rec = dense.dense_records(st, L)
    rows = ("st_waveforms", L, len(st))
    pool = np.arange(17 * 16, dtype=np.uint16)
    with MD.ShardedRun([0, 0, 0], session_factory=DenseSession) as run:
        uploads = lambda: [s.uploads for s in run.sessions]  # noqa: E731
        run.run(rec, st, BASIC_FEATURES_DTYPE, _count, rows=rows)
        assert uploads() == [1, 1, 1] and all(t is not None and t[0] is st for t in run._dense)
        views = [t[3] for t in run._dense]
        run.run(rec, st, BASIC_FEATURES_DTYPE, _count, rows=rows)
        assert uploads() == [1, 1, 1]                                              # the same object: nothing uploaded
        assert all(t[3] is v for t, v in zip(run._dense, views))                   # the view object is kept
        twin = st.copy()
        run.run(rec, twin, BASIC_FEATURES_DTYPE, _count, rows=rows)
        assert uploads() == [2, 2, 2] and all(t[0] is twin for t in run._dense)    # equal contents, another object
        run.run(rec, pool, BASIC_FEATURES_DTYPE, _count)                           # a records-route run in between
        assert uploads() == [3, 3, 3] and run._dense == [None] * 3 and all(t is not None for t in run._resident)
        run.run(rec, twin, BASIC_FEATURES_DTYPE, _count, rows=rows)
        assert uploads() == [4, 4, 4] and run._resident == [None] * 3              # and the other way round
        run.run(rec, pool, BASIC_FEATURES_DTYPE, _count)
        assert uploads() == [5, 5, 5]
    assert run._dense == [None] * 3 and run._resident == [None] * 3                # close drops every tag


def test_filtered_rows_are_tagged_beside_the_raw_rows():
    st, L = _st(10, 12), 12
    rec = dense.dense_records(st, L)
    rows = ("st_waveforms", L, len(st))
    out = np.zeros(len(st), dtype=create_filtered_waveform_dtype(st.dtype))

    def fill(sess, rec_k, out):
        sess._drop_f32_tags()                                                      # what the filters do
        out["wave"] = 1.5

    with MD.ShardedRun([0, 0, 0], session_factory=DenseSession) as run:
        got = run.run(rec, st, out.dtype, fill, rows=rows, out=out, note_out=True)
        assert got is out and np.all(out["wave"] == 1.5)
        for k, (r0, r1) in enumerate(MD.split_rows(10, 12, 3)):
            sess, tag = run.sessions[k], run._dense_f32[k]
            assert tag[0] is out and tag[1:3] == (r0, r1) and sess.noted[-1] is tag[3]
            assert sess.holds_dense(tag[3]) and sess.holds_dense(run._dense[k][3])  # both buffers, as one session
        run.run(rec, out, BASIC_FEATURES_DTYPE, _count, rows=("filtered_waveforms", L, len(st)))
        run.run(rec, st, BASIC_FEATURES_DTYPE, _count, rows=rows)
        assert [s.uploads for s in run.sessions] == [1, 1, 1]                      # neither array went up again
        run.run(rec, st, out.dtype, fill, rows=rows, out=out, note_out=False)      # a layout that cannot stay
        assert run._dense_f32 == [None] * 3 and run._dense == [None] * 3
        assert not any(s.holds_dense(st[r0:r1]) for s, (r0, r1) in zip(run.sessions, MD.split_rows(10, 12, 3)))


def test_a_layout_the_device_refuses_is_sharded_through_the_records_route_and_leaves_no_tag():
    st = _st(16, 12)
    view = st[::2]
    one = HipBasicFeaturesPlugin().compute(_ctx(view), "run")
    ctx = _ctx(view, devices=[0, 0, 0])
    for _ in range(2):
        got = HipBasicFeaturesPlugin().compute(ctx, "run")
        assert got.tobytes() == one.tobytes()
    (run,) = MD.peek_sharded_runs(ctx)
    assert [s.uploads for s in run.sessions] == [2, 2, 2] and all(s.dense_seen == [] for s in run.sessions)
    assert run._dense == run._dense_f32 == run._resident == [None] * 3
    MD.close_sharded_runs(ctx)


# ---- failures --------------------------------------------------------------------------------------------------------
def test_a_failing_shard_raises_is_replaced_and_the_others_finish():
    st, L = _st(21, 13), 13
    rec = dense.dense_records(st, L)
    finished = []

    def task(sess, rec_k, out):
        if sess.device_id == 5:
            raise RuntimeError("device lost")
        finished.append(sess.device_id)

    run = MD.ShardedRun([3, 5, 4], session_factory=DenseSession)
    old = list(run.sessions)
    result = None
    with pytest.raises(MD.ShardError, match="device 5") as err:
        result = run.run(rec, st, BASIC_FEATURES_DTYPE, task, rows=("st_waveforms", L, len(st)))
    assert result is None and err.value.device_id == 5 and err.value.shard == 1
    assert isinstance(err.value.__cause__, RuntimeError) and sorted(finished) == [3, 4]
    assert old[1].closed and run.sessions[1] is not old[1] and run.sessions[1].device_id == 5
    assert run._dense[1] is None and run._dense[0] is not None and run.sessions[0] is old[0]
    run.close()


def test_a_negative_sample_names_the_absolute_row_and_a_good_call_follows():
    st = _st(21, 13)
    bad = st.copy()
    bad["wave"][11, 4] = -3                                                        # rows 8..15 are the second shard's
    bad["wave"][19, 0] = -1                                                        # and a later one in the third
    ctx = _ctx(bad, devices=[0, 0, 0])
    with pytest.raises(MD.ShardError, match="shard 1") as err:
        HipBasicFeaturesPlugin().compute(ctx, "run")
    assert isinstance(err.value.__cause__, ValueError) and NEGATIVE in str(err.value.__cause__)
    (run,) = MD.peek_sharded_runs(ctx)
    assert [s.first_negative_row for s in run.sessions] == [-1, 11, 19]
    ctx._data["st_waveforms"] = st
    got = HipBasicFeaturesPlugin().compute(ctx, "run")
    assert got.tobytes() == HipBasicFeaturesPlugin().compute(_ctx(st), "run").tobytes()
    assert [s.first_negative_row for s in run.sessions] == [-1, -1, -1]
    MD.close_sharded_runs(ctx)


# ---- waveform_width's hit partition ----------------------------------------------------------------------------------
def test_partition_and_scatter_back_is_the_identity_on_hit_order():
    rng = np.random.default_rng(11)
    for trial in range(200):
        n_rows = int(rng.integers(0, 40))
        L = int(rng.integers(1, 20))
        shards = int(rng.integers(1, 6))
        parts = MD.split_rows(n_rows, L, shards)
        bounds = [r0 for r0, _ in parts] + [parts[-1][1]]
        index = rng.integers(-3, n_rows + 4, int(rng.integers(0, 60)))
        picks = MD.partition_hits(index, bounds)
        assert len(picks) == shards
        back = np.full(len(index), -99, dtype=np.int64)
        for (r0, r1), mine in zip(parts, picks):
            assert np.all(np.diff(mine) > 0)                                       # hit order kept inside a shard
            assert np.all((index[mine] >= r0) & (index[mine] < r1))
            back[mine] = (index[mine] - r0) + r0
        placed = (index >= 0) & (index < n_rows)
        assert np.array_equal(back[placed], index[placed]) and np.all(back[~placed] == -99), trial
        assert sum(len(m) for m in picks) == int(placed.sum())


def test_waveform_width_routes_cut_and_scatter_the_hit_table():
    """Both routes through K's hit routes with a pass that answers from what it was handed: the shifted index plus the
    shard's first row must give the hit's own row back, in hit order; hits with no row stay invalid."""
    st, L = _st(21, 13), 13
    row = np.array([15, 16, 7, 8, -1, 0, 20, 21, 400, 8, 15], dtype=np.int64)     # edges of shards, unsorted, invalid
    position = np.arange(len(row)) * 10
    handed = {}

    def widths(sess, rec_k, mine, row_k, n_rows):
        handed.setdefault(sess.device_id, []).append((np.array(position[mine]), np.array(row_k), n_rows))
        out = np.zeros(len(row_k), dtype=WAVEFORM_WIDTH_DTYPE)
        out["peak_position"] = position[mine]
        out["record_id"] = row_k
        return out, (row_k >= 0) & (row_k < n_rows)

    ctx = _ctx(st, devices=[0, 1, 2, 3])                                           # rows 0-8, 8-8 (empty), 8-16, 16-21
    parts = MD.split_rows(21, 13, 4)
    assert parts == [(0, 0), (0, 8), (8, 16), (16, 21)]
    rows, valid = K.dense_hit_route(ctx, HipWaveformWidthPlugin(), K.dense_input(st, "st_waveforms"), row, widths)
    assert np.array_equal(valid, (row >= 0) & (row < 21)) and np.array_equal(rows["peak_position"][valid], position[valid])
    first = np.array([parts[k][0] for k in (1, 2, 3)])
    shard_of = np.searchsorted(first, row[valid], side="right") - 1
    assert np.array_equal(rows["record_id"][valid] + first[shard_of], row[valid])
    assert 0 not in handed and [h[2] for k in (1, 2, 3) for h in handed[k]] == [8, 8, 5]
    (run,) = MD.peek_sharded_runs(ctx)
    assert [s.uploads for s in run.sessions] == [0, 1, 1, 1]
    # a shard with no hits uploads nothing
    K.dense_hit_route(ctx, HipWaveformWidthPlugin(), K.dense_input(st.copy(), "st_waveforms"), np.array([3, 17]), widths)
    assert [s.uploads for s in run.sessions] == [0, 2, 1, 2]
    MD.close_sharded_runs(ctx)

    # the records route: record_id is an index into records, shards by sample count
    rec = dense.dense_records(st, L)
    pool = np.ascontiguousarray(st["wave"]).reshape(-1).view(np.uint16)
    ctx = _ctx(st, devices=[0, 1, 2])
    handed.clear()
    rows, valid = K.records_hit_route(ctx, HipWaveformWidthPlugin(), rec, pool, row, widths)
    shards = MD.split_records(rec, 3)
    first = np.array([sh.r0 for sh in shards])
    assert np.array_equal(valid, (row >= 0) & (row < 21))
    shard_of = np.searchsorted(first, row[valid], side="right") - 1
    assert np.array_equal(rows["record_id"][valid] + first[shard_of], row[valid])
    assert np.array_equal(rows["peak_position"][valid], position[valid])
    MD.close_sharded_runs(ctx)
