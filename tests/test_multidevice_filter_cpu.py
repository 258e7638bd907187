"""wave_pool_filtered and hit with the `devices` option, without a GPU: an oracle-backed stand-in session plays the
device (its filters, ranged download and find_peaks are the numpy / scipy oracle), so what is checked here is the
sharding -- record ranges, per-shard filter groups, which samples each shard writes back, the residency of the filtered
slices and failure handling."""

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests.test_multidevice_cpu import OracleSession, pinned_calls, traced
from waveformanalysis_amd import _lib, multidevice as MD
from waveformanalysis_amd import device as D
from waveformanalysis_amd.dtypes import HIT_DTYPE, RECORDS_DTYPE
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import (
    HipBasicFeaturesPlugin,
    HipHitFinderPlugin,
    HipThresholdHitPlugin,
    HipWaveformWidthIntegralPlugin,
    HipWavePoolFilteredPlugin,
)

DEVICE_SETS = [[0, 1], [0, 1, 2]]


class FilterOracleSession(OracleSession):
    """OracleSession with the device's float32 pool: the filters write the records' slices into it (the whole buffer
    zeroed first unless filter_keep_output(True)), download_filtered copies any range of it, the float32 source of the
    hit / feature passes reads it, find_peaks runs the oracle on the chosen source."""

    def __init__(self, device_id=0):
        super().__init__(device_id)
        self.f32 = None
        self.keep = False
        self.sg = (11, 2)
        self.peaks = None

    def upload_pool(self, wave_pool):
        super().upload_pool(wave_pool)
        self.f32 = self.pool.copy() if self.pool.dtype == np.float32 else None
        self.keep = False

    def upload_filtered_pool(self, pool_f32):
        self._note()
        assert pool_f32.size == self.n_samples
        self._drop_f32_tags()
        self.uploads += 1
        self.f32 = np.array(pool_f32, dtype=np.float32, copy=True)

    def filter_keep_output(self, keep):
        if keep and self.f32 is None:
            raise RuntimeError("keep requested but no filtered output exists yet")
        self.keep = bool(keep)

    def set_sg_plan(self, sg_window_size=11, sg_poly_order=2):
        self.sg = (int(sg_window_size), int(sg_poly_order))

    def _filter(self, kind, **kw):
        self._note()
        assert self.pool.dtype == np.uint16
        self._drop_f32_tags()
        if not self.keep or self.f32 is None:
            self.f32 = np.zeros(self.n_samples, dtype=np.float32)
        for o, n in zip(self.rec["wave_offset"].tolist(), self.rec["event_length"].tolist()):
            if n > 0:  # records.py:434-436: a later record's write wins
                self.f32[o:o + n] = O.apply_filter_core(self.pool[o:o + n].astype(np.float32), kind, **kw)

    def savgol(self, download=True):
        self._filter("SG", sg_window_size=self.sg[0], sg_poly_order=self.sg[1])
        return self.f32.copy() if download else None

    def sosfiltfilt(self, sos, zi, padlen, download=True):
        assert padlen == O.sosfiltfilt_padlen(sos)
        self._filter("BW", bw_sos=sos)
        return self.f32.copy() if download else None

    def download_filtered(self, out=None, start=0):
        self._note()
        if self.f32 is None:
            raise RuntimeError("no float32 pool is resident")
        if out is None:
            out = np.empty(self.n_samples - start, dtype=np.float32)
        D._check_out(out, np.dtype(np.float32), len(out))
        if start < 0 or start + len(out) > self.n_samples:
            raise ValueError("range outside the pool")
        out[:] = self.f32[start:start + len(out)]
        return out

    def _source(self, source):
        if source == _lib.SRC_RAW:
            assert self.pool is not None and self.pool.dtype == np.uint16
            return self.pool
        assert source == _lib.SRC_F32 and self.f32 is not None, "float32 source without a float32 pool"
        return self.f32

    def _on(self, source, fn):
        saved, self.pool = self.pool, self._source(source)
        try:
            return fn()
        finally:
            self.pool = saved

    def threshold_hits(self, source=_lib.SRC_RAW, left_extension=2, right_extension=2, max_len=0, download=True):
        return self._on(source, lambda: OracleSession.threshold_hits(self, _lib.SRC_RAW, left_extension,
                                                                     right_extension, max_len, download))

    def basic_features(self, source=_lib.SRC_RAW, *a, **k):
        return self._on(source, lambda: OracleSession.basic_features(self, _lib.SRC_RAW, *a, **k))

    def width_integral(self, source=_lib.SRC_RAW, *a, **k):
        return self._on(source, lambda: OracleSession.width_integral(self, _lib.SRC_RAW, *a, **k))

    def find_peaks(self, source=_lib.SRC_F32, use_derivative=True, height=30.0, distance=2, prominence=0.7, width=4,
                   threshold=None, height_method="minmax", height_window_extension=4, dense_rows=False, download=True):
        self._note()
        assert not dense_rows
        self.peaks = O.find_peak_hits(self.rec, self._source(source), use_derivative=use_derivative, height=height,
                                      distance=distance, prominence=prominence, width=width, threshold=threshold,
                                      height_method=height_method, height_window_extension=height_window_extension)
        return self.peaks if download else len(self.peaks)

    def download_peaks(self, out):
        self._note()
        D._check_out(out, HIT_DTYPE, len(self.peaks))
        out[:] = self.peaks


class OnePool:
    def __init__(self, factory):
        self.s = factory()

    def session(self):
        return self.s

    def peek_session(self):
        return self.s

    def drop_session(self):
        return True


def _ctx(rec, pool, factory=FilterOracleSession, **config):
    ctx = SimpleContext({"wave_source": "records", **config}, {"records": rec, "wave_pool": pool},
                        plugins=[HipWavePoolFilteredPlugin(), HipHitFinderPlugin(), HipThresholdHitPlugin(),
                                 HipBasicFeaturesPlugin(), HipWaveformWidthIntegralPlugin()])
    ctx.wfa_device_pool = OnePool(factory)
    ctx.wfa_session_factory = factory
    return ctx


def _get(rec, pool, name, devices, **config):
    """One plugin's output through a fresh context; the ShardedRun the call made (None for devices=None)."""
    ctx = _ctx(rec, pool, devices=devices, **config)
    try:
        out = ctx.get_data("run", name)
        runs = MD.peek_sharded_runs(ctx)
        return out, runs
    finally:
        MD.close_sharded_runs(ctx)


def _assert_same(name, rec, pool, devices, what, **config):
    want, none_runs = _get(rec, pool, name, None, **config)
    got, runs = _get(rec, pool, name, devices, **config)
    assert none_runs == [] and len(runs) == 1 and runs[0].n_shards == len(devices), what
    assert got.dtype == want.dtype and len(got) == len(want), what
    assert got.tobytes() == want.tobytes(), f"{what}: devices={devices} differs from devices=None"
    return got


# ---- inputs ----------------------------------------------------------------------------------------------------------
CHANNEL_FILTERS = {"0:3": {"filter_type": "BW", "lowcut": 0.01, "highcut": 0.2, "fs": 0.5, "filter_order": 2},
                   "0:7": {"sg_window_size": 21, "sg_poly_order": 4},
                   "0:12": {"filter_type": "BW", "lowcut": 0.02, "highcut": 0.15, "fs": 0.5, "filter_order": 5}}


def _fixture(name):
    case = G.load_case(name)
    cfg = {k: v for k, v in G.filter_params(case).items()} if name.startswith("sgbw_") else {}
    if name == "v1725_channel_cfg":
        cfg["channel_config"] = CHANNEL_FILTERS
    return case["records"], case["wave_pool"], cfg


def _hand_made(layout, seed=3):
    """Records on one pool, not as the builders lay them out.  "interleaved": disjoint slices with gaps, offsets out of
    order (every shard's span holds other shards' records); "overlapping": on top of that some records share samples,
    within one shard and between shards; "first_shard_overlap": only the first two records share samples."""
    rng = np.random.default_rng(seed)
    n = 36
    lengths = rng.integers(40, 260, n)
    lengths[[5, 17]] = [0, 9]                               # an empty record and one shorter than the SG window
    gaps = rng.integers(0, 30, n)
    starts = np.cumsum(np.concatenate(([3], (lengths + gaps)[:-1])))
    offsets = starts.copy()
    if layout in ("interleaved", "overlapping"):
        perm = rng.permutation(n)                           # every record keeps its slot, the slots come in any order
        offsets, lengths = starts[perm], lengths[perm]
    if layout == "overlapping":
        offsets[3] = offsets[1] + 10                        # inside shard 0
        offsets[30] = offsets[2] + 5                        # a late record over an early one
        lengths[[3, 30]] = [120, 200]
    if layout == "first_shard_overlap":
        offsets[1] = offsets[0] + lengths[0] // 2
    size = int((offsets + lengths).max()) + 17
    t = np.arange(size)
    pool = (8000 + 6 * np.sin(t / 7.0) + rng.normal(0, 3, size)).astype(np.int64)
    for o in rng.integers(0, size - 40, 60):                # negative pulses
        pool[o:o + 30] -= (300 * np.exp(-np.arange(30) / 6.0)).astype(np.int64)
    rec = np.zeros(n, dtype=RECORDS_DTYPE)
    rec["wave_offset"], rec["event_length"] = offsets, lengths
    rec["record_id"] = np.arange(n)
    rec["timestamp"] = np.arange(n) * 10_000
    rec["dt"] = 4
    rec["channel"] = np.arange(n) % 4
    rec["baseline"] = 8000.0
    rec["polarity"] = "negative"
    return rec, pool.astype(np.uint16)


FIXTURES = ["sgbw_bw1", "sgbw_bw9", "sgbw_bw12", "sgbw_sg15_13", "sgbw_sg21_16", "sgbw_sg63_12", "v1725_channel_cfg",
            "ragged_mixed"]
LAYOUTS = ["interleaved", "overlapping", "first_shard_overlap"]


def _inputs(name):
    if name in LAYOUTS:
        rec, pool = _hand_made(name)
        return rec, pool, {"channel_config": {"0:2": {"filter_type": "BW", "lowcut": 0.01, "highcut": 0.2,
                                                      "fs": 0.5, "filter_order": 3}}}
    return _fixture(name)


# ---- wave_pool_filtered ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", DEVICE_SETS, ids=lambda d: ",".join(map(str, d)))
@pytest.mark.parametrize("name", FIXTURES + LAYOUTS)
def test_wave_pool_filtered_equals_one_device(name, devices):
    rec, pool, cfg = _inputs(name)
    got = _assert_same("wave_pool_filtered", rec, pool, devices, f"{name} wave_pool_filtered", **cfg)
    assert got.dtype == np.float32 and len(got) == len(pool)
    covered = np.zeros(len(pool), dtype=bool)
    for o, n in zip(rec["wave_offset"].tolist(), rec["event_length"].tolist()):
        covered[o:o + max(n, 0)] = True
    assert not np.any(got[~covered])                          # gap samples 0.0
    assert np.any(got[covered] != 0)


def test_the_hand_made_layouts_take_the_routes_they_are_meant_for():
    for layout, shared in (("interleaved", False), ("overlapping", True), ("first_shard_overlap", False)):
        rec, _pool = _hand_made(layout)
        for n_shards in (2, 3):
            shards = MD.split_records(rec, n_shards)
            runs, _merged, got_shared = MD._own_samples(rec, shards)
            assert got_shared == shared, (layout, n_shards)
            if layout == "interleaved":                        # some span holds another shard's samples
                assert any(r[0].size and (r[0][0] > sh.span_start or r[1][-1] < sh.span_end or r[0].size > 1)
                           for r, sh in zip(runs, shards))
    rec, _pool = _hand_made("first_shard_overlap")
    sh0 = MD.split_records(rec, 2)[0]
    assert sh0.r0 == 0 and sh0.r1 > 1                          # the two overlapping records share a shard


def test_fixtures_filtered_equal_the_stored_reference():
    """The oracle stand-in is the reference's filter: the sharded output equals the stored wave_pool_filtered."""
    for name in ("sgbw_bw9", "sgbw_sg21_16", "ragged_mixed"):
        case = G.load_case(name)
        rec, pool, cfg = _fixture(name)
        got, _runs = _get(rec, pool, "wave_pool_filtered", [0, 1, 2], **cfg)
        np.testing.assert_array_equal(got, case["wave_pool_filtered"], err_msg=name)


# ---- hit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", DEVICE_SETS, ids=lambda d: ",".join(map(str, d)))
@pytest.mark.parametrize("name", FIXTURES + LAYOUTS)
def test_hit_equals_one_device(name, devices):
    rec, pool, cfg = _inputs(name)
    filt = {f"wave_pool_filtered.{k}": v for k, v in cfg.items()}
    for hit_cfg in ({}, {"use_filtered": False, "height": 12.0, "width": 2, "prominence": 2.0}):
        hit = {f"hit.{k}": v for k, v in hit_cfg.items()}
        got = _assert_same("hit", rec, pool, devices, f"{name} hit {hit_cfg}", **filt, **hit)
        assert got.dtype == HIT_DTYPE
    want_rows = _get(rec, pool, "hit", None, **filt, **{"hit.height": 6.0, "hit.width": 1, "hit.prominence": 0.5})[0]
    assert len(want_rows), f"{name}: no hits at all -- the comparison above shows little"


def test_hit_on_the_peaks_fixtures_equals_the_stored_reference():
    for name in ("peaks_ragged", "peaks_v1725"):
        case = G.load_peaks(name)
        for k, cfg in enumerate(case["configs"]):
            ctx = SimpleContext({"wave_source": "records", "devices": [0, 1, 2], **{f"hit.{a}": b for a, b in cfg.items()}},
                                {"records": case["records"], "wave_pool": case["wave_pool"],
                                 "wave_pool_filtered": case["wave_pool_filtered"]}, plugins=[HipHitFinderPlugin()])
            ctx.wfa_device_pool = OnePool(FilterOracleSession)
            ctx.wfa_session_factory = FilterOracleSession
            try:
                G.assert_struct_equal(ctx.get_data("run", "hit"), case[f"hit_{k}"], what=f"{name} cfg {k}")
                assert len(MD.peek_sharded_runs(ctx)) == 1
            finally:
                MD.close_sharded_runs(ctx)


# ---- residency -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v1725_channel_cfg", "ragged_mixed", "interleaved"])
def test_the_filtered_slices_stay_resident(name):
    rec, pool, cfg = _inputs(name)
    devices = [0, 1, 2]
    ctx = _ctx(rec, pool, devices=devices, use_filtered=True,
               **{f"wave_pool_filtered.{k}": v for k, v in cfg.items()})
    try:
        filtered = ctx.get_data("run", "wave_pool_filtered")
        run = MD.sharded_run(ctx, devices)
        busy = [sh.n_records > 0 for sh in MD.split_records(rec, 3)]
        assert [s.uploads for s in run.sessions] == [int(b) for b in busy]  # one raw slice each
        out = {k: ctx.get_data("run", k) for k in ("hit_threshold", "basic_features", "waveform_width_integral", "hit")}
        assert [s.uploads for s in run.sessions] == [int(b) for b in busy]  # and no float32 pool at all
        assert MD.peek_sharded_runs(ctx) == [run]
    finally:
        MD.close_sharded_runs(ctx)
    # the same chain on one device, float32 pool uploaded from the host
    one = _ctx(rec, pool, use_filtered=True, **{f"wave_pool_filtered.{k}": v for k, v in cfg.items()})
    np.testing.assert_array_equal(one.get_data("run", "wave_pool_filtered"), filtered)
    for k, v in out.items():
        assert one.get_data("run", k).tobytes() == v.tobytes(), k


def test_a_new_filtered_array_is_uploaded_again():
    rec, pool, cfg = _inputs("ragged_mixed")
    ctx = _ctx(rec, pool, devices=[0, 0], use_filtered=True)
    try:
        filtered = ctx.get_data("run", "wave_pool_filtered")
        run = MD.sharded_run(ctx, [0, 0])
        ctx.get_data("run", "hit_threshold")
        assert [s.uploads for s in run.sessions] == [1, 1]
        ctx._results[("run", "wave_pool_filtered")] = filtered.copy()  # equal contents, another object
        ctx._results.pop(("run", "basic_features"), None)
        ctx.get_data("run", "basic_features")
        assert [s.uploads for s in run.sessions] == [2, 2]
    finally:
        MD.close_sharded_runs(ctx)


# ---- failures --------------------------------------------------------------------------------------------------------
def _flaky(method):
    class Flaky(FilterOracleSession):
        pass

    def broken(self, *a, **k):
        if self.device_id == 5:
            raise RuntimeError("device lost")
        return getattr(FilterOracleSession, method)(self, *a, **k)

    setattr(Flaky, method, broken)
    return Flaky


@pytest.mark.parametrize("name,method", [("wave_pool_filtered", "savgol"), ("hit", "find_peaks")])
def test_a_failing_shard_raises_and_returns_no_table(name, method):
    case = G.load_case("ragged_mixed")
    factory = _flaky(method)
    ctx = _ctx(case["records"], case["wave_pool"], factory=factory, devices=[3, 5, 4])
    if name == "hit":  # the filtered pool comes in ready-made: only the hit pass can fail
        ctx._data["wave_pool_filtered"] = case["wave_pool_filtered"]
        del ctx._plugins["wave_pool_filtered"]
    try:
        with pytest.raises(RuntimeError) as err:
            ctx.get_data("run", name)
        shard_error = err.value if isinstance(err.value, MD.ShardError) else err.value.__cause__
        assert isinstance(shard_error, MD.ShardError) and shard_error.device_id == 5 and shard_error.shard == 1
        assert ("run", name) not in ctx._results
        run = MD.sharded_run(ctx, [3, 5, 4])
        assert run.sessions[1].device_id == 5 and run._filtered[1] is None
    finally:
        MD.close_sharded_runs(ctx)


def test_run_pool_failure_returns_nothing():
    case = G.load_case("ragged_mixed")
    run = MD.ShardedRun([3, 5], session_factory=_flaky("savgol"))
    old = list(run.sessions)

    def task(sess, rec_k):
        sess.upload_records(rec_k)
        sess.savgol(download=False)

    result = None
    with pytest.raises(MD.ShardError, match="device 5"):
        result = run.run_pool(case["records"], case["wave_pool"], task)
    assert result is None and old[1].closed and run.sessions[1] is not old[1] and run._filtered[1] is None
    run.close()


# ---- options ---------------------------------------------------------------------------------------------------------
def test_devices_none_constructs_no_sharded_run(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("ShardedRun constructed with devices=None")

    monkeypatch.setattr(MD.ShardedRun, "__init__", refuse)
    rec, pool, cfg = _inputs("v1725_channel_cfg")
    ctx = _ctx(rec, pool, **cfg)
    f = ctx.get_data("run", "wave_pool_filtered")
    h = ctx.get_data("run", "hit")
    assert len(f) == len(pool) and len(h) and MD.peek_sharded_runs(ctx) == []


def _sg(window, order):
    return [("set_sg_plan", {"sg_window_size": window, "sg_poly_order": order}), ("savgol", {"download": False})]


def test_each_route_does_the_parent_commits_device_work():
    """The ordered session calls of wave_pool_filtered and hit, as recorded before the records route became one function
    (tests/test_multidevice_cpu.py has the three other plugins): devices=None filters on the calling thread's session
    and downloads the whole float32 pool, devices=[0, 1] leaves each shard's output on its device and downloads the
    span of its own records; the filter groups of `v1725_channel_cfg` run in the order one device runs them, a shard
    skipping the groups none of its records belong to."""
    pool_up = [("ensure_pool", {"cacheable": True}), ("upload_pool", {})]
    records_up = ("upload_records", {"thresholds": None})
    off, on = ("filter_keep_output", {"keep": False}), ("filter_keep_output", {"keep": True})
    whole = [("download_filtered", {"out": None, "start": 0}), off, ("note_filtered", {})]
    bw = ("sosfiltfilt", {"download": False})
    Traced = traced(FilterOracleSession)

    def part(n, start):
        return [off, ("download_filtered", {"out": n, "start": start}), ("note_filtered", {})]

    def calls(plugin_cls, name, devices, **data):
        rec, pool, cfg = _inputs(name)
        ctx = _ctx(rec, pool, **cfg)
        ctx._data.update(data)
        got, seen = pinned_calls(plugin_cls, ctx, devices, Traced)
        return got, seen, rec

    # ragged_mixed: one Savitzky-Golay group; records [0, 6) on samples [4, 2339), records [6, 20) on [2340, 3756)
    one_group = pool_up + [off, records_up] + _sg(11, 2)
    got, seen, rec = calls(HipWavePoolFilteredPlugin, "ragged_mixed", None)
    assert got == [one_group + whole] and len(seen) == 1 and seen[0] is rec
    got, _seen, _rec = calls(HipWavePoolFilteredPlugin, "ragged_mixed", [0, 1])
    assert got == [one_group + part(2335, 4), one_group + part(1416, 4)]

    # v1725_channel_cfg: SG(11, 2), BW, SG(21, 4), BW in that order; the second half of the records has no first BW group
    groups = [off, records_up] + _sg(11, 2) + [records_up, on, bw, records_up] + _sg(21, 4) + [records_up, bw]
    got, _seen, _rec = calls(HipWavePoolFilteredPlugin, "v1725_channel_cfg", None)
    assert got == [pool_up + groups + whole]
    got, _seen, _rec = calls(HipWavePoolFilteredPlugin, "v1725_channel_cfg", [0, 1])
    second = [off, records_up] + _sg(11, 2) + [records_up, on] + _sg(21, 4) + [records_up, bw]
    assert got == [pool_up + groups + part(19200, 0), pool_up + second + part(19200, 0)]

    # hit on a ready-made wave_pool_filtered
    filtered = G.load_case("ragged_mixed")["wave_pool_filtered"]
    find = pool_up + [("upload_records", {"thresholds": "given"})]
    got, seen, rec = calls(HipHitFinderPlugin, "ragged_mixed", None, wave_pool_filtered=filtered)
    assert got == [find + [("find_peaks", {"download": True})]] and len(seen) == 1 and seen[0] is rec
    got, _seen, _rec = calls(HipHitFinderPlugin, "ragged_mixed", [0, 1], wave_pool_filtered=filtered)
    assert got == [find + [("find_peaks", {"download": False}), ("download_peaks", {})]] * 2


def test_devices_option_on_the_two_plugins():
    for cls in (HipWavePoolFilteredPlugin, HipHitFinderPlugin):
        opt = cls.options["devices"]
        assert opt.default is None and opt.track is False and "dense" in opt.help
