"""multidevice.split_records and ShardedRun without a GPU: an oracle-backed stand-in session plays the device."""

import threading

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from waveformanalysis_amd import _lib, multidevice as MD
from waveformanalysis_amd import device as D
from waveformanalysis_amd.dtypes import RECORDS_DTYPE, THRESHOLD_HIT_DTYPE
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipBasicFeaturesPlugin, HipThresholdHitPlugin, HipWaveformWidthIntegralPlugin


class OracleSession(D.DeviceSession):
    """DeviceSession whose 'device' is the numpy oracle: what a shard computes is what the reference computes on the
    records it was given, with the padded width it was told."""

    def __init__(self, device_id=0):  # no wfa_ctx
        self._h = None
        self.device_id = int(device_id)
        self._res_pool = self._res_filtered = None
        self.uploads = self.n_samples = self.n_records = self.max_len = 0
        self.pool = self.rec = self.thr = self.rows = None
        self.closed = False
        self.threads = set()

    def _note(self):
        self.threads.add(threading.get_ident())

    def upload_pool(self, wave_pool):
        self._note()
        self.forget_resident()
        self.uploads += 1
        self.pool = np.array(wave_pool, copy=True)
        self.n_samples = wave_pool.size

    def upload_records(self, records, thresholds=10.0, polarity=None):
        self._note()
        n = len(records)
        off = records["wave_offset"].astype(np.int64)
        ln = records["event_length"].astype(np.int64)
        assert np.all(off >= 0) and np.all((ln <= 0) | (off + ln <= self.n_samples)), "record outside the pool slice"
        self.rec = records.copy()
        self.thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, dtype=np.float64), (n,)))
        self.n_records = n
        self.max_len = int(ln.max()) if n else 0

    def threshold_hits(self, source=_lib.SRC_RAW, left_extension=2, right_extension=2, max_len=0, download=True):
        self._note()
        assert source == _lib.SRC_RAW
        assert max_len == 0 or max_len >= self.max_len
        rec, pool, thr = self.rec, self.pool, self.thr
        if max_len > self.max_len:  # the run's width: a record no threshold can fire on, padded to max_len
            ph = np.zeros(1, dtype=rec.dtype)
            ph["wave_offset"], ph["event_length"], ph["dt"] = len(pool), max_len, 1
            ph["record_id"] = int(rec["record_id"].max()) + 1 if len(rec) else 0
            rec = np.concatenate([rec, ph])
            pool = np.concatenate([pool, np.zeros(max_len, dtype=pool.dtype)])
            thr = np.append(thr, np.inf)
        self.rows = O.threshold_hits(rec, pool, thresholds=thr, left_extension=left_extension,
                                     right_extension=right_extension)
        return self.rows if download else len(self.rows)

    def download_hits(self, out):
        self._note()
        D._check_out(out, THRESHOLD_HIT_DTYPE, len(self.rows))
        out[:] = self.rows

    def basic_features(self, source=_lib.SRC_RAW, height_range=(40, 90), area_range=(0, None), fixed_baseline=None,
                       out=None):
        self._note()
        rows = O.basic_features(self.rec, self.pool, height_range=height_range, area_range=area_range,
                                fixed_baseline=fixed_baseline)
        if out is None:
            return rows
        out[:] = rows
        return out

    def width_integral(self, source=_lib.SRC_RAW, q_low=0.1, q_high=0.9, dt=2.0, out=None):
        self._note()
        rows = O.width_integral(self.rec, self.pool, q_low=q_low, q_high=q_high, dt=dt)
        if out is None:
            return rows
        out[:] = rows
        return out

    def release_scratch(self):
        return 0

    def close(self):
        self.forget_resident()
        self.closed = True


class OnePool:
    """wfa_device_pool of a context: one stand-in session for the calling thread."""

    def __init__(self):
        self.s = OracleSession()

    def session(self):
        return self.s

    def peek_session(self):
        return self.s

    def drop_session(self):
        return True


def _ctx(rec, pool, **config):
    ctx = SimpleContext({"wave_source": "records", **config}, {"records": rec, "wave_pool": pool})
    ctx.wfa_device_pool = OnePool()
    ctx.wfa_session_factory = OracleSession
    return ctx


# ---- split_records ---------------------------------------------------------------------------------------------------
def _records(lengths, offsets):
    rec = np.zeros(len(lengths), dtype=RECORDS_DTYPE)
    rec["event_length"] = lengths
    rec["wave_offset"] = offsets
    rec["record_id"] = np.arange(len(lengths))
    return rec


def _check_split(rec, shards, n_shards):
    assert len(shards) == n_shards
    assert shards[0].r0 == 0 and shards[-1].r1 == len(rec)
    for a, b in zip(shards, shards[1:]):
        assert a.r1 == b.r0                              # contiguous, in order, every record once
    off = rec["wave_offset"].astype(np.int64)
    ln = np.maximum(rec["event_length"].astype(np.int64), 0)
    for sh in shards:
        assert sh.r0 <= sh.r1 and sh.span_start <= sh.span_end
        for r in range(sh.r0, sh.r1):                     # every sample of a record inside its shard's span
            assert sh.span_start <= off[r] and off[r] + ln[r] <= sh.span_end


@pytest.mark.parametrize("n_shards", [1, 2, 3, 7, 8])
def test_split_builders_layout_is_exact_and_balanced(n_shards):
    rng = np.random.default_rng(n_shards)
    lengths = rng.integers(1, 2000, 400)
    offsets = np.concatenate(([0], np.cumsum(lengths)[:-1]))
    rec = _records(lengths, offsets)
    shards = MD.split_records(rec, n_shards)
    _check_split(rec, shards, n_shards)
    for sh in shards:                                     # exactly the shard's slice
        assert sh.span_start == offsets[sh.r0] and sh.span_end == offsets[sh.r1 - 1] + lengths[sh.r1 - 1]
    samples = np.array([lengths[sh.r0:sh.r1].sum() for sh in shards])
    assert samples.max() - samples.min() <= 2 * lengths.max()


def test_split_uniform_records_is_even():
    rec = _records(np.full(1000, 800), np.arange(1000) * 800)
    assert [sh.n_records for sh in MD.split_records(rec, 8)] == [125] * 8


def test_split_more_shards_than_records_and_zero_lengths():
    rec = _records([5, 0, 7], [0, 5, 5])
    shards = MD.split_records(rec, 7)
    _check_split(rec, shards, 7)
    assert sum(sh.n_records for sh in shards) == 3 and sum(sh.n_records == 0 for sh in shards) >= 4
    assert all(sh.span_start == sh.span_end == 0 for sh in shards if sh.n_records == 0)
    zeros = _records([0, 0, 0, 0], [3, 3, 9, 0])
    shards = MD.split_records(zeros, 2)
    _check_split(zeros, shards, 2)
    assert [sh.n_records for sh in shards] == [2, 2]
    empty = MD.split_records(_records([], []), 3)
    assert [(sh.r0, sh.r1) for sh in empty] == [(0, 0)] * 3


@pytest.mark.parametrize("n_shards", [2, 3, 7])
def test_split_out_of_order_and_overlapping_offsets(n_shards):
    rng = np.random.default_rng(11)
    lengths = rng.integers(0, 300, 60)
    offsets = rng.integers(0, 5000, 60)                  # any order, overlaps, gaps
    rec = _records(lengths, offsets)
    _check_split(rec, MD.split_records(rec, n_shards), n_shards)
    with pytest.raises(ValueError):
        MD.split_records(rec, 0)


# ---- ShardedRun through the plugins ----------------------------------------------------------------------------------
def _widest_alone(rec, n_shards):
    iw = int(np.argmax(rec["event_length"]))
    return any(sh.r0 == iw and sh.r1 == iw + 1 for sh in MD.split_records(rec, n_shards))


def _wanted(case):
    rec, pool = case["records"], case["wave_pool"]
    hits = O.threshold_hits(rec, pool, **G.hit_params(case))
    bf = O.basic_features(rec, pool, height_range=(40, 90), area_range=(0, None))
    wi = O.width_integral(rec, pool, dt=2.0)
    return hits, bf, wi


@pytest.mark.parametrize("n_shards", [2, 3, 7])
@pytest.mark.parametrize("name", ["ragged_mixed", "kat_padded_width"])
def test_sharded_plugins_equal_the_unsharded_oracle(name, n_shards):
    case = G.load_case(name)
    rec, pool = case["records"], case["wave_pool"]
    assert not case["options"]["hit"] and not case["options"]["bf"] and not case["options"]["wi"]
    want_hits, want_bf, want_wi = _wanted(case)
    ctx = _ctx(rec, pool, devices=[0] * n_shards)
    got_hits = HipThresholdHitPlugin().compute(ctx, "run")
    got_bf = HipBasicFeaturesPlugin().compute(ctx, "run")
    got_wi = HipWaveformWidthIntegralPlugin().compute(ctx, "run")
    G.assert_struct_equal(got_hits, want_hits, what=f"{name} hits, {n_shards} shards")
    G.assert_struct_equal(got_bf, want_bf, what=f"{name} basic_features, {n_shards} shards")
    G.assert_struct_equal(got_wi, want_wi, what=f"{name} width_integral, {n_shards} shards")
    run = MD.sharded_run(ctx, [0] * n_shards)
    assert run.n_shards == n_shards and all(isinstance(s, OracleSession) for s in run.sessions)
    assert all(len(s.threads) <= 1 for s in run.sessions)        # each session only ever used on its own worker
    assert len({t for s in run.sessions for t in s.threads}) == sum(1 for s in run.sessions if s.threads)
    MD.close_sharded_runs(ctx)
    assert run.closed and all(s.closed for s in run.sessions)


def test_widest_record_alone_is_what_the_width_test_covers():
    """The padded-width cases above put the widest record in its own shard: the other shards' hits at a record end
    read past it only under the run-wide width."""
    kat = G.load_case("kat_padded_width")["records"]
    ragged = G.load_case("ragged_mixed")["records"]
    assert _widest_alone(kat, 2) and _widest_alone(ragged, 7)
    # and the width matters there: the shard's own width gives other rows
    case = G.load_case("kat_padded_width")
    short = O.threshold_hits(case["records"][:1], case["wave_pool"])
    want = O.threshold_hits(case["records"], case["wave_pool"])
    assert len(short) and not np.array_equal(short, want[want["record_id"] == 0])


def test_per_channel_options_are_sliced_per_shard():
    case = G.load_case("v1725_channel_cfg")
    rec, pool = case["records"], case["wave_pool"]
    hit_opt, bf_opt = case["options"]["hit"], case["options"]["bf"]
    bp = G.bf_params(case)
    ctx = _ctx(rec, pool, devices=[0, 0, 0], **{"hit_threshold": hit_opt, "basic_features": bf_opt})
    G.assert_struct_equal(HipThresholdHitPlugin().compute(ctx, "run"), O.threshold_hits(rec, pool, **G.hit_params(case)),
                          what="per-channel thresholds")
    G.assert_struct_equal(HipBasicFeaturesPlugin().compute(ctx, "run"),
                          O.basic_features(rec, pool, fixed_baseline=bp["fixed_baseline"]), what="fixed_baseline")
    MD.close_sharded_runs(ctx)


def test_second_call_on_the_same_pool_uploads_nothing():
    case = G.load_case("ragged_mixed")
    rec, pool = case["records"], case["wave_pool"]
    ctx = _ctx(rec, pool, devices=[0, 0, 0])
    HipThresholdHitPlugin().compute(ctx, "run")
    run = MD.sharded_run(ctx, [0, 0, 0])
    before = [s.uploads for s in run.sessions]
    assert before == [1, 1, 1]
    HipBasicFeaturesPlugin().compute(ctx, "run")
    HipWaveformWidthIntegralPlugin().compute(ctx, "run")
    assert [s.uploads for s in run.sessions] == before
    ctx._data["wave_pool"] = pool.copy()                   # another object with equal contents: uploaded again
    HipBasicFeaturesPlugin().compute(ctx, "run")
    assert [s.uploads for s in run.sessions] == [2, 2, 2]
    MD.close_sharded_runs(ctx)


def test_a_failing_worker_raises_returns_no_table_and_replaces_its_session():
    case = G.load_case("ragged_mixed")
    rec, pool = case["records"], case["wave_pool"]
    finished = []

    class Flaky(OracleSession):
        def threshold_hits(self, *a, **k):
            if self.device_id == 5:
                raise RuntimeError("device lost")
            out = super().threshold_hits(*a, **k)
            finished.append(self.device_id)
            return out

    run = MD.ShardedRun([3, 5, 4], session_factory=Flaky)
    old = list(run.sessions)

    def task(sess, rec_k, out=None):
        sess.upload_records(rec_k)
        return sess.threshold_hits(_lib.SRC_RAW, 2, 2, max_len=int(rec["event_length"].max()), download=False)

    result = None
    with pytest.raises(MD.ShardError, match="device 5") as err:
        result = run.run(rec, pool, THRESHOLD_HIT_DTYPE, task, fetch=lambda s, out: s.download_hits(out))
    assert result is None and err.value.device_id == 5 and err.value.shard == 1
    assert isinstance(err.value.__cause__, RuntimeError)
    assert sorted(finished) == [3, 4]                      # the other workers finished
    assert old[1].closed and run.sessions[1] is not old[1] and run.sessions[1].device_id == 5
    assert run.sessions[0] is old[0] and run.sessions[2] is old[2] and not old[0].closed
    run.close()


def test_devices_none_constructs_no_sharded_run(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("ShardedRun constructed with devices=None")

    monkeypatch.setattr(MD.ShardedRun, "__init__", refuse)
    case = G.load_case("ragged_mixed")
    rec, pool = case["records"], case["wave_pool"]
    want_hits, want_bf, want_wi = _wanted(case)
    ctx = _ctx(rec, pool)
    G.assert_struct_equal(HipThresholdHitPlugin().compute(ctx, "run"), want_hits, what="hits")
    G.assert_struct_equal(HipBasicFeaturesPlugin().compute(ctx, "run"), want_bf, what="basic_features")
    G.assert_struct_equal(HipWaveformWidthIntegralPlugin().compute(ctx, "run"), want_wi, what="width_integral")
    assert MD.peek_sharded_runs(ctx) == []


# what a traced call keeps of its arguments (by parameter name); everything else about a call is its name and its place
PINNED_ARGS = {"ensure_pool": ("cacheable",), "upload_pool": (), "upload_records": ("thresholds",),
               "threshold_hits": ("download", "max_len"), "download_hits": (), "basic_features": ("out",),
               "width_integral": ("out",), "ensure_filtered_pool": ("cacheable",), "upload_filtered_pool": (),
               "filter_keep_output": ("keep",), "set_sg_plan": ("sg_window_size", "sg_poly_order"),
               "savgol": ("download",), "sosfiltfilt": ("download",), "download_filtered": ("out", "start"),
               "note_filtered": (), "find_peaks": ("download",), "download_peaks": ()}


def traced(base):
    """`base` (an OracleSession class) whose instances list their device calls in `calls`: (name, {pinned argument:
    value}), defaults filled in.  An array argument is pinned as "given" / None, `out` as its length; `records_seen`
    keeps the records objects that were uploaded."""
    import functools
    import inspect

    class Traced(base):
        def __init__(self, device_id=0):
            super().__init__(device_id)
            self.calls, self.records_seen = [], []

    def wrap(name, fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def method(self, *a, **k):
            bound = sig.bind(self, *a, **k)
            explicit = set(bound.arguments)
            bound.apply_defaults()
            pinned = {}
            for arg in PINNED_ARGS[name]:
                v = bound.arguments[arg]
                if arg == "out":
                    v = None if v is None else len(v)
                elif arg == "thresholds":
                    v = "given" if arg in explicit else None
                pinned[arg] = v
            if name == "upload_records":
                self.records_seen.append(bound.arguments["records"])
            self.calls.append((name, pinned))
            return fn(self, *a, **k)

        return method

    for name in PINNED_ARGS:
        if hasattr(base, name):
            setattr(Traced, name, wrap(name, getattr(base, name)))
    return Traced


def pinned_calls(plugin_cls, ctx, devices, session_cls):
    """The device calls of one compute() on `ctx`: [calls] of the calling thread's session for devices=None, else one
    list per shard session; and the records objects those sessions were given."""
    ctx.config["devices"] = devices
    ctx.wfa_session_factory = session_cls
    ctx.wfa_device_pool.s = session_cls()
    try:
        plugin_cls().compute(ctx, "run")
        sessions = [ctx.wfa_device_pool.s] if devices is None else MD.sharded_run(ctx, devices).sessions
        assert devices is not None or MD.peek_sharded_runs(ctx) == []
        if devices is not None:
            assert ctx.wfa_device_pool.s.calls == []         # the calling thread's session stays out of a sharded run
        return [s.calls for s in sessions], [r for s in sessions for r in s.records_seen]
    finally:
        MD.close_sharded_runs(ctx)


POOL_UP = [("ensure_pool", {"cacheable": True}), ("upload_pool", {})]
RECORDS_UP = ("upload_records", {"thresholds": None})


def test_each_route_does_the_parent_commits_device_work():
    """The ordered session calls of the three per-record plugins on `ragged_mixed`, as recorded before the records route
    became one function: devices=None on the calling thread's session (download inside the pass, padded width 0 = the
    longest uploaded record, the context's records object uploaded as it is), devices=[0, 1] on each shard's session
    (the run's padded width 1500, rows fetched / written into the shard's slice of the table)."""
    case = G.load_case("ragged_mixed")
    rec, pool = case["records"], case["wave_pool"]
    Traced = traced(OracleSession)
    rows = [sh.n_records for sh in MD.split_records(rec, 2)]
    assert min(rows) > 0 and int(rec["event_length"].max()) == 1500

    one = {
        HipThresholdHitPlugin: POOL_UP + [("upload_records", {"thresholds": "given"}),
                                          ("threshold_hits", {"download": True, "max_len": 0})],
        HipBasicFeaturesPlugin: POOL_UP + [RECORDS_UP, ("basic_features", None)],
        HipWaveformWidthIntegralPlugin: POOL_UP + [RECORDS_UP, ("width_integral", None)],
    }
    for cls, want in one.items():
        (calls,), seen = pinned_calls(cls, _ctx(rec, pool), None, Traced)
        # the feature passes: `out` of a fresh zeroed table or None is the same device work, only name and place count
        got = [(n, None if n in ("basic_features", "width_integral") else a) for n, a in calls]
        assert got == want, cls.provides
        assert len(seen) == 1 and seen[0] is rec, f"{cls.provides}: records copied on the way to the session"

    def two(k):
        return {
            HipThresholdHitPlugin: POOL_UP + [("upload_records", {"thresholds": "given"}),
                                              ("threshold_hits", {"download": False, "max_len": 1500}),
                                              ("download_hits", {})],
            HipBasicFeaturesPlugin: POOL_UP + [RECORDS_UP, ("basic_features", {"out": rows[k]})],
            HipWaveformWidthIntegralPlugin: POOL_UP + [RECORDS_UP, ("width_integral", {"out": rows[k]})],
        }

    for cls in one:
        per_session, _seen = pinned_calls(cls, _ctx(rec, pool), [0, 1], Traced)
        assert per_session == [two(0)[cls], two(1)[cls]], cls.provides


def test_devices_option_is_untracked_and_resolves():
    for cls in (HipThresholdHitPlugin, HipBasicFeaturesPlugin, HipWaveformWidthIntegralPlugin):
        opt = cls.options["devices"]
        assert opt.default is None and opt.track is False and "dense" in opt.help
    assert MD.resolve_devices(None) is None
    assert MD.resolve_devices([0, 0, 2]) == (0, 0, 2)
    with pytest.raises(ValueError):
        MD.resolve_devices("some")
    with pytest.raises(ValueError):
        MD.resolve_devices([])
