"""HipRecordsView / DeviceSession.view_gather on the GPU: every call of tests/golden/vx2730csv_records_view.npz (the reference's
RecordsView) byte for byte, a 2*10^4-record synthetic run of both adapters' record shapes against the numpy restatement
with many small device batches, the known answers of the reference's own test_records_view.py, a view over the pool
HipWavePoolFilteredPlugin leaves resident, and the argument checks of wfa_view_gather."""

import numpy as np
import pytest

from tests import records_view_util as U
from waveformanalysis_amd import _lib, synth
from waveformanalysis_amd.device import DevicePool, DeviceSession
from waveformanalysis_amd.dtypes import RECORDS_DTYPE
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipWavePoolFilteredPlugin
from waveformanalysis_amd.records_view import HipRecordsView, hip_records_view

pytestmark = pytest.mark.gpu

RECORDS, POOLS, CALLS, ARRAYS = U.load()


@pytest.fixture(scope="module")
def sess():
    with DeviceSession(0) as s:
        yield s


# ---- the reference's recorded arrays -----------------------------------------------------------------------------------
def test_every_fixture_call_byte_identical(sess):
    views = {name: HipRecordsView(RECORDS, pool, session=sess) for name, pool in POOLS.items()}
    for k, call in enumerate(CALLS):
        U.assert_same_bytes(U.run_call(views[call["pool"]], call), U.expected(call, k, ARRAYS), f"call {k} {call}")


def test_every_fixture_call_through_view_gather(sess):
    """The batch calls again through the session method, the row list and the window worked out here."""
    row_of = {int(rid): i for i, rid in enumerate(RECORDS["record_id"])}
    done = 0
    for name, pool in POOLS.items():
        sess.upload_pool(pool)
        sess.upload_records(RECORDS)
        for k, call in enumerate(CALLS):
            if call["pool"] != name or call["method"] == "query_time_window" or np.isscalar(call["ids"]) or not call["ids"]:
                continue
            kw = U.call_kwargs(call)
            want = U.expected(call, k, ARRAYS)
            mode = "signals" if call["method"] == "signals" else "waves_baseline" if kw.get("baseline_correct") else "waves"
            got = sess.view_gather([row_of[i] for i in call["ids"]], mode=mode, source=name, out_dtype=want[0].dtype,
                                   pad_len=want[0].shape[1], sample_start=kw.get("sample_start", 0),
                                   sample_end=kw.get("sample_end"), mask=bool(kw.get("mask")))
            got = (got[0], got[1].view(np.bool_)) if kw.get("mask") else (got,)
            U.assert_same_bytes(got, want, f"view_gather call {k} {call}")
            done += 1
    assert done >= 50


# ---- a larger run: several device batches, both buffers ------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["v1725", "vx2730"])
def test_synthetic_run_against_numpy(sess, preset):
    n = 20_000
    rec, pool = synth.make_run(n, preset, cfg=5)
    rng = np.random.default_rng(11)
    rec["polarity"] = rng.choice(["positive", "negative", "unknown"], size=n)
    rec["record_id"] = rng.permutation(n).astype(np.int64) * 3 + 17
    ids = rng.choice(rec["record_id"], size=n // 2, replace=False)
    ids = np.concatenate([ids, ids[:50], ids[-3:]])
    rng.shuffle(ids)
    want_view = U.NumpyRecordsView(rec, pool)
    view = HipRecordsView(rec, pool, session=sess)
    L = int(rec["event_length"][0])
    sess.profile(True)
    try:
        for batch_bytes in (L * 4 * 333 + 5, 256 << 20):
            view.batch_bytes = batch_bytes
            got = view.signals(ids, mask=True)
            U.assert_same_bytes(got, want_view.signals(ids, mask=True), f"{preset} signals batch_bytes={batch_bytes}")
        launches = sess.profile_report()["k_view_gather"][1]
        assert launches == -(-len(ids) // 333) + 1, launches   # many batches (both buffers in turn), then one
    finally:
        sess.profile(False)
    view.batch_bytes = L * 8 * 1000
    some = ids[:4321]
    U.assert_same_bytes((view.signals(some, dtype=np.float64, sample_start=7, sample_end=L - 9, pad_to=L + 3),),
                        (want_view.signals(some, dtype=np.float64, sample_start=7, sample_end=L - 9, pad_to=L + 3),),
                        f"{preset} float64 window")
    U.assert_same_bytes(view.waves(some, mask=True, sample_start=1), want_view.waves(some, mask=True, sample_start=1),
                        f"{preset} uint16 waves from an odd sample")
    U.assert_same_bytes((view.waves(some, baseline_correct=True),), (want_view.waves(some, baseline_correct=True),),
                        f"{preset} baseline-corrected waves")


# ---- the reference's own known answers (tests/test_records_view.py of the reference) ---------------------------------
def _sample_view(sess):
    records = np.zeros(3, dtype=RECORDS_DTYPE)
    records["timestamp"] = [10, 20, 30]
    records["channel"] = [0, 0, 1]
    records["record_id"] = [10, 11, 12]
    records["baseline"] = [1.0, 2.0, 0.0]
    records["polarity"] = ["positive", "negative", "unknown"]
    records["wave_offset"] = [0, 3, 5]
    records["event_length"] = [3, 2, 1]
    return HipRecordsView(records, np.array([1, 2, 3, 10, 11, 99], dtype=np.uint16), session=sess)


def test_known_answers_of_the_reference_suite(sess):
    rv = _sample_view(sess)
    wave0 = rv.waves(10)
    assert wave0.dtype == np.uint16 and wave0.tolist() == [1, 2, 3]
    wave1 = rv.waves(11, baseline_correct=True)
    assert wave1.dtype == np.float32 and wave1.tolist() == [8.0, 9.0]
    waves, mask = rv.waves([10, 12], pad_to=4, mask=True, dtype=np.float32)
    assert waves.dtype == np.float32 and waves.tolist() == [[1.0, 2.0, 3.0, 0.0], [99.0, 0.0, 0.0, 0.0]]
    assert mask.dtype == np.bool_ and mask.tolist() == [[True, True, True, False], [True, False, False, False]]
    subset = rv.query_time_window(t_min=15, t_max=25)
    assert subset.shape == (1,) and subset["timestamp"][0] == 20
    assert rv.waves(10, sample_start=1, sample_end=3).tolist() == [2, 3]
    assert rv.signals(11, sample_start=0, sample_end=2).tolist() == [8.0, 9.0]
    signal0 = rv.signals(10)
    assert signal0.tolist() == [0.0, -1.0, -2.0] and np.signbit(signal0).tolist() == [True, True, True]
    assert rv.signals(11).tolist() == [8.0, 9.0] and rv.signals(12).tolist() == [99.0]
    assert rv.signals(10, baseline=2.0).tolist() == [1.0, 0.0, -1.0]
    signals, mask = rv.signals([10, 11], pad_to=4, mask=True)
    assert signals.dtype == np.float32 and signals.tolist() == [[0.0, -1.0, -2.0, 0.0], [8.0, 9.0, 0.0, 0.0]]
    assert mask.tolist() == [[True, True, True, False], [True, True, False, False]]
    waves, mask = rv.waves([10, 11], sample_start=1, sample_end=3, pad_to=3, mask=True)
    assert waves.dtype == np.uint16 and waves.tolist() == [[2, 3, 0], [11, 0, 0]]
    assert mask.tolist() == [[True, True, False], [True, False, False]]
    assert len(rv) == 3


# ---- the pool wave_pool_filtered leaves resident ---------------------------------------------------------------------------
def test_view_over_the_filtered_pool_uploads_nothing():
    rec, pool = synth.make_run(512, "v1725", cfg=3)
    rec["polarity"][::3] = "positive"
    ctx = SimpleContext({"wave_source": "records"}, {"records": rec, "wave_pool": pool}, [HipWavePoolFilteredPlugin()])
    ctx.wfa_device_pool = DevicePool([0])
    try:
        filtered = ctx.get_data("run", "wave_pool_filtered")
        assert filtered.dtype == np.float32 and filtered.shape == pool.shape
        sess = ctx.wfa_device_pool.session()
        before = sess.uploads
        view = hip_records_view(ctx, "run", wave_pool_name="wave_pool_filtered")
        assert view.wave_pool is filtered
        ids = rec["record_id"][[5, 400, 17, 5, 511, 0]]
        got, mask = view.waves(ids, mask=True, sample_start=3, pad_to=800)
        assert got.dtype == np.float32 and mask[:, :797].all() and not mask[:, 797:].any()
        for row, rid in zip(got, ids):
            r = int(np.flatnonzero(rec["record_id"] == rid)[0])
            off = int(rec["wave_offset"][r])
            assert row[:797].tobytes() == filtered[off + 3:off + 800].tobytes() and not row[797:].any()
        assert view.waves(int(ids[1])).tobytes() == filtered[400 * 800:401 * 800].tobytes()
        U.assert_same_bytes((view.signals(ids, dtype=np.float64),),
                            (U.NumpyRecordsView(rec, filtered).signals(ids, dtype=np.float64),), "signals over filtered")
        assert sess.uploads == before
        raw = hip_records_view(ctx, "run")   # the raw pool is still the session's too
        assert raw.waves(int(ids[0])).tobytes() == pool[5 * 800:6 * 800].tobytes() and sess.uploads == before
    finally:
        ctx.wfa_device_pool.close()


# ---- argument checks and scratch ---------------------------------------------------------------------------------------------
def test_invalid_arguments_raise_before_any_launch(sess):
    view = HipRecordsView(RECORDS, POOLS["u16"], session=sess)
    view.waves(int(RECORDS["record_id"][3]))   # pool and records resident
    longest = int(RECORDS["event_length"].max())
    ok = dict(mode="signals", source="u16", out_dtype=np.float32, pad_len=longest)
    sess.profile(True)
    try:
        for rows, change, text in (
                ([0, len(RECORDS)], {}, "outside the resident table"),
                ([-1], {}, "outside the resident table"),
                ([0, 5], {"pad_len": longest - 1}, r"pad_len \(1499\) < max length \(1500\)"),
                ([0], {"pad_len": -1}, "negative pad_len"),
                ([0], {"mode": "waves", "source": "f32"}, "float32 pool not resident"),
                ([0], {"out_dtype": np.uint16}, "uint16 output is a copy"),
                ([0], {"mode": "waves_baseline", "out_dtype": np.uint16}, "uint16 output is a copy")):
            with pytest.raises((ValueError, _lib.WfaError), match=text):
                sess.view_gather(rows, **{**ok, **change})
            assert text.split(" ")[0].replace("\\", "") in _lib.last_error()
        lib = _lib.load()
        for mode, source, dtype, text in ((7, 0, 1, "unknown view mode"), (0, 5, 1, "unknown view source"),
                                          (0, 0, 9, "unknown view output type")):
            rc = lib.wfa_view_gather(sess._h, 0, None, 0, -1, 0, mode, source, dtype, None, 1 << 20, None, None)
            assert rc == _lib.WFA_E_INVALID and text in _lib.last_error()
        assert lib.wfa_view_gather(sess._h, -1, None, 0, -1, 0, 0, 0, 1, None, 1 << 20, None, None) == _lib.WFA_E_INVALID
        assert "negative row count" in _lib.last_error()
        # nothing to gather: zeros of the right shape, still no launch
        got, mask = sess.view_gather([3, 4], **{**ok, "pad_len": 6}, sample_start=9, sample_end=3, mask=True)
        assert got.shape == mask.shape == (2, 6) and not got.any() and not mask.any()
        assert sess.view_gather([3, 4], **{**ok, "pad_len": 0}, sample_end=0).shape == (2, 0)
        assert "k_view_gather" not in sess.profile_report()
        with pytest.raises(ValueError, match="one value per row"):
            sess.view_gather([0, 1], **ok, baseline_override=[1.0])
        with pytest.raises(ValueError, match="unknown view mode"):
            sess.view_gather([0], **{**ok, "mode": "bogus"})
        with pytest.raises(ValueError, match="out must be"):
            sess.view_gather([0], **ok, out=np.zeros((1, longest), dtype=np.float64))
        out = np.full((2, longest), 7.0, dtype=np.float32)
        assert sess.view_gather([5, 0], **ok, out=out) is out and not out[1].any() and out[0].any()
        assert sess.profile_report()["k_view_gather"][1] == 1
    finally:
        sess.profile(False)


def test_scratch_is_counted_and_released(sess):
    view = HipRecordsView(RECORDS, POOLS["u16"], session=sess)
    ids = [int(i) for i in RECORDS["record_id"]]
    want = view.signals(ids, mask=True)
    assert sess.scratch_bytes() >= want[0].nbytes + want[1].nbytes
    assert sess.release_scratch() > 0 and sess.scratch_bytes() == 0
    U.assert_same_bytes(view.signals(ids, mask=True), want, "after release_scratch")   # rebuilt on demand
    assert sess.release_scratch() > 0


def test_view_without_records_or_pool_is_a_state_error():
    with DeviceSession(0) as fresh:
        with pytest.raises(_lib.WfaError, match="records not uploaded"):
            fresh.view_gather([0], mode="waves", source="u16", out_dtype=np.float32, pad_len=4)
