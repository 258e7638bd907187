"""The S1/S2 peak chain on the device (wfa_peak_chain_count / _fill, DeviceSession.peak_chain) and the stream on top of
it (HipS1S2Stream): against the oracle chain, against the static HIP plugin chain byte for byte, chunk by chunk, and
the state the call leaves behind.  Every comparison is exact."""

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests import s1s2_chain_util as U
from tests import width_records_util as W
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DeviceSession
from waveformanalysis_amd.dtypes import HIT_DTYPE, S1_S2_CLASSIFIER_DTYPE
from waveformanalysis_amd.filter_engine import design_bw
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import hip_default
from waveformanalysis_amd.s1s2_stream import HipS1S2Stream

pytestmark = pytest.mark.gpu

STRICT_TEXT = "No S1/S2 criteria configured; set ranges or disable strict."


@pytest.fixture(scope="module")
def sess():
    with DeviceSession(0) as s:
        yield s


def _stage(sess, name, filter_type="SG"):
    """Pool + records up, filter and find_peaks with nothing downloaded; returns the peak count."""
    rec, pool, hit_kw = U.run(name)
    sess.upload_pool(pool)
    sess.upload_records(rec, 0.0)
    if filter_type == "SG":
        sess.set_sg_plan(11, 2)
        sess.savgol(download=False)
    else:
        sess.sosfiltfilt(*design_bw(0.1, 0.2, 0.5, 4), download=False)
    return sess.find_peaks(_lib.SRC_F32, download=False, **hit_kw)


# ---- 1. the session call against the oracle chain -------------------------------------------------------------------
def test_positive_run_equals_the_oracle_chain(sess):
    assert _stage(sess, "positive") == 15
    got = sess.peak_chain(**U.C5_RANGES)
    want = U.oracle_rows("positive", U.C5_RANGES)
    assert len(want) == 15 and len(np.unique(want["record_id"])) == 32 - 18
    assert got.dtype == S1_S2_CLASSIFIER_DTYPE
    G.assert_struct_equal(got, want, what="positive run")


def test_ragged_run_range_sets_width_options_and_sources(sess):
    assert _stage(sess, "ragged") == 32
    for class_kw, label_counts in U.RANGE_SETS:
        want = U.oracle_rows("ragged", class_kw)
        assert len(want) == 26 and U.counts(want) == label_counts, (class_kw, U.counts(want))
        got = sess.peak_chain(**class_kw)
        G.assert_struct_equal(got, want, what=f"ragged {class_kw}")
        assert U.counts(got) == label_counts
    # every range None: all unknown; strict refuses with the reference's text, on the host
    got = sess.peak_chain()
    G.assert_struct_equal(got, U.oracle_rows("ragged", {}), what="no ranges")
    assert U.counts(got) == (26, 0, 0)
    with pytest.raises(ValueError) as err:
        sess.peak_chain(strict=True)
    assert str(err.value) == STRICT_TEXT
    with pytest.raises(ValueError) as err:
        O.s1_s2_classify(*U.oracle_tables("ragged")[2:], strict=True)
    assert str(err.value) == STRICT_TEXT
    # the fixture's four width option sets (one without interpolation)
    options = W.load()["options"]
    assert len(options) == 4 and sum(o.get("interpolation") is False for o in options) == 1
    for k, opt in enumerate(options):
        want = U.oracle_rows("ragged", U.C5_RANGES, k)
        assert len(want) == 26
        G.assert_struct_equal(sess.peak_chain(**U.C5_RANGES, **opt), want, what=f"width options {k}")
    # widths on the float32 twin
    want = U.oracle_rows("ragged", U.C5_RANGES, 0, True)
    assert len(want) == 21
    G.assert_struct_equal(sess.peak_chain(_lib.SRC_F32, _lib.SRC_RAW, **U.C5_RANGES), want, what="float32 widths")


# ---- 2. byte for byte against the static HIP chain ------------------------------------------------------------------
def _static_rows(name, extra=None):
    rec, pool, hit_kw = U.run(name)
    ctx = SimpleContext({"wave_source": "records", **hit_kw, **U.C5_RANGES, **(extra or {})},
                        {"records": rec, "wave_pool": pool}, plugins=hip_default())
    return ctx.get_data("run", "s1_s2")


@pytest.fixture(scope="module")
def static_rows():
    return {name: _static_rows(name) for name in ("positive", "ragged", "uniform")}


@pytest.mark.parametrize("name", ["positive", "ragged", "uniform"])
def test_equals_the_static_chain_byte_for_byte(sess, static_rows, name):
    want = static_rows[name]
    assert len(want) > 10
    sess.profile(True)
    _stage(sess, name)
    got = sess.peak_chain(**U.C5_RANGES)
    report = sess.profile_report()
    sess.profile(False)
    assert got.tobytes() == want.tobytes()
    if name == "uniform":  # the routes of uniform records
        assert "k_find_peaks_hot" in report and "k_basic_features_leaf" in report, sorted(report)
    if name == "ragged":
        assert U.counts(want) == (0, 17, 9) and "k_basic_features" in report and "k_find_peaks_slots" in report, sorted(report)


def test_butterworth_filter_equals_the_static_chain(sess):
    bw = {"filter_type": "BW", "lowcut": 0.1, "highcut": 0.2, "fs": 0.5, "filter_order": 4}
    want = _static_rows("ragged", bw)
    assert len(want) > 5
    _stage(sess, "ragged", "BW")
    assert sess.peak_chain(**U.C5_RANGES).tobytes() == want.tobytes()


# ---- 3. the stream against the static chain -------------------------------------------------------------------------
def _stream(name, streaming_config, extra=None):
    rec, pool, hit_kw = U.run(name)
    ctx = SimpleContext({"wave_source": "records", **hit_kw, **U.C5_RANGES, **(extra or {})},
                        {"records": rec, "wave_pool": pool})
    outs = list(HipS1S2Stream().compute(ctx, "run", streaming_config=streaming_config))
    return rec, outs


def _check_stream(name, outs, rec, want, c):
    assert len(outs) == -(-len(rec) // c)
    assert all(o.data.dtype == S1_S2_CLASSIFIER_DTYPE for o in outs)
    got = np.concatenate([o.data for o in outs])
    assert got.tobytes() == want.tobytes(), name
    # the run's ids, chunk by chunk: chunk k holds rows of records [k * c, (k + 1) * c) only
    assert np.array_equal(got["record_id"], want["record_id"]) and np.all(np.isin(got["record_id"], rec["record_id"]))
    for k, o in enumerate(outs):
        assert np.all(o.data["record_id"] // c == k), (name, k)


@pytest.mark.parametrize("chunk_size", [1, 3, 7, 16, 40, 1000])
def test_stream_on_the_ragged_run(static_rows, chunk_size):
    want = static_rows["ragged"]
    assert len(want) == 26 and len(np.unique(want["record_id"])) > 10
    rec, outs = _stream("ragged", {"chunk_size": chunk_size, "parallel": False})
    _check_stream(f"ragged c={chunk_size}", outs, rec, want, chunk_size)
    empty = sum(len(o.data) == 0 for o in outs)
    hits = U.oracle_tables("ragged")[1]
    n_chunks = -(-40 // chunk_size)
    without_hit = n_chunks - len(np.unique(hits["record_id"] // chunk_size))
    all_dropped = n_chunks - len(np.unique(want["record_id"] // chunk_size)) - without_hit
    assert empty == without_hit + all_dropped
    if chunk_size == 1:  # 9 chunks without a hit, 6 whose hits were all dropped
        assert (without_hit, all_dropped) == (9, 6)
    if chunk_size == 3:
        assert without_hit == 2


@pytest.mark.parametrize("parallel", [True, False])
def test_stream_on_the_uniform_run(static_rows, parallel):
    want = static_rows["uniform"]
    rec, outs = _stream("uniform", {"chunk_size": 64, "parallel": parallel, "max_workers": 2})
    _check_stream(f"uniform parallel={parallel}", outs, rec, want, 64)
    assert len(outs) == 4 and all(len(o.data) for o in outs) and outs[-1].data["record_id"].max() >= 192


# ---- 4. state after the call ----------------------------------------------------------------------------------------
def test_state_after_the_call():
    rec, pool, hit_kw = U.run("ragged")
    hits = U.oracle_tables("ragged")[1]
    with DeviceSession(0) as sess:
        sess.ensure_pool(pool)
        sess.upload_records(rec, 0.0)
        sess.note_records(rec)
        sess.set_sg_plan(11, 2)
        sess.savgol(download=False)
        n = sess.find_peaks(_lib.SRC_F32, download=False, **hit_kw)
        assert n == len(hits) == 32
        before = sess.scratch_bytes()
        sess.profile(True)
        first = sess.peak_chain(**U.C5_RANGES)
        report = sess.profile_report()
        sess.profile(False)
        assert "k_peak_chain" in report and "k_peak_chain_compact" in report and "k_waveform_width_rec" not in report
        assert "k_basic_features" in report or "k_basic_features_leaf" in report
        assert len(first) == 26
        # the bound the header states: 36 B per record + 45 B per peak + 45 B per kept row; flags and offsets live in
        # find_peaks' per-candidate buffers
        grown = sess.scratch_bytes() - before
        assert 0 < grown <= 36 * len(rec) + 45 * n + 45 * len(first), grown
        out = np.empty(n, dtype=HIT_DTYPE)
        sess.download_peaks(out)
        G.assert_struct_equal(out, hits, what="hit table after peak_chain")
        assert sess.holds_pool(pool) and sess.holds_records(rec)
        assert sess.peak_chain(**U.C5_RANGES).tobytes() == first.tobytes()
        assert sess.release_scratch() > 0
        assert sess.peak_chain(**U.C5_RANGES).tobytes() == first.tobytes()
        # after a release the flags and offsets come back too: 12 B per peak and the scan's blocks
        assert sess.scratch_bytes() <= 36 * len(rec) + 45 * n + 45 * len(first) + 12 * n + 8 * (n // 1024 + 2)


# ---- 5. errors ------------------------------------------------------------------------------------------------------
def test_errors_leave_the_session_usable():
    rec, pool, hit_kw = U.run("positive")  # uniform records: the table also describes dense rows
    with DeviceSession(0) as sess:
        sess.upload_pool(pool)
        sess.upload_records(rec, 0.0)
        with pytest.raises(_lib.WfaError, match="no find_peaks pass"):
            sess.peak_chain(**U.C5_RANGES)
        assert sess.find_peaks(_lib.SRC_RAW, dense_rows=True, download=False) >= 0
        with pytest.raises(_lib.WfaError, match="WFA_PEAK_SIGNAL_RECORDS"):
            sess.peak_chain(**U.C5_RANGES)
        assert sess.find_peaks(_lib.SRC_RAW, download=False) > 0
        with pytest.raises(_lib.WfaError, match="wave_pool_filtered"):
            sess.peak_chain(_lib.SRC_F32, _lib.SRC_RAW, **U.C5_RANGES)
        with pytest.raises(_lib.WfaError, match="wave_pool_filtered"):
            sess.peak_chain(_lib.SRC_RAW, _lib.SRC_F32, **U.C5_RANGES)
        with pytest.raises(ValueError, match="float division by zero"):
            sess.peak_chain(sampling_rate=0.0, **U.C5_RANGES)
        with pytest.raises(ValueError, match="WFA_SRC_RAW or WFA_SRC_F32"):
            sess.peak_chain(_lib.SRC_SG_FUSED, _lib.SRC_RAW)
        sess.set_sg_plan(11, 2)
        sess.savgol(download=False)
        sess.upload_records(rec, 0.0)  # a new table: the rows of the pass before it are not evaluated on it
        with pytest.raises(_lib.WfaError, match="records have been replaced"):
            sess.peak_chain(**U.C5_RANGES)
        out = np.empty(sess.find_peaks(_lib.SRC_RAW, download=False), dtype=HIT_DTYPE)
        sess.upload_records(rec, 0.0)
        sess.download_peaks(out)  # (find_peaks' own fill is as it was)
        assert sess.find_peaks(_lib.SRC_F32, download=False, **hit_kw) == 15
        G.assert_struct_equal(sess.peak_chain(**U.C5_RANGES), U.oracle_rows("positive", U.C5_RANGES), what="after the errors")


def test_empty_tables_need_no_launch():
    rec, pool, _kw = U.run("positive")
    with DeviceSession(0) as sess:
        sess.upload_pool(pool)
        sess.upload_records(rec, 0.0)
        assert sess.find_peaks(_lib.SRC_RAW, download=False, height=1e9) == 0
        sess.profile(True)
        out = sess.peak_chain(sampling_rate=0.0, **U.C5_RANGES)  # (no peak: nothing is evaluated, as in the width pass)
        assert out.dtype == S1_S2_CLASSIFIER_DTYPE and len(out) == 0 and sess.profile_report() == {}
