"""Per-channel filter settings and fixed baselines of the S1/S2 stream on the device: wfa_savgol_group against
wfa_savgol on the member sub-table, wfa_peak_chain_count_fixed against the static chain, and HipS1S2Stream with
filter_source="wave_pool_filtered" and baseline_source="basic_features" against the reference's fixture and the static HIP
chain.  Every comparison is exact."""

import numpy as np
import pytest

from tests import s1s2_chain_util as U
from tests import s1s2_settings_util as T
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DevicePool, DeviceSession
from waveformanalysis_amd.dtypes import S1_S2_CLASSIFIER_DTYPE
from waveformanalysis_amd.filter_engine import design_bw
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import hip_default
from waveformanalysis_amd.s1s2_stream import HipS1S2Stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sess():
    with DeviceSession(0) as s:
        yield s


@pytest.fixture(scope="module")
def ref():
    """A second session: wfa_savgol on the member sub-tables."""
    with DeviceSession(0) as s:
        yield s


def _slices(rec, mask, n_samples):
    """The samples of the records rec[mask] in a pool of n_samples."""
    keep = np.zeros(n_samples, dtype=bool)
    for o, n in zip(rec["wave_offset"][mask], rec["event_length"][mask]):
        keep[o : o + n] = True
    return keep


# ---- 1. savgol_group against savgol on the member sub-table -----------------------------------------------------------
@pytest.mark.parametrize("kind,kernel", [("ragged", "k_savgol<group>"), ("span", "k_savgol_span<group>"),
                                         ("padded", "k_savgol_span<padded, group>")])
def test_savgol_group_equals_savgol_on_the_member_records(sess, ref, kind, kernel):
    rec, pool, gor, plans = T.split_run(kind)
    sess.upload_pool(pool)
    sess.upload_records(rec, 0.0)
    sess.set_sg_plan(5, 3)
    base = expected = sess.savgol()  # what every sample of the twin reads before the group calls
    assert np.count_nonzero(expected) > len(pool) // 2
    ref.upload_pool(pool)
    for slot, pair in enumerate(plans):
        sess.store_sg_plan(slot, *pair)
    sess.profile(True)
    for g in (1, 0, 2):  # (group order is the caller's business)
        mine = gor == g
        assert mine.any() and not mine.all()
        ref.upload_records(rec[mine], 0.0)
        ref.set_sg_plan(*plans[g])
        want = ref.savgol()
        sess.savgol_group(g, gor, g)
        got = sess.download_filtered()
        member = _slices(rec, mine, len(pool))
        assert got[member].tobytes() == want[member].tobytes(), (kind, g)
        expected = np.where(member, want, expected)
        assert got.tobytes() == expected.tobytes(), (kind, g)  # the others' samples and the gaps as they were
    report = sess.profile_report()
    sess.profile(False)
    assert kernel in report, sorted(report)
    if kind != "ragged":  # (5, 2) .. (11, 2) all take the span kernel; the plan of set_sg_plan is untouched
        assert "k_savgol<group>" not in report
    assert expected.tobytes() != base.tobytes() and sess.savgol().tobytes() == base.tobytes()


def test_savgol_group_general_route_on_uniform_records_and_errors(sess, ref):
    rec, pool, gor, _plans = T.split_run("span")
    sess.upload_pool(pool)  # a new pool: the twin is gone, the first group call zeroes it
    sess.upload_records(rec, 0.0)
    sess.store_sg_plan(3, 21, 4)  # no integer route: one wave per record over the uniform table
    with pytest.raises(ValueError, match="plan slot must be in"):
        sess.savgol_group(_lib.MAX_HIT_GROUPS, gor, 0)
    with pytest.raises(_lib.WfaError, match="holds no plan"):
        sess.savgol_group(7, gor, 0)
    with pytest.raises(ValueError, match="one group index per uploaded record"):
        sess.savgol_group(3, gor[:-1], 0)
    sess.savgol_group(3, gor, 1)
    got = sess.download_filtered()
    ref.upload_pool(pool)
    ref.upload_records(rec[gor == 1], 0.0)
    ref.set_sg_plan(21, 4)
    want = ref.savgol()
    member = _slices(rec, gor == 1, len(pool))
    assert got[member].tobytes() == want[member].tobytes() and not got[~member].any()
    sess.savgol_group(3, gor, 5)  # a group without a record writes nothing
    assert sess.download_filtered().tobytes() == got.tobytes()


# ---- 2. peak_chain(fixed_baseline) against the static chain -----------------------------------------------------------
def _static_rows(run, ranges="c5", **extra):
    rec, pool, hit_kw = run
    ctx = SimpleContext(T.config(ranges, hit_kw, **extra), {"records": rec, "wave_pool": pool}, plugins=hip_default())
    return ctx.get_data("run", "s1_s2")


def test_peak_chain_with_a_fixed_baseline_column_equals_the_static_chain(sess):
    rec, pool, hit_kw = U.run("ragged")
    col = T.fixed_column(rec, T.BASELINE_CC)
    assert np.count_nonzero(~np.isnan(col)) == 6
    sess.upload_pool(pool)
    sess.upload_records(rec, 0.0)
    sess.set_sg_plan(11, 2)
    sess.savgol(download=False)
    assert sess.find_peaks(_lib.SRC_F32, download=False, **hit_kw) == 32
    plain = sess.peak_chain(**U.C5_RANGES)
    for ranges in sorted(T.RANGE_SETS):
        want = _static_rows(U.run("ragged"), ranges, wave_pool_filtered={})  # basic_features' channel_config alone
        got = sess.peak_chain(fixed_baseline=col, **T.RANGE_SETS[ranges])
        assert got.dtype == S1_S2_CLASSIFIER_DTYPE and got.tobytes() == want.tobytes(), ranges
        oracle = T.restate(rec, pool, hit_kw, {}, T.BASELINE_CC, T.RANGE_SETS[ranges])["s1_s2"]
        assert got.tobytes() == oracle.tobytes(), ranges
    assert got.tobytes() != sess.peak_chain(**T.AREA_RANGES).tobytes()
    # the column is an argument of one call: nothing of it stays behind; NaN everywhere = none
    assert sess.peak_chain(**U.C5_RANGES).tobytes() == plain.tobytes()
    assert sess.peak_chain(fixed_baseline=np.full(len(rec), np.nan), **U.C5_RANGES).tobytes() == plain.tobytes()
    assert sess.peak_chain(_lib.SRC_RAW, _lib.SRC_F32, fixed_baseline=col, **U.C5_RANGES).tobytes() == \
        _static_rows(U.run("ragged"), wave_pool_filtered={}, basic_features={"channel_config": T.BASELINE_CC,
                                                                              "use_filtered": True}).tobytes()
    with pytest.raises(ValueError, match="one entry per record"):
        sess.peak_chain(fixed_baseline=col[:-1], **U.C5_RANGES)


# ---- 3. the stream with both options on -------------------------------------------------------------------------------
def _stream(run, streaming_config, ranges="c5", **extra):
    rec, pool, hit_kw = run
    ctx = SimpleContext(T.config(ranges, hit_kw, **extra), {"records": rec, "wave_pool": pool})
    outs = list(HipS1S2Stream().compute(ctx, "run", streaming_config=streaming_config))
    assert len(outs) == -(-len(rec) // streaming_config["chunk_size"])
    return np.concatenate([o.data for o in outs])


@pytest.mark.parametrize("parallel", [False, True])
@pytest.mark.parametrize("chunk_size", T.CHUNK_SIZES)
def test_stream_equals_the_reference_fixture(chunk_size, parallel):
    fx = T.load()
    got = _stream(U.run("ragged"), {"chunk_size": chunk_size, "parallel": parallel, "max_workers": 2})
    want = fx["s1_s2_c5"]
    assert len(want) == 22 and got.dtype == want.dtype and got.tobytes() == want.tobytes()
    if chunk_size in (7, 1000):  # the range set the fixed baselines move labels under
        got = _stream(U.run("ragged"), {"chunk_size": chunk_size, "parallel": parallel, "max_workers": 2}, "area")
        assert got.tobytes() == fx["s1_s2_area"].tobytes()
        assert not np.array_equal(got["label"], fx["labels_area_no_fixed"])


@pytest.mark.parametrize("name,chunk_size", [("ragged", 7), ("uniform", 64)])
def test_stream_equals_the_static_chain(name, chunk_size):
    run = U.run("ragged") if name == "ragged" else T.mixed_uniform()
    want = _static_rows(run)
    plain = _static_rows(run, wave_pool_filtered={}, basic_features={})
    assert len(want) > 10 and want.tobytes() != plain.tobytes()  # the settings are seen
    for parallel in (False, True):
        got = _stream(run, {"chunk_size": chunk_size, "parallel": parallel, "max_workers": 2})
        assert got.tobytes() == want.tobytes(), (name, parallel)
    if name == "ragged":
        assert want.tobytes() == T.load()["s1_s2_c5"].tobytes()


@pytest.mark.parametrize("name,chunk_size", [("ragged", 7), ("uniform", 64)])
def test_stream_sources_equal_the_static_chain(name, chunk_size):
    run = U.run("ragged") if name == "ragged" else T.mixed_uniform()
    cfg = {"chunk_size": chunk_size, "parallel": False}
    both = {"waveform_width": {"use_filtered": True}, "width_use_filtered": True,
            "basic_features": {"channel_config": T.BASELINE_CC, "use_filtered": True}, "features_use_filtered": True}
    want = _static_rows(run, **both)
    assert len(want) > 5 and _stream(run, cfg, **both).tobytes() == want.tobytes()
    stream = {"filter_source": "wave_pool_filtered", "baseline_source": "basic_features", "use_filtered": False}
    raw = {"hit": {"use_filtered": False}, "s1_s2_stream": stream, "waveform_width": {"use_filtered": True},
           "width_use_filtered": True}
    want_raw = _static_rows(run, **raw)
    assert len(want_raw) > 5 and want_raw.tobytes() != want.tobytes()
    assert _stream(run, cfg, **raw).tobytes() == want_raw.tobytes()


# ---- 4. one session, two chunks: nothing of the first chunk's twin shows in the second ---------------------------------
def test_reused_session_shows_no_filtered_samples_of_the_previous_chunk():
    rec, pool, _hit_kw = U.run("ragged")
    fx = T.load()
    groups = np.array([T.GROUP_OF_CHANNEL.get(int(c), 0) for c in rec["channel"]], dtype=np.int32)

    def stage(sess, lo, hi):
        part = rec[lo:hi].copy()
        first = int(part["wave_offset"].min())
        last = int((part["wave_offset"] + part["event_length"]).max())
        part["wave_offset"] -= first
        part["record_id"] -= lo
        sess.upload_pool(np.ascontiguousarray(pool[first:last]))
        sess.upload_records(part, 0.0)
        for g in np.unique(groups[lo:hi]):
            key = T.KEYS[g]
            if key[0] == "SG":
                sess.store_sg_plan(int(g), key[1], key[2])
                sess.savgol_group(int(g), groups[lo:hi], int(g))
            else:
                sess.sosfiltfilt_group(*design_bw(*key[1:]), groups[lo:hi], int(g))
        return first, last

    with DeviceSession(0) as sess:
        first, last = stage(sess, 0, 16)
        assert set(groups[:16].tolist()) == {0, 1, 2, 3}
        assert np.array_equal(sess.download_filtered(), fx["wave_pool_filtered"][first:last])
        assert set(groups[16:25].tolist()) == {0, 1, 3}  # no record of group 2 here
        first2, last2 = stage(sess, 16, 25)
        assert last2 - first2 < last - first  # the same device buffer, not grown
        got = sess.download_filtered()
        assert np.array_equal(got, fx["wave_pool_filtered"][first2:last2])
        gaps = ~_slices(rec[16:25], np.ones(9, dtype=bool), len(pool))[first2:last2]
        assert gaps.any() and not got[gaps].any()
    # the stream on a pool of one session: every chunk reuses it
    ctx = SimpleContext(T.config(), {"records": rec, "wave_pool": pool})
    dp = DevicePool(device_ids=[0], max_sessions=1)
    outs = list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config={"chunk_size": 7, "parallel": False}))
    dp.close()
    assert np.concatenate([o.data for o in outs]).tobytes() == fx["s1_s2_c5"].tobytes()
