"""hit_threshold with use_filtered=True, fuse_filter=True on runs whose channels resolve to different filter settings
(wave_pool_filtered's filter_type / channel_config): one device pass per setting over the resident pool, the rows merged
on the device (wfa_hits_enqueue_groups).

Fixture: tests/golden/c5_fused_groups.npz (tests/golden/make_fused_groups_golden.py) -- three runs of 4 channels x 40
records, channels interleaved: "a" L = 128 (in-place streaming), "b" L = 100 (padded), "c" ragged 20..300 samples (general
route); channel 0 SG(11, 2), 1 SG(7, 3), 2 SG(21, 4), 3 Butterworth; per-channel thresholds on channels 1 and 3."""

import functools

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests import stream_groups_util as U
from tests.fused_groups_util import (FILTER_CC, HIT_CC, KEYS, RUNS, context, group_column, group_plan, host_merge, load_run,
                                     run_groups, stage_groups, thresholds_of)
from waveformanalysis_amd import _lib
from waveformanalysis_amd import multidevice as MD
from waveformanalysis_amd.device import DeviceSession, device_count
from waveformanalysis_amd.dtypes import THRESHOLD_HIT_DTYPE
from waveformanalysis_amd.filter_engine import design_bw
from waveformanalysis_amd.plugins.threshold_hit import records_pass

pytestmark = pytest.mark.gpu

FLOAT_RTOL = 1e-6  # hit rows against the reference, as tests/test_hip_parity.py
FUSED = {"use_filtered": True, "fuse_filter": True, "channel_config": HIT_CC}


@pytest.fixture(scope="module")
def sess():
    with DeviceSession(0) as s:
        yield s


def _plugin_rows(run, hit_cfg, filter_cfg, devices=None):
    ctx = context(run, hit_cfg, filter_cfg, devices=devices)
    try:
        return ctx.get_data("run", "hit_threshold")
    finally:
        MD.close_sharded_runs(ctx)


# ---- 1. plugin parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", RUNS)
def test_plugin_matches_reference_and_unfused_route(tag):
    run = load_run(tag)
    got = _plugin_rows(run, FUSED, {"channel_config": FILTER_CC})
    G.assert_struct_equal(got, run["hits"], float_rtol=FLOAT_RTOL, what=f"run {tag}: fused groups vs reference")
    ctx = context(run, {"use_filtered": True, "channel_config": HIT_CC}, {"channel_config": FILTER_CC})
    np.testing.assert_array_equal(ctx.get_data("run", "wave_pool_filtered"), run["wave_pool_filtered"])
    G.assert_struct_equal(got, ctx.get_data("run", "hit_threshold"), float_rtol=FLOAT_RTOL,
                          what=f"run {tag}: fused groups vs the unfused route")
    # (what a fused pass that ignores the channel_config returns is stored too, and differs)
    assert len(run["hits_uniform"]) != len(got) or got.tobytes() != run["hits_uniform"].tobytes()


def test_run_wide_butterworth_is_filtered_on_the_device():
    """filter_type="BW" for the whole run: one group, no merge; equal to the unfused route."""
    run = load_run("c")
    bw = {"filter_type": "BW", "lowcut": 0.01, "highcut": 0.2, "fs": 0.5}
    got = _plugin_rows(run, FUSED, bw)
    want = context(run, {"use_filtered": True, "channel_config": HIT_CC}, bw).get_data("run", "hit_threshold")
    assert len(want) > 100
    G.assert_struct_equal(got, want, float_rtol=FLOAT_RTOL, what="run-wide Butterworth")


# ---- 2. the merge alone -------------------------------------------------------------------------------------------------
def _isolated(sess, run, thr, *, option=None):
    """(device-merged table, host merge of the passes' downloads)."""
    rec, pool = run["records"], run["wave_pool"]
    plan = group_plan(rec)
    if option:
        sess.set_option(option, True)
    try:
        sess.upload_pool(pool)
        parts, n = run_groups(sess, rec, thr, plan)
        got = np.empty(n, dtype=THRESHOLD_HIT_DTYPE)
        sess.download_hits(got)
    finally:
        if option:
            sess.set_option(option, False)
    return got, host_merge(rec, parts), parts


@pytest.mark.parametrize("option", [None, "no_runs32", "no_span", "no_pad", "no_fast"])
@pytest.mark.parametrize("tag", RUNS)
def test_device_merge_equals_host_merge(sess, tag, option):
    run = load_run(tag)
    got, want, parts = _isolated(sess, run, thresholds_of(run["records"]), option=option)
    assert all(len(p) >= 20 for p in parts) and len(want) > 300
    assert got.tobytes() == want.tobytes()
    # and the merged table is the reference's: the groups are disjoint, every record's rows come from its own pass
    G.assert_struct_equal(got, run["hits"], float_rtol=FLOAT_RTOL, what=f"run {tag} {option}")


@pytest.mark.parametrize("tag", RUNS)
def test_device_merge_with_unordered_record_ids(sess, tag):
    run = load_run(tag)
    rec = run["records"].copy()
    rec["record_id"] = np.random.default_rng(5).permutation(len(rec)) * 7 + 3
    got, want, _parts = _isolated(sess, dict(run, records=rec), thresholds_of(rec))
    assert len(want) == len(run["hits"])
    assert got.tobytes() == want.tobytes()


def test_device_merge_with_an_empty_pass_and_with_no_rows(sess):
    run = load_run("a")
    rec = run["records"]
    thr = thresholds_of(rec)
    thr[rec["channel"] == 1] = 1e9  # the SG(7, 3) group finds nothing
    got, want, parts = _isolated(sess, run, thr)
    assert sorted(len(p) == 0 for p in parts) == [False, False, False, True] and len(want) > 100
    assert got.tobytes() == want.tobytes()
    got, want, parts = _isolated(sess, run, np.full(len(rec), 1e9))
    assert len(got) == len(want) == 0 and all(len(p) == 0 for p in parts)
    # the row count of an empty table sizes the next pass's speculative launch: that pass is still complete
    sess.upload_records(rec, thresholds_of(rec))
    sess.set_sg_plan(11, 2)
    G.assert_struct_equal(sess.threshold_hits(_lib.SRC_SG_FUSED), run["hits_uniform"], float_rtol=FLOAT_RTOL,
                          what="single pass after an empty merge")


# ---- 3. the masked passes keep the state of the context -------------------------------------------------------------------
def test_masked_passes_keep_baselines_and_the_padded_shadow(sess):
    run = load_run("b")
    rec, pool = run["records"], run["wave_pool"]
    blank = rec.copy()
    blank["baseline"] = np.nan  # a pass that read the uploaded baselines would find nothing
    sess.upload_pool(pool)
    sess.upload_records(blank, 10.0)
    sess.set_sg_plan(7, 3)  # L = 100: windows up to 9 read the padded shadow (L % 16 >= W / 2), 11 and above do not
    sess.profile(True)
    try:
        first = sess.fused_baseline_filter_hits((0, 40))
        # two masked passes under the same plan, no baseline window: the baselines the first pass left, the shadow it built
        sess.store_sg_plan(2, 7, 3)
        sess.store_sg_plan(3, 7, 3)
        sess.hits_enqueue_groups([(_lib.SRC_SG_FUSED, 2), (_lib.SRC_SG_FUSED, 3)], rec["channel"] % 2, 2, 2)
        second = sess._fill_hits(sess.hits_wait())
        report = sess.profile_report()
    finally:
        sess.profile(False)
    assert len(first) > 100 and first.tobytes() == second.tobytes()
    assert report["k_pad_rows (once per upload)"][1] == 1 and report["k_grp_mask"][1] == 2, report
    # two groups whose passes both read the shadow: built once, not once per group
    even = rec["channel"] % 2 == 0
    sess.profile(True)
    try:
        got = records_pass(sess, blank, 10.0, np.where(even, 0, 1).astype(np.int32), source=_lib.SRC_SG_FUSED, sg=None,
                           fuse_baseline=(0, 40), le=2, re=2, groups=[("SG", 7, 3), ("SG", 5, 2)])
        report = sess.profile_report()
    finally:
        sess.profile(False)
    assert report["k_pad_rows (once per upload)"][1] == 1 and report["k_sg_mask_span16<baseline>"][1] == 2, report
    assert len(got) > 100 and np.all(np.diff(got["record_id"]) >= 0)
    # the fixture's configuration: four passes, one shadow
    plan = group_plan(rec)
    sess.profile(True)
    try:
        got = records_pass(sess, blank, thresholds_of(rec), group_column(plan), source=_lib.SRC_SG_FUSED, sg=None,
                           fuse_baseline=(0, 40), le=2, re=2, groups=[k for k, _m in plan])
        report = sess.profile_report()
    finally:
        sess.profile(False)
    assert report["k_pad_rows (once per upload)"][1] == 1, report
    assert any(name.startswith("k_hit_rows_merge_scatter") for name in report), report
    # (the fixture's baselines are the mean of the first 40 samples)
    G.assert_struct_equal(got, run["hits"], float_rtol=FLOAT_RTOL, what="group loop with fuse_baseline")


# ---- 4. resident consumers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "c"])
def test_resident_stages_read_the_merged_table(sess, tag):
    run = load_run(tag)
    rec = run["records"]
    plan = group_plan(rec)
    sess.upload_pool(run["wave_pool"])
    n = records_pass(sess, rec, thresholds_of(rec), group_column(plan), source=_lib.SRC_SG_FUSED, sg=None,
                     fuse_baseline=None, le=2, re=2, groups=[k for k, _m in plan], download=False)
    rows = np.empty(n, dtype=THRESHOLD_HIT_DTYPE)
    sess.download_hits(rows)
    assert n == len(run["hits"])
    sess.hit_rows_source("hits")
    order, offset = sess.hit_merge_clusters_resident(n, 200.0, 4000.0)
    want_order, want_offset = sess.hit_merge_clusters(rows["timestamp"], rows["position"], rows["edge_start"],
                                                      rows["edge_end"], rows["dt"], rows["board"], rows["channel"], 200.0, 4000.0)
    np.testing.assert_array_equal(order, want_order)
    np.testing.assert_array_equal(offset, want_offset)
    assert 1 < len(offset) - 1 < n
    got = sess.group_hit_windows_resident(n, 1000.0)
    want = sess.group_hit_windows(rows["timestamp"], rows["position"], rows["edge_start"], rows["edge_end"], rows["dt"],
                                  rows["board"], rows["channel"], rows["record_id"], 1000.0)
    for name in want:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)


# ---- 5. one group: today's path -------------------------------------------------------------------------------------------
def test_single_group_takes_the_single_pass(sess):
    run = load_run("a")
    rec, pool = run["records"], run["wave_pool"]
    thr = thresholds_of(rec)
    sess.upload_pool(pool)
    sess.upload_records(rec, thr)
    sess.set_sg_plan(7, 3)
    want = sess.threshold_hits(_lib.SRC_SG_FUSED)
    # one group, and two groups of which the second has no record here (a shard): the single pass either way
    first = np.zeros(len(rec), dtype=np.int32)
    for groups in ([("SG", 7, 3)], [("SG", 7, 3), ("SG", 21, 4)]):
        sess.profile(True)
        try:
            got = records_pass(sess, rec, thr, first, source=_lib.SRC_SG_FUSED, sg=None, fuse_baseline=None, le=2, re=2,
                               groups=groups)
            report = sess.profile_report()
        finally:
            sess.profile(False)
        assert not [name for name in report if name.startswith("k_hit_rows_merge")], report
        assert report["k_sg_runs32"][1] == 1, report
        assert len(got) > 300 and got.tobytes() == want.tobytes()
    # the plugin with a uniform configuration: the same bytes
    got = _plugin_rows(run, FUSED, {"sg_window_size": 7, "sg_poly_order": 3,
                                    "channel_config": {"0:2": {"sg_window_size": 7}}})
    assert got.tobytes() == want.tobytes()


# ---- 6. several devices ---------------------------------------------------------------------------------------------------
def _ids(which):
    if which == "three_on_0":
        return [0, 0, 0]
    n = device_count()
    if n < 2:
        pytest.skip(f"{n} device visible: the every-device set needs two or more")
    return list(range(n))


@pytest.mark.parametrize("which", [pytest.param("three_on_0", id="0,0,0"), pytest.param("all", id="all-visible")])
@pytest.mark.parametrize("tag", RUNS)
def test_sharded_run_is_byte_identical(tag, which):
    ids = _ids(which)
    run = load_run(tag)
    for fuse_baseline in (None, (0, 40)):
        cfg = dict(FUSED, fuse_baseline=fuse_baseline)
        want = _plugin_rows(run, cfg, {"channel_config": FILTER_CC})
        got = _plugin_rows(run, cfg, {"channel_config": FILTER_CC}, devices=ids)
        assert len(want) > 300 and got.tobytes() == want.tobytes(), (tag, fuse_baseline)
    # the first shard holds records of one group only (its single pass), the others mix all four
    rec = run["records"].copy()
    first = MD.split_records(rec, 3)[0]
    rec["channel"][first.r0:first.r1] = 0
    one = dict(run, records=rec)
    want = _plugin_rows(one, FUSED, {"channel_config": FILTER_CC})
    got = _plugin_rows(one, FUSED, {"channel_config": FILTER_CC}, devices=[0, 0, 0])
    assert len(want) > 200 and got.tobytes() == want.tobytes()


# ---- 7. the baseline window through the grouped call ------------------------------------------------------------------------
@functools.cache
def _window_oracle(tag):
    """The oracle's rows of a run under FILTER_CC / HIT_CC with every baseline the mean of samples [0, min(40, length))."""
    run = load_run(tag)
    rec, pool = run["records"].copy(), run["wave_pool"]
    rec["baseline"] = [pool[o : o + min(40, n)].astype(np.float64).mean() for o, n in zip(rec["wave_offset"], rec["event_length"])]
    return O.threshold_hits(rec, U.oracle_filtered(rec, pool, list(KEYS)), thresholds=thresholds_of(rec), left_extension=2,
                            right_extension=2)


@pytest.mark.parametrize("tag", RUNS)
def test_baseline_window_through_the_grouped_call(tag):
    """Window (0, 40) on the queued grouped call over records whose Savitzky-Golay groups are uploaded with NaN
    baselines -- a pass that did not get the window finds nothing there -- cold, twice warm, and once behind a call that
    found nothing (its bounds are exceeded, hits_wait redoes).  Each time: the host merge of the groups' single passes
    (fused_baseline_filter_hits for the Savitzky-Golay groups, baseline_mean + threshold_hits for the Butterworth one),
    byte for byte; the oracle's rows under window baselines; and the reference's rows.  The fixture's baselines are the
    mean of the first 40 samples the run was generated with; run "c" cut seven records to 20..33 samples afterwards,
    where the window ends with the record, so the reference's own rows are compared on the records that hold the whole
    window (all of "a" and "b", 153 of 160 in "c") and the oracle's on all of them."""
    run = load_run(tag)
    rec, pool = run["records"], run["wave_pool"]
    blank = rec.copy()
    blank["baseline"] = np.nan
    plan, thr = group_plan(rec), thresholds_of(rec)
    whole = rec["record_id"][rec["event_length"] >= 40]
    assert len(whole) >= len(rec) - 7

    def equals_reference(rows, what):
        G.assert_struct_equal(rows, _window_oracle(tag), float_rtol=FLOAT_RTOL, what=what + " vs oracle")
        want_rows = run["hits"][np.isin(run["hits"]["record_id"], whole)]
        assert len(want_rows) >= len(run["hits"]) - 8
        G.assert_struct_equal(rows[np.isin(rows["record_id"], whole)], want_rows, float_rtol=FLOAT_RTOL, what=what)

    with DeviceSession(0) as s:  # its own context: the first grouped call is a cold one
        s.upload_pool(pool)
        s.upload_records(blank[plan[3][1]])
        s.sosfiltfilt(*design_bw(*KEYS[3][1:]), download=False)
        parts = []
        for key, mask in plan:
            s.upload_records(blank, np.where(mask, thr, np.inf))
            if key[0] == "SG":
                s.set_sg_plan(key[1], key[2])
                parts.append(s.fused_baseline_filter_hits((0, 40)))
            else:
                s.baseline_mean(0, 40, update_records=True)
                parts.append(s.threshold_hits(_lib.SRC_F32))
        want = host_merge(rec, parts)
        assert all(len(p) >= 20 for p in parts) and len(want) > 300
        equals_reference(want, f"run {tag}: single passes with the window")
        # the Butterworth records alone get a baseline on the host (its pass reads the uploaded ones); the Savitzky-Golay
        # records stay NaN, so their rows can only come from the window of the grouped call
        s.upload_records(blank)
        sg_blank = blank.copy()
        sg_blank["baseline"][plan[3][1]] = s.baseline_mean(0, 40)[plan[3][1]]
        assert np.isnan(sg_blank["baseline"]).sum() == int((~plan[3][1]).sum())

        def grouped(thresholds, window=(0, 40)):
            s.upload_records(sg_blank, thresholds)
            stage_groups(s, KEYS, group_column(plan), baseline_window=window)
            return s._fill_hits(s.hits_wait())

        s.upload_pool(pool)  # (drops the float32 twin of the single passes)
        for call in ("cold", "warm", "warm again"):
            got = grouped(thr)
            assert got.tobytes() == want.tobytes(), (tag, call)
            equals_reference(got, f"run {tag} {call}: grouped call with the window")
        assert len(grouped(np.full(len(rec), 1e9))) == 0
        got = grouped(thr)  # every group's launch was sized by a pass without rows
        assert got.tobytes() == want.tobytes(), (tag, "after an empty call")
        equals_reference(got, f"run {tag}: grouped call after an empty one")
        # and without the window only the Butterworth records, the ones with a baseline, give rows
        got = grouped(thr, window=(0, 0))
        assert got.tobytes() == parts[3].tobytes()


# ---- 8. the grouped call only reads the context's own plan, thresholds and options ------------------------------------------
def test_grouped_calls_leave_the_plan_thresholds_and_options_of_the_context():
    """One session, plan (7, 3) and the records' own thresholds set once; `want` is the plain pass under them.  Every
    kind of grouped call over slots (11, 2) -- streaming route, queued when warm -- and (21, 4) -- general route, completed
    -- is followed by the same plain pass, which must give `want` byte for byte: a call that is waited for, a warm one
    nobody waits for (the plain pass ends it), one refused in the middle of its validation (slot 5 holds no plan), and one
    whose wait takes the exact redo.  Run "a" has a few hundred rows and never outgrows the smallest row bound (4096), so
    the last case uploads U.exceeding_run() once (the run of test_exceeded_bound_is_redone_exactly) and gets its calls
    that find nothing from a group column that owns no record: no upload stands between a grouped call and the plain
    pass that checks it.  The redo is seen from outside (k_grp_mask: two queued passes + two exact ones) and leaves
    no_speculate false: a plain warm hits_enqueue stays pending."""
    run = load_run("a")
    rec, pool = run["records"], run["wave_pool"]
    groups = [(_lib.SRC_SG_FUSED, 0), (_lib.SRC_SG_FUSED, 1)]

    def parity(records):
        return np.ascontiguousarray(records["channel"] % 2, dtype=np.int32)

    with DeviceSession(0) as s:
        def plain():
            return s.threshold_hits(_lib.SRC_SG_FUSED).tobytes()

        s.upload_pool(pool)
        s.upload_records(rec, thresholds_of(rec))
        s.set_sg_plan(7, 3)
        want = plain()
        assert len(want) > 300 * THRESHOLD_HIT_DTYPE.itemsize
        s.store_sg_plan(0, 11, 2)
        s.store_sg_plan(1, 21, 4)
        # cold, waited for
        s.hits_enqueue_groups(groups, parity(rec))
        merged = s._fill_hits(s.hits_wait())
        assert len(merged) > 100 and merged.tobytes() != want
        assert plain() == want
        # warm, not waited for: the plain pass ends the queued one
        s.hits_enqueue_groups(groups, parity(rec))
        assert s.hits_pending()
        assert plain() == want and not s.hits_pending()
        # refused after group 0 has been accepted
        gor = parity(rec)
        bad = (_lib.C.c_int32 * 4)(_lib.SRC_SG_FUSED, 0, _lib.SRC_SG_FUSED, 5)
        assert s._lib.wfa_hits_enqueue_groups(s._h, 2, bad, gor.ctypes.data, 0, 0, 2, 2, 0) == _lib.WFA_E_STATE
        assert "slot 5" in _lib.last_error()
        assert plain() == want
        # the exact redo
        big, big_pool = U.exceeding_run()
        s.upload_pool(big_pool)
        s.upload_records(big, thresholds_of(big))
        want = plain()
        for _call in range(2):      # every record unowned: both groups find nothing, their next launches are sized for 4096 rows
            s.hits_enqueue_groups(groups, np.full(len(big), -1, dtype=np.int32))
            assert s.hits_wait() == 0
        s.profile(True)
        try:
            s.hits_enqueue_groups(groups, parity(big))
            assert s.hits_pending()
            redone = s._fill_hits(s.hits_wait())
            report = s.profile_report()
        finally:
            s.profile(False)
        assert report["k_grp_mask"][1] == 4, report
        assert len(redone) > 2 * (4096 + 4096 // 8)
        assert plain() == want
        s.hits_enqueue(_lib.SRC_SG_FUSED)
        assert s.hits_pending()
        assert s._fill_hits(s.hits_wait()).tobytes() == want
        s.hits_enqueue_groups(groups, parity(big))      # and the bounds the redo left behind hold: the same table, standing
        assert s._fill_hits(s.hits_wait()).tobytes() == redone.tobytes()


# ---- 9. error contract ----------------------------------------------------------------------------------------------------
def test_error_codes_of_the_new_calls():
    run = load_run("a")
    rec, pool = run["records"], run["wave_pool"]
    with DeviceSession(0) as s:
        lib, h = s._lib, s._h
        s.upload_pool(pool)
        s.upload_records(rec, 10.0)
        s.store_sg_plan(0, 11, 2)
        s.store_sg_plan(1, 11, 2)
        groups = (_lib.C.c_int32 * 4)(_lib.SRC_SG_FUSED, 0, _lib.SRC_SG_FUSED, 1)
        gor = np.ascontiguousarray(rec["channel"] % 2, dtype=np.int32)
        assert lib.wfa_hits_enqueue_groups(h, 2, groups, gor.ctypes.data, -1, 40, 2, 2, 0) == _lib.WFA_E_INVALID
        assert "baseline window start" in _lib.last_error()
        assert lib.wfa_hits_enqueue_groups(h, 2, groups, gor.ctypes.data, -1, -1, 2, 2, 0) == 0  # an empty window: none
        n = s.hits_wait()
        assert n > 100
        first = s._fill_hits(n)
        # a merged table carries no record index: the next call stashes the rows of its own passes, never the table
        assert lib.wfa_hits_enqueue_groups(h, 2, groups, gor.ctypes.data, 0, 0, 2, 2, 0) == 0
        assert s.hits_wait() == n and s._fill_hits(n).tobytes() == first.tobytes()
        # the stash is scratch
        held = s.scratch_bytes()
        assert held >= n * 64
        s.release_scratch()
        assert s.scratch_bytes() == 0
        assert len(s._fill_hits(n)) == n  # the merged table stays
