"""hit_threshold with use_filtered=True, fuse_filter=True on runs whose channels resolve to different filter settings
(wave_pool_filtered's filter_type / channel_config): one device pass per setting over the resident pool, the rows merged
on the device (wfa_set_thresholds, wfa_hit_rows_merge_*).

Fixture: tests/golden/c5_fused_groups.npz (tests/golden/make_fused_groups_golden.py) -- three runs of 4 channels x 40
records, channels interleaved: "a" L = 128 (in-place streaming), "b" L = 100 (padded), "c" ragged 20..300 samples (general
route); channel 0 SG(11, 2), 1 SG(7, 3), 2 SG(21, 4), 3 Butterworth; per-channel thresholds on channels 1 and 3."""

import numpy as np
import pytest

from tests import golden_util as G
from tests.fused_groups_util import (FILTER_CC, HIT_CC, RUNS, context, group_plan, host_merge, load_run, run_groups,
                                     thresholds_of)
from waveformanalysis_amd import _lib
from waveformanalysis_amd import multidevice as MD
from waveformanalysis_amd.device import DeviceSession, device_count
from waveformanalysis_amd.dtypes import THRESHOLD_HIT_DTYPE
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


# ---- 3. set_thresholds keeps the state of the context ---------------------------------------------------------------------
def test_set_thresholds_keeps_baselines_and_the_padded_shadow(sess):
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
        sess.set_thresholds(np.full(len(rec), 10.0))
        second = sess.threshold_hits(_lib.SRC_SG_FUSED)  # no baseline window: the baselines the first pass left
        report = sess.profile_report()
    finally:
        sess.profile(False)
    assert len(first) > 100 and first.tobytes() == second.tobytes()
    assert report["k_pad_rows (once per upload)"][1] == 1, report
    # two groups whose passes both read the shadow: built once, not once per group
    even = rec["channel"] % 2 == 0
    sess.profile(True)
    try:
        got = records_pass(sess, blank, 10.0, even, ~even, source=_lib.SRC_SG_FUSED, sg=None, fuse_baseline=(0, 40), le=2,
                           re=2, groups=[("SG", 7, 3), ("SG", 5, 2)])
        report = sess.profile_report()
    finally:
        sess.profile(False)
    assert report["k_pad_rows (once per upload)"][1] == 1 and report["k_sg_mask_span16<baseline>"][1] == 2, report
    assert len(got) > 100 and np.all(np.diff(got["record_id"]) >= 0)
    # the fixture's configuration: four passes, one shadow
    plan = group_plan(rec)
    sess.profile(True)
    try:
        got = records_pass(sess, blank, thresholds_of(rec), *[m for _k, m in plan], source=_lib.SRC_SG_FUSED, sg=None,
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
    n = records_pass(sess, rec, thresholds_of(rec), *[m for _k, m in plan], source=_lib.SRC_SG_FUSED, sg=None,
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
    one = np.ones(len(rec), dtype=bool)
    for groups, group_masks in (([("SG", 7, 3)], [one]), ([("SG", 7, 3), ("SG", 21, 4)], [one, ~one])):
        sess.profile(True)
        try:
            got = records_pass(sess, rec, thr, *group_masks, source=_lib.SRC_SG_FUSED, sg=None, fuse_baseline=None, le=2, re=2,
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


# ---- 7. error contract ----------------------------------------------------------------------------------------------------
def test_error_codes_of_the_new_calls():
    run = load_run("a")
    rec, pool = run["records"], run["wave_pool"]
    with DeviceSession(0) as s:
        lib, h = s._lib, s._h
        thr = np.full(len(rec), 10.0)
        ptr = thr.ctypes.data
        assert lib.wfa_set_thresholds(h, ptr, len(rec)) == _lib.WFA_E_STATE  # no records
        assert lib.wfa_hit_rows_merge_add(h) == _lib.WFA_E_STATE  # no open set
        n = _lib.C.c_int64(-1)
        assert lib.wfa_hit_rows_merge_end(h, _lib.C.byref(n)) == _lib.WFA_E_STATE
        s.upload_pool(pool)
        s.upload_records(rec, 10.0)
        assert lib.wfa_set_thresholds(h, ptr, len(rec) - 1) == _lib.WFA_E_INVALID  # wrong count
        assert lib.wfa_set_thresholds(h, ptr, len(rec)) == 0
        assert lib.wfa_hit_rows_merge_begin(h) == 0
        assert lib.wfa_hit_rows_merge_add(h) == _lib.WFA_E_STATE  # no pass yet
        assert lib.wfa_hit_rows_merge_end(h, _lib.C.byref(n)) == 0 and n.value == 0  # an empty set: 0 rows
        assert len(s._fill_hits(0)) == 0
        assert lib.wfa_hit_rows_merge_add(h) == _lib.WFA_E_STATE  # the set is closed
        # a merged table carries no record index: it cannot be added to another set
        s.set_sg_plan(11, 2)
        with s.merged_hit_rows() as merge:
            assert s.threshold_hits(_lib.SRC_SG_FUSED, download=False) > 100
            merge.add()
        assert merge.n_hits > 100
        assert lib.wfa_hit_rows_merge_begin(h) == 0
        assert lib.wfa_hit_rows_merge_add(h) == _lib.WFA_E_STATE
        # the stash is scratch
        held = s.scratch_bytes()
        assert held >= merge.n_hits * 64
        s.release_scratch()
        assert s.scratch_bytes() == 0
        assert lib.wfa_hit_rows_merge_add(h) == _lib.WFA_E_STATE  # the open set went with the scratch
        assert len(s._fill_hits(merge.n_hits)) == merge.n_hits  # the merged table stays
