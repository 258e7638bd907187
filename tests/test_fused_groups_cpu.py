"""The host side of the fused hit pass over several filter groups: the group plan of the fixture's configuration, the
order of the calls records_pass makes on a session (a recording stub: no device), the single-group shortcut, a shard's
empty groups, and the reference's messages for an invalid per-channel filter setting."""

import numpy as np
import pytest

from tests.fused_groups_util import (FILTER_CC, HIT_CC, KEYS, context, group_column, group_plan, load_run,
                                     thresholds_of)
from waveformanalysis_amd import _lib
from waveformanalysis_amd.dtypes import THRESHOLD_HIT_DTYPE
from waveformanalysis_amd.filter_engine import plan_fused_groups
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipThresholdHitPlugin, HipWavePoolFilteredPlugin
from waveformanalysis_amd.plugins.threshold_hit import records_pass


class RecordingSession:
    """Stands in for DeviceSession: records every call records_pass makes, computes nothing."""

    def __init__(self):
        self.calls = []

    def _note(self, name, *args):
        self.calls.append((name,) + args)

    def upload_records(self, records, thresholds=10.0):
        self._note("upload_records", len(records), None if np.ndim(thresholds) == 0 else np.array(thresholds))

    def set_sg_plan(self, window, order):
        self._note("set_sg_plan", int(window), int(order))

    def sosfiltfilt_group(self, sos, zi, padlen, group_of_record, group):
        self._note("sosfiltfilt_group", int(sos.shape[0]), int(padlen), np.array(group_of_record), int(group))

    def store_sg_plan(self, slot, window, order):
        self._note("store_sg_plan", int(slot), int(window), int(order))

    def hits_enqueue_groups(self, groups, group_of_record, le=2, re=2, max_len=0, baseline_window=(0, 0)):
        self._note("hits_enqueue_groups", [tuple(g) for g in groups], np.array(group_of_record), tuple(baseline_window))

    def hits_wait(self):
        self._note("hits_wait")
        return 12

    def baseline_mean(self, start, end, update_records=False):
        self._note("baseline_mean", int(start), int(end), update_records)

    def threshold_hits(self, source, le, re, max_len=0, download=True):
        self._note("threshold_hits", int(source), download)
        return 3 if not download else np.zeros(3, dtype=THRESHOLD_HIT_DTYPE)

    def fused_baseline_filter_hits(self, window, le, re, max_len=0, download=True):
        self._note("fused_baseline_filter_hits", tuple(window), download)
        return 3 if not download else np.zeros(3, dtype=THRESHOLD_HIT_DTYPE)

    def _fill_hits(self, n):
        self._note("fill_hits", n)
        return np.zeros(n, dtype=THRESHOLD_HIT_DTYPE)

    def names(self):
        return [c[0] for c in self.calls]


def _pass(sess, rec, plan, **kw):
    kw = {"source": _lib.SRC_SG_FUSED, "sg": None, "fuse_baseline": None, "le": 2, "re": 2, **kw}
    return records_pass(sess, rec, thresholds_of(rec), group_column(plan), groups=[k for k, _m in plan], **kw)


def test_plan_of_the_fixture_configuration():
    rec = load_run("a")["records"]
    ctx = context(load_run("a"), {"use_filtered": True, "fuse_filter": True, "channel_config": HIT_CC},
                  {"channel_config": FILTER_CC})
    plan = plan_fused_groups(ctx, ctx.get_plugin("wave_pool_filtered"), "run", rec)
    assert [key for key, _m in plan] == KEYS
    for (_key, mask), (_k, want) in zip(plan, group_plan(rec)):
        np.testing.assert_array_equal(mask, want)
    # no wave_pool_filtered plugin: the reference's defaults; a plugin without a channel_config: its run-wide options,
    # nothing per record
    assert plan_fused_groups(ctx, None, "run", rec) == [(("SG", 11, 2), None)]
    ctx = SimpleContext({"wave_pool_filtered": {"sg_window_size": 8, "sg_poly_order": 3}}, {}, [HipWavePoolFilteredPlugin()])
    assert plan_fused_groups(ctx, ctx.get_plugin("wave_pool_filtered"), "run", rec) == [(("SG", 9, 3), None)]
    # channels that resolve to one setting are one group
    ctx = SimpleContext({"wave_pool_filtered": {"channel_config": {"0:1": {"sg_window_size": 11}, "0:2": {"filter_order": 6}}}},
                        {}, [HipWavePoolFilteredPlugin()])
    plan = plan_fused_groups(ctx, ctx.get_plugin("wave_pool_filtered"), "run", rec)
    assert [key for key, _m in plan] == [("SG", 11, 2)] and plan[0][1].all()


def test_pass_order_and_group_column():
    rec = load_run("b")["records"]
    plan = group_plan(rec)
    thr = thresholds_of(rec)
    sess = RecordingSession()
    rows = _pass(sess, rec, plan)
    assert len(rows) == 12
    assert sess.names() == [
        "upload_records",                                        # one upload of the whole table, the records' own thresholds
        "store_sg_plan", "store_sg_plan", "store_sg_plan", "sosfiltfilt_group",  # per group, in order
        "hits_enqueue_groups", "hits_wait", "fill_hits"]
    calls = sess.calls
    assert calls[0][1] == len(rec)  # the whole table: the layout (and its padded shadow) stays
    np.testing.assert_array_equal(calls[0][2], thr)
    # the Butterworth filter call runs before the queued call and over the uploaded table: no second upload
    assert calls[4][:3] == ("sosfiltfilt_group", 4, 27) and calls[4][4] == 3
    assert sess.names().count("upload_records") == 1
    plans = [c[1:] for c in calls if c[0] == "store_sg_plan"]
    assert plans == [(0, 11, 2), (1, 7, 3), (2, 21, 4)]
    assert calls[5][1] == [(_lib.SRC_SG_FUSED, 0), (_lib.SRC_SG_FUSED, 1), (_lib.SRC_SG_FUSED, 2), (_lib.SRC_F32, 0)]
    assert calls[5][3] == (0, 0)
    # group_of_record is the plan's masks: record r can hit in the pass of its own group only
    for column in (calls[4][3], calls[5][2]):
        assert column.dtype == np.int32
        for g, (_key, mask) in enumerate(plan):
            np.testing.assert_array_equal(column == g, mask)
    # download=False leaves the merged table on the device and returns its row count
    sess = RecordingSession()
    assert _pass(sess, rec, plan, download=False) == 12 and "fill_hits" not in sess.names()
    # fuse_baseline: the window on the queued call for the Savitzky-Golay groups, one baseline_mean for the Butterworth pass
    sess = RecordingSession()
    _pass(sess, rec, plan, fuse_baseline=(0, 40))
    assert sess.names()[:2] == ["upload_records", "baseline_mean"] and sess.names()[-3:] == ["hits_enqueue_groups", "hits_wait", "fill_hits"]
    assert [c for c in sess.calls if c[0] == "baseline_mean"] == [("baseline_mean", 0, 40, True)]
    assert sess.calls[-3][3] == (0, 40)
    # without a Butterworth group nobody reads the uploaded baselines: no baseline_mean
    sg_only = rec[rec["channel"] != 3]
    sess = RecordingSession()
    _pass(sess, sg_only, group_plan(sg_only), fuse_baseline=(0, 40))
    assert "baseline_mean" not in sess.names() and sess.calls[-3][3] == (0, 40)


def test_single_group_shortcut_and_a_shards_empty_groups():
    rec = load_run("a")["records"]
    thr = thresholds_of(rec)
    # groups=None (what the plugin passes for one Savitzky-Golay setting): the calls of the single pass, nothing else
    sess = RecordingSession()
    records_pass(sess, rec, thr, source=_lib.SRC_SG_FUSED, sg=(7, 3), fuse_baseline=None, le=2, re=2)
    single = sess.names()
    assert single == ["upload_records", "set_sg_plan", "threshold_hits"]
    # a shard whose records all belong to one Savitzky-Golay group: the same calls, with the records' own thresholds
    one = rec[rec["channel"] == 1]
    sess = RecordingSession()
    _pass(sess, one, group_plan(one))
    assert sess.names() == single and sess.calls[1] == ("set_sg_plan", 7, 3)
    np.testing.assert_array_equal(sess.calls[0][2], thresholds_of(one))
    # a shard without Butterworth records skips that group (no filter call) and the groups it has no record of
    two = rec[(rec["channel"] == 0) | (rec["channel"] == 2)]
    sess = RecordingSession()
    _pass(sess, two, group_plan(two))
    assert sess.names() == ["upload_records", "store_sg_plan", "store_sg_plan", "hits_enqueue_groups", "hits_wait", "fill_hits"]
    assert [c[1:] for c in sess.calls if c[0] == "store_sg_plan"] == [(0, 11, 2), (2, 21, 4)]  # each key's run-wide slot
    assert sess.calls[3][1] == [(_lib.SRC_SG_FUSED, 0), (_lib.SRC_SG_FUSED, 2)]
    np.testing.assert_array_equal(sess.calls[3][2], two["channel"] // 2)  # renumbered to the groups that are left
    # only Butterworth records: filtered over the uploaded table, then the queued call with that one group
    bw = rec[rec["channel"] == 3]
    sess = RecordingSession()
    _pass(sess, bw, group_plan(bw))
    assert sess.names() == ["upload_records", "sosfiltfilt_group", "hits_enqueue_groups", "hits_wait", "fill_hits"]
    assert sess.calls[2][1] == [(_lib.SRC_F32, 0)] and not sess.calls[2][2].any()
    # the plugin takes the shortcut itself for a uniform configuration: no group arguments reach the pass
    seen = {}

    def route(context, plugin, records, pool, row_dtype, run_pass, per_record=(), **kw):
        seen["groups"], seen["sg"], seen["per_record"] = run_pass.keywords["groups"], run_pass.keywords["sg"], len(per_record)
        return np.zeros(0, dtype=THRESHOLD_HIT_DTYPE)

    from waveformanalysis_amd.plugins import _common as K

    for filter_cfg, want in (({"sg_window_size": 7, "sg_poly_order": 3}, (None, (7, 3), 1)),
                             ({"channel_config": FILTER_CC}, (KEYS, None, 2))):
        ctx = context(load_run("a"), {"use_filtered": True, "fuse_filter": True}, filter_cfg)
        original, K.records_route = K.records_route, route
        try:
            HipThresholdHitPlugin().compute(ctx, "run")
        finally:
            K.records_route = original
        assert (seen["groups"], seen["sg"], seen["per_record"]) == want


@pytest.mark.parametrize("setting, message", [
    ({"filter_type": "FIR"}, "不支持的滤波器类型: FIR"),
    ({"sg_window_size": 5, "sg_poly_order": 5}, r"SG 多项式阶数 \(5\) 必须小于窗口大小 \(5\)"),
    ({"sg_window_size": 0}, r"SG 窗口大小 \(0\) 必须大于 0"),
    ({"filter_type": "BW"}, r"highcut \(0.5\) 必须小于奈奎斯特频率 \(0.25\)"),  # the reference's own defaults
    ({"filter_type": "BW", "lowcut": 0.3, "highcut": 0.2, "fs": 1.0}, r"lowcut \(0.3\) 必须小于 highcut \(0.2\)"),
])
def test_invalid_per_channel_setting_raises_the_reference_message(setting, message):
    ctx = context(load_run("a"), {"use_filtered": True, "fuse_filter": True}, {"channel_config": {"0:2": setting}})
    with pytest.raises(ValueError, match=message):
        HipThresholdHitPlugin().compute(ctx, "run")
    # the same message as the unfused route's wave_pool_filtered
    with pytest.raises(ValueError, match=message):
        HipWavePoolFilteredPlugin().compute(ctx, "run")


def test_more_settings_than_the_grouped_pass_takes_is_refused_before_any_upload():
    run = load_run("a")
    rec = run["records"].copy()
    rec["channel"] = np.arange(len(rec)) % 9
    nine = {f"0:{c}": {"sg_window_size": 5 + 2 * c, "sg_poly_order": 2} for c in range(9)}
    ctx = context(dict(run, records=rec), {"use_filtered": True, "fuse_filter": True}, {"channel_config": nine})
    seen = []
    from waveformanalysis_amd.plugins import _common as K

    original, K.records_route = K.records_route, lambda *a, **kw: seen.append(a)
    try:
        with pytest.raises(ValueError, match=r"9 distinct filter settings, the grouped pass takes at most 8 .*fuse_filter=False"):
            HipThresholdHitPlugin().compute(ctx, "run")
    finally:
        K.records_route = original
    assert not seen  # nothing reached a session
