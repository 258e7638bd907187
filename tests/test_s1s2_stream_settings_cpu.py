"""HipS1S2Stream under per-channel settings without a GPU: what a chunk hands to its session with
filter_source="wave_pool_filtered" and baseline_source="basic_features" (through a recording double), run-wide group
numbering, the single-setting shortcut, the refusals, the declared entry points, and the reference's fixture against a
numpy restatement of the chain."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest

from tests import s1s2_chain_util as U
from tests import s1s2_settings_util as T
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DevicePool
from waveformanalysis_amd.dtypes import S1_S2_CLASSIFIER_DTYPE
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipBasicFeaturesPlugin, HipWavePoolFilteredPlugin
from waveformanalysis_amd.s1s2_stream import HipS1S2Stream

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SERIAL = {"parallel": False}


class RecordingSession:
    """Stands where a DeviceSession would: keeps every call with its arguments, computes nothing."""

    def __init__(self, device_id, calls):
        self.device_id, self.calls = device_id, calls
        self.n = 0

    def upload_pool(self, pool):
        self.calls.append(("upload_pool", pool.copy()))

    def upload_records(self, records, thresholds=10.0, polarity=None):
        self.n = len(records)
        self.calls.append(("upload_records", records.copy()))

    def set_sg_plan(self, window, order):
        self.calls.append(("set_sg_plan", (window, order)))

    def savgol(self, download=True):
        self.calls.append(("savgol", download))

    def sosfiltfilt(self, sos, zi, padlen, download=True):
        self.calls.append(("sosfiltfilt", (np.asarray(sos).shape, int(padlen), download)))

    def store_sg_plan(self, slot, window, order):
        self.calls.append(("store_sg_plan", (slot, window, order)))

    def savgol_group(self, slot, group_of_record, group):
        self.calls.append(("savgol_group", (slot, np.array(group_of_record), group)))

    def sosfiltfilt_group(self, sos, zi, padlen, group_of_record, group):
        self.calls.append(("sosfiltfilt_group", (np.asarray(sos).shape, int(padlen), np.array(group_of_record), group)))

    def find_peaks(self, source, download=True, **kw):
        self.calls.append(("find_peaks", dict(source=source, download=download, **kw)))
        return self.n

    def peak_chain(self, width_source, feature_source, **kw):
        self.calls.append(("peak_chain", dict(width_source=width_source, feature_source=feature_source, **kw)))
        return np.zeros(0, dtype=S1_S2_CLASSIFIER_DTYPE)

    def close(self):
        pass


def recording_pool():
    calls = []
    pool = DevicePool(device_ids=[0], session_factory=lambda dev: RecordingSession(dev, calls))
    pool.calls = calls
    return pool


def _context(plugins=(), **config):
    rec, pool, _kw = U.run("ragged")
    return rec, pool, SimpleContext(T.config(**config), {"records": rec, "wave_pool": pool}, plugins=plugins)


def _per_chunk(calls):
    """The call list cut at every upload_pool."""
    out = []
    for c in calls:
        if c[0] == "upload_pool":
            out.append([])
        out[-1].append(c)
    return out


def _groups(records):
    return np.array([T.GROUP_OF_CHANNEL.get(int(c), 0) for c in records["channel"]], dtype=np.int32)


def _filter_names(present):
    names = []
    for g in present:
        names += ["sosfiltfilt_group"] if T.KEYS[g][0] == "BW" else ["store_sg_plan", "savgol_group"]
    return names


@pytest.mark.parametrize("chunk_size", T.CHUNK_SIZES)
def test_call_sequence_group_numbering_and_baseline_slice(chunk_size):
    rec, pool, ctx = _context()
    dp = recording_pool()
    outs = list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config={"chunk_size": chunk_size, **SERIAL}))
    bounds = list(range(0, len(rec), chunk_size))
    assert len(outs) == len(bounds)
    with_samples = [lo for lo in bounds if rec["event_length"][lo : lo + chunk_size].sum() > 0]
    chunks = _per_chunk(dp.calls)
    assert len(chunks) == len(with_samples)
    fixed = T.fixed_column(rec, T.BASELINE_CC)
    shapes = set()
    for lo, calls in zip(with_samples, chunks):
        part = rec[lo : lo + chunk_size]
        want = _groups(part)
        present = sorted(set(want.tolist()))  # the groups of the RUN that have a record here, in group order
        shapes.add(tuple(present))
        assert [c[0] for c in calls] == ["upload_pool", "upload_records"] + _filter_names(present) + ["find_peaks", "peak_chain"]
        first = int(part["wave_offset"].min())
        assert np.array_equal(calls[0][1], pool[first : int((part["wave_offset"] + part["event_length"]).max())])
        assert np.array_equal(calls[1][1]["wave_offset"], part["wave_offset"] - first)
        assert np.array_equal(calls[1][1]["record_id"], np.arange(len(part)))
        filters = iter(calls[2:-2])
        for g in present:
            key = T.KEYS[g]
            if key[0] == "BW":
                shape, padlen, gor, group = next(filters)[1]
                assert shape == (2, 6) and padlen == 15 and group == g  # order 2 band pass: 2 sections, 3 * (2 * 2 + 1)
            else:
                assert next(filters)[1] == (g, key[1], key[2])  # slot g of the run holds group g's pair
                slot, gor, group = next(filters)[1]
                assert slot == g and group == g
            assert gor.dtype == np.int32 and np.array_equal(gor, want)
        peaks, chain = calls[-2][1], calls[-1][1]
        assert peaks["source"] == _lib.SRC_F32 and peaks["download"] is False
        assert chain["record_id_base"] == lo and (chain["width_source"], chain["feature_source"]) == (_lib.SRC_RAW, _lib.SRC_RAW)
        assert chain["fixed_baseline"].dtype == np.float64
        assert chain["fixed_baseline"].tobytes() == fixed[lo : lo + chunk_size].tobytes()  # (NaN = none)
    if chunk_size == 1:
        # a chunk that holds only the Butterworth group, chunks that lack groups, and slices without a fixed baseline
        assert (3,) in shapes and (0,) in shapes and (1,) in shapes and (2,) in shapes
        only_bw = [c for c in chunks if [x[0] for x in c[2:-2]] == ["sosfiltfilt_group"]]
        assert only_bw and all(c[2][1][3] == 3 for c in only_bw)
        assert any(np.all(np.isnan(c[-1][1]["fixed_baseline"])) for c in chunks)
    if chunk_size == 7:
        assert any(len(s) < len(T.KEYS) for s in shapes) and any(len(s) > 1 for s in shapes)
    if chunk_size >= 40:
        assert shapes == {(0, 1, 2, 3)}
    dp.close()


def test_groups_are_numbered_over_the_run_in_plan_order():
    rec, _pool, ctx = _context()
    plugin = HipS1S2Stream()
    plan = plugin._run_plan(plugin._configure(ctx), ctx, "run")
    assert plan.keys == T.KEYS and np.array_equal(plan.lookup(rec)[0], _groups(rec))
    assert plugin._run_plan(plugin._configure(ctx), ctx, "run") is plan  # resolved once per run
    # a chunk of the run's last records alone numbers its groups as the run does
    assert np.array_equal(plan.lookup(rec[33:])[0], _groups(rec)[33:])
    assert plan.lookup(rec[33:])[1].tobytes() == T.fixed_column(rec, T.BASELINE_CC)[33:].tobytes()
    other = SimpleContext(T.config(sg_window_size=9), ctx._data)
    assert plugin._run_plan(plugin._configure(other), other, "run").keys[0] == ("SG", 9, 2)
    # the registered plugin is the one asked; without one a fresh plugin stands in
    reg = SimpleContext(T.config(), ctx._data, plugins=[HipWavePoolFilteredPlugin(), HipBasicFeaturesPlugin()])
    assert plugin._run_plan(plugin._configure(reg), reg, "run").keys == T.KEYS
    with pytest.raises(ValueError, match="a chunk holds a \\(board, channel\\) the run's records do not"):
        stray = rec[:2].copy()
        stray["channel"] = 77
        plan.lookup(stray)


def test_no_fixed_baseline_in_the_run_hands_none_over():
    _rec, _pool, ctx = _context(basic_features={"channel_config": {"0:99": {"fixed_baseline": 5.0}}})
    dp = recording_pool()
    list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config={"chunk_size": 7, **SERIAL}))
    chains = [c[1] for c in dp.calls if c[0] == "peak_chain"]
    assert len(chains) == 6 and all(c.get("fixed_baseline") is None for c in chains)
    dp.close()
    # the options are independent: fixed baselines with the stream's own filter
    _rec, _pool, ctx = _context(s1_s2_stream={"baseline_source": "basic_features"}, wave_pool_filtered={})
    dp = recording_pool()
    list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config={"chunk_size": 40, **SERIAL}))
    assert [c[0] for c in dp.calls] == ["upload_pool", "upload_records", "set_sg_plan", "savgol", "find_peaks", "peak_chain"]
    assert dp.calls[2][1] == (11, 2) and dp.calls[-1][1]["fixed_baseline"] is not None
    dp.close()


def test_single_setting_takes_the_ungrouped_calls():
    same = {f"0:{c}": {"sg_window_size": 7, "sg_poly_order": 3} for c in range(14)}
    for wpf, want in (({}, ("set_sg_plan", (11, 2))), ({"sg_window_size": 9}, ("set_sg_plan", (9, 2))),
                      ({"channel_config": same}, ("set_sg_plan", (7, 3))), (dict(T.BW), ("sosfiltfilt", ((2, 6), 15, False)))):
        _rec, _pool, ctx = _context(wave_pool_filtered=wpf)
        dp = recording_pool()
        list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config={"chunk_size": 40, **SERIAL}))
        names = [c[0] for c in dp.calls]
        if want[0] == "set_sg_plan":
            assert names == ["upload_pool", "upload_records", "set_sg_plan", "savgol", "find_peaks", "peak_chain"]
            assert dp.calls[3][1] is False
        else:
            assert names == ["upload_pool", "upload_records", "sosfiltfilt", "find_peaks", "peak_chain"]
        assert dp.calls[2] == want
        dp.close()


def test_no_filter_call_when_no_stage_reads_filtered_samples():
    _rec, _pool, ctx = _context(use_filtered=False)
    dp = recording_pool()
    list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config={"chunk_size": 40, **SERIAL}))
    assert [c[0] for c in dp.calls] == ["upload_pool", "upload_records", "find_peaks", "peak_chain"]
    assert dp.calls[2][1]["source"] == _lib.SRC_RAW
    dp.close()
    _rec, _pool, ctx = _context(use_filtered=False, width_use_filtered=True)
    dp = recording_pool()
    list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config={"chunk_size": 40, **SERIAL}))
    names = [c[0] for c in dp.calls]
    assert names == ["upload_pool", "upload_records"] + _filter_names([0, 1, 2, 3]) + ["find_peaks", "peak_chain"]
    assert dp.calls[-2][1]["source"] == _lib.SRC_RAW and dp.calls[-1][1]["width_source"] == _lib.SRC_F32
    dp.close()


def test_new_refusals_happen_before_any_session_call():
    rec, pool, ctx = _context()
    dp = recording_pool()
    cfg = {"chunk_size": 16, **SERIAL}
    data = {"records": rec, "wave_pool": pool}
    for name, value in (("sg_window_size", 7), ("filter_type", "BW"), ("filter_order", 2)):
        with pytest.raises(ValueError, match="contradict filter_source='wave_pool_filtered'"):
            HipS1S2Stream(device_pool=dp, filter_source="wave_pool_filtered", **{name: value})
        with pytest.raises(ValueError, match="contradict filter_source='wave_pool_filtered'"):
            list(HipS1S2Stream(device_pool=dp, **{name: value}).compute(ctx, "run", streaming_config=cfg))
    with pytest.raises(ValueError, match="filter_source must be one of"):
        HipS1S2Stream(filter_source="hit")
    with pytest.raises(ValueError, match="baseline_source must be one of"):
        HipS1S2Stream(baseline_source="fixed")
    many = {f"0:{c}": {"sg_window_size": 11 + 2 * c, "sg_poly_order": 2} for c in range(1, 10)}  # + the run-wide (11, 2)
    over = SimpleContext(T.config(wave_pool_filtered={"channel_config": many}), data)
    with pytest.raises(ValueError, match=r"s1_s2_stream: the run resolves to 10 distinct filter settings, the grouped "
                                         rf"filter takes at most {_lib.MAX_HIT_GROUPS}"):
        list(HipS1S2Stream(device_pool=dp).compute(over, "run", streaming_config=cfg))
    chunk = next(HipS1S2Stream()._data_to_chunks(rec, "run"))
    with pytest.raises(ValueError, match="distinct filter settings"):
        HipS1S2Stream(device_pool=dp).compute_chunk(chunk, over, "run")
    # plan_filter_groups' messages for a bad per-channel setting
    bad = SimpleContext(T.config(wave_pool_filtered={"channel_config": {"0:3": {"sg_window_size": 5, "sg_poly_order": 5}}}), data)
    with pytest.raises(ValueError, match=r"SG 多项式阶数 \(5\) 必须小于窗口大小 \(5\)"):
        list(HipS1S2Stream(device_pool=dp).compute(bad, "run", streaming_config=cfg))
    bad = SimpleContext(T.config(wave_pool_filtered={"channel_config": {"0:3": {"filter_type": "FIR"}}}), data)
    with pytest.raises(ValueError, match="不支持的滤波器类型: FIR"):
        list(HipS1S2Stream(device_pool=dp).compute(bad, "run", streaming_config=cfg))
    # the deprecated option stays outside in both modes
    old = SimpleContext(T.config(**{"basic_features.fixed_baseline": {"0:1": 8000.0}}), data)
    with pytest.raises(ValueError, match="outside the stream"):
        list(HipS1S2Stream(device_pool=dp).compute(old, "run", streaming_config=cfg))
    assert dp.calls == []
    dp.close()


def test_defaults_still_refuse_and_each_option_lifts_its_own_refusal():
    rec, pool, _ctx = _context()
    dp = recording_pool()
    cfg = {"chunk_size": 16, **SERIAL}
    data = {"records": rec, "wave_pool": pool}
    assert HipS1S2Stream.options["filter_source"].default == "own"
    assert HipS1S2Stream.options["baseline_source"].default == "records"
    filt, base = {"wave_pool_filtered": {"channel_config": T.FILTER_CC}}, {"basic_features": {"channel_config": T.BASELINE_CC}}
    for config in (filt, base, {**filt, **base},
                   {**filt, **base, "s1_s2_stream": {"filter_source": "wave_pool_filtered"}},
                   {**filt, **base, "s1_s2_stream": {"baseline_source": "basic_features"}}):
        with pytest.raises(ValueError, match="outside the stream"):
            list(HipS1S2Stream(device_pool=dp).compute(SimpleContext(config, data), "run", streaming_config=cfg))
    assert dp.calls == []
    for config, kw in ((filt, {"filter_source": "wave_pool_filtered"}), (base, {"baseline_source": "basic_features"})):
        list(HipS1S2Stream(device_pool=dp, **kw).compute(SimpleContext(config, data), "run", streaming_config=cfg))
        assert [c[0] for c in dp.calls].count("peak_chain") == 3
        del dp.calls[:]
    dp.close()


def test_header_and_binding_declare_the_entry_points():
    header = open(os.path.join(REPO, "include", "wfa_hip.h")).read()
    for name in ("wfa_savgol_group", "wfa_peak_chain_count_fixed"):
        assert re.search(rf"^int {name}\(wfa_ctx\* ctx", header, flags=re.M), name
        assert name in _lib.SIGNATURES
    assert int(re.search(r"#define WFA_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 10
    assert len(_lib.SIGNATURES["wfa_savgol_group"][1]) == 4
    fixed, plain = _lib.SIGNATURES["wfa_peak_chain_count_fixed"][1], _lib.SIGNATURES["wfa_peak_chain_count"][1]
    assert fixed[:-1] == plain[:-1] + [_lib._p] and fixed[-1] is plain[-1]  # the column, then n_rows
    assert "no fixed baseline)" not in header


# ---- the reference's fixture ------------------------------------------------------------------------------------------
def test_fixture_holds_what_the_issue_states():
    fx = T.load()
    assert fx["config"]["wave_pool_filtered"]["channel_config"] == T.FILTER_CC
    assert fx["config"]["basic_features"]["channel_config"] == T.BASELINE_CC and fx["config"]["hit"] == U.RAGGED_HIT
    rows = fx["s1_s2_c5"]
    assert rows.dtype == S1_S2_CLASSIFIER_DTYPE and U.counts(rows) == (0, 15, 7)
    assert U.counts(U.oracle_rows("ragged", U.C5_RANGES)) == (0, 17, 9)  # without the settings
    for g in range(len(T.KEYS)):  # every filter group has a hit
        assert any(T.GROUP_OF_CHANNEL.get(int(c), 0) == g for c in fx["hit"]["channel"]), g
    assert np.count_nonzero(fx["s1_s2_area"]["label"] != fx["labels_area_no_fixed"]) >= 1


@pytest.mark.parametrize("ranges", sorted(T.RANGE_SETS))
def test_numpy_restatement_equals_the_fixture(ranges):
    fx, mine = T.load(), T.restated(ranges)
    for name in ("wave_pool_filtered", "hit", "waveform_width", "basic_features"):
        assert fx[name].dtype == mine[name].dtype and fx[name].tobytes() == mine[name].tobytes(), name
    assert T.same_rows(fx[f"s1_s2_{ranges}"], mine["s1_s2"])


@pytest.mark.parametrize("variant", ["filter_ignored", "filter_swapped", "baseline_ignored", "baseline_wrong_channel"])
def test_wrong_chains_differ_from_the_fixture(variant):
    fx = T.load()
    for ranges in sorted(T.RANGE_SETS):
        assert not T.same_rows(fx[f"s1_s2_{ranges}"], T.restated(ranges, variant)["s1_s2"]), ranges
    stage = "wave_pool_filtered" if variant.startswith("filter") else "basic_features"
    assert fx[stage].tobytes() != T.restated("c5", variant)[stage].tobytes()
    if variant == "baseline_ignored":  # the labels move under the range set made for it
        assert not np.array_equal(fx["s1_s2_area"]["label"], T.restated("area", variant)["s1_s2"]["label"])
