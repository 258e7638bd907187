"""df, df_events and df_paired without a GPU: HipDataFramePlugin and HipPairedEventsPlugin against the reference's
frames (tests/golden/legacy_events_df.npz), HipGroupedEventsPlugin with a session that groups in the host order, the error
texts, the empty run and the hip_full() profile."""

import gc
import warnings

import numpy as np
import pandas as pd
import pytest

from tests import events_util as E
from waveformanalysis_amd.event_grouping import MULTI_CHANNEL_COLUMNS
from waveformanalysis_amd.plugins import (
    HipDataFramePlugin,
    HipGroupedEventsPlugin,
    HipPairedEventsPlugin,
    hip_full,
)
from waveformanalysis_amd.plugins import event_analysis as EA

Z = E.load()
CASES = E.case_names(Z)


def _plugins():
    return (HipDataFramePlugin(), HipGroupedEventsPlugin(), HipPairedEventsPlugin())


def test_fixture_covers_the_issue_cases():
    assert len(CASES) >= 15
    sizes = {c: len(Z[f"{c}/df_paired/index"]) for c in CASES}
    events = {c: len(Z[f"{c}/df_events/index"]) for c in CASES}
    assert sizes["pair_drop_all"] == 0 and 0 < sizes["pair_drop_some"] < events["pair_drop_some"]
    assert events["window_0"] > events["records_plain"] > events["window_5000"]


@pytest.mark.parametrize("case", CASES)
def test_df_matches_reference(case):
    ctx = E.make_context(Z, case, plugins=_plugins())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = ctx.get_data(E.RUN_ID, "df")
    E.assert_frame_matches(got, Z, f"{case}/df")


@pytest.mark.parametrize("case", CASES)
def test_df_events_and_df_paired_match_reference(case):
    ctx = E.make_context(Z, case, plugins=_plugins(), pool=E.HostGroupingPool())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        events = ctx.get_data(E.RUN_ID, "df_events")
        paired = ctx.get_data(E.RUN_ID, "df_paired")
    E.assert_frame_matches(events, Z, f"{case}/df_events")
    E.assert_frame_matches(paired, Z, f"{case}/df_paired")


@pytest.mark.parametrize("case", CASES)
def test_df_paired_from_a_frame_built_elsewhere(case):
    """A df_events frame the plugin did not build (a cache reload): the ragged columns are concatenated."""
    events = E.expected_frame(Z, f"{case}/df_events")
    ctx = E.make_context(Z, case, plugins=(HipPairedEventsPlugin(),))
    ctx._data["df_events"] = events
    E.assert_frame_matches(ctx.get_data(E.RUN_ID, "df_paired"), Z, f"{case}/df_paired")


def test_df_paired_charges_peaks_fallback():
    events = E.expected_frame(Z, "records_plain/df_events").rename(columns={"areas": "charges", "heights": "peaks"})
    got = EA.pair_events(events, 100.0)
    want = E.expected_frame(Z, "records_plain/df_paired")
    for col in ("area_ch6", "height_ch6", "area_ch7", "height_ch7", "delta_t"):
        pd.testing.assert_series_equal(got[col], want[col], check_dtype=True)


@pytest.mark.parametrize("name, source, cut, config, wrap", [
    ("len_records", "records", 3, {"df": {"wave_source": "records"}, "basic_features": {"wave_source": "records"}}, False),
    ("len_st", "st_waveforms", 2, {}, False),
    ("bf_not_records", "records", 0, {"df": {"wave_source": "records"}}, False),
    ("bf_not_array", "st_waveforms", 0, {}, True),
])
def test_df_error_texts(name, source, cut, config, wrap):
    table = Z["table/rec"]
    table = table[: len(table) - cut]
    bf = [Z["bf"]] if wrap else Z["bf"]
    ctx = E.EventsContext(config, {source: table, "basic_features": bf})
    with pytest.raises(ValueError) as info:
        HipDataFramePlugin().compute(ctx, E.RUN_ID)
    assert str(info.value) == str(Z[f"err/{name}"])


def test_df_dependencies_follow_wave_source():
    p = HipDataFramePlugin()
    assert p.resolve_depends_on(E.EventsContext()) == ["st_waveforms", "basic_features"]
    assert p.resolve_depends_on(E.EventsContext({"df": {"use_filtered": True}})) == ["filtered_waveforms", "basic_features"]
    assert p.resolve_depends_on(E.EventsContext({"df": {"wave_source": "records", "use_filtered": True}})) == \
        ["records", "basic_features"]
    assert (p.provides, p.version, p.uses_run_config) == ("df", "1.7.0+hip1", True)
    assert set(p.options) == {"use_filtered", "wave_source", "gain_adc_per_pe"}


def test_df_sort_is_stable_on_equal_timestamps():
    rec = Z["table/rec"].copy()
    rec["timestamp"] = rec["timestamp"] // 10_000_000 * 10_000_000  # many ties
    ctx = E.EventsContext({}, {"st_waveforms": rec, "basic_features": Z["bf"]})
    got = HipDataFramePlugin().compute(ctx, E.RUN_ID)
    np.testing.assert_array_equal(got.index.to_numpy(), np.argsort(rec["timestamp"], kind="stable"))


def test_empty_run():
    rec = Z["table/rec"][:0]
    ctx = E.EventsContext({}, {"st_waveforms": rec, "basic_features": Z["bf"][:0]}, _plugins())
    ctx.wfa_device_pool = E.HostGroupingPool()
    df = ctx.get_data(E.RUN_ID, "df")
    assert len(df) == 0 and list(df.columns)[:8] == ["timestamp", "record_id", "area", "height", "amp",
                                                     "max_abs_diff", "board", "channel"]
    events = ctx.get_data(E.RUN_ID, "df_events")
    assert list(events.columns) == MULTI_CHANNEL_COLUMNS and len(events) == 0
    paired = ctx.get_data(E.RUN_ID, "df_paired")
    assert list(paired.columns) == MULTI_CHANNEL_COLUMNS and len(paired) == 0


def test_df_events_options_and_ignored_keys():
    p = HipGroupedEventsPlugin()
    assert p.options["time_window_ns"].default == 100.0 and p.depends_on == ["df"]
    ctx = E.make_context(Z, "records_plain", plugins=_plugins(), pool=E.HostGroupingPool())
    ctx.config.update({"use_numba": False, "n_processes": 4})
    E.assert_frame_matches(ctx.get_data(E.RUN_ID, "df_events"), Z, "records_plain/df_events")


def test_flat_memo_follows_the_frame():
    ctx = E.make_context(Z, "records_plain", plugins=_plugins(), pool=E.HostGroupingPool())
    events = ctx.get_data(E.RUN_ID, "df_events")
    assert EA._recall(events) is not None
    assert EA._recall(events.copy()) is None
    n = len(EA._flat_memo)
    ctx._results.clear()
    del events
    gc.collect()
    assert len(EA._flat_memo) == n - 1


def test_hip_full_covers_cpu_default():
    # the provides names of the reference's cpu_default() profile, minus raw_files (the input files themselves)
    cpu_default = {
        "basic_features", "df", "df_events", "df_paired", "filtered_waveforms", "hit", "hit_grouped",
        "hit_merge_clusters", "hit_merged", "hit_merged_components", "hit_threshold", "records", "s1_s2",
        "st_waveforms", "wave_pool", "wave_pool_filtered", "waveform_width", "waveform_width_integral",
    }
    provides = [p.provides for p in hip_full()]
    assert len(provides) == len(set(provides))
    assert set(provides) - {"signal_peaks_stream"} == cpu_default
