"""df_events and df_paired on the GPU: every case of tests/golden/legacy_events_df.npz, a 1.25 M-row run against the host
route, equal timestamps, and the device memory of the grouping pass."""

import warnings

import numpy as np
import pandas as pd
import pytest

from tests import events_util as E
from waveformanalysis_amd.device import DeviceSession
from waveformanalysis_amd.event_grouping import group_multi_channel_hits
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipDataFramePlugin, HipGroupedEventsPlugin, HipPairedEventsPlugin

pytestmark = pytest.mark.gpu

Z = E.load()
CASES = E.case_names(Z)


def _plugins():
    return (HipDataFramePlugin(), HipGroupedEventsPlugin(), HipPairedEventsPlugin())


@pytest.mark.parametrize("case", CASES)
def test_df_events_and_df_paired_match_reference(case):
    ctx = E.make_context(Z, case, plugins=_plugins())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        events = ctx.get_data(E.RUN_ID, "df_events")
        paired = ctx.get_data(E.RUN_ID, "df_paired")
    E.assert_frame_matches(events, Z, f"{case}/df_events")
    E.assert_frame_matches(paired, Z, f"{case}/df_paired")


def _run(rows: int, seed: int, tick_ps: int = 1):
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.exponential(1e6, rows)).astype(np.int64) // tick_ps * tick_ps
    perm = rng.permutation(rows)
    return pd.DataFrame({
        "timestamp": ts[perm],
        "area": rng.uniform(0, 4000, rows).astype(np.float32),
        "height": rng.uniform(5, 400, rows).astype(np.float32),
        "board": np.zeros(rows, np.int16),
        "channel": rng.integers(0, 16, rows).astype(np.int16),
    })


def _paired_restated(events: pd.DataFrame, tw: float, n_channels: int, s: int) -> dict:
    """EventAnalyzer.pair_events restated on the concatenated ragged columns of a host-route frame."""
    keep = events["dt/ns"].to_numpy() <= tw
    off_t, ts = E.ragged_flat(events["timestamps"])
    off_a, ar = E.ragged_flat(events["areas"])
    off_h, he = E.ragged_flat(events["heights"])
    out = {"delta_t": ((ts[off_t[1:] - 1] - ts[off_t[:-1]]) / 1000.0)[keep]}
    for i in range(n_channels):
        for name, off, flat in (("area_ch", off_a, ar), ("height_ch", off_h, he)):
            lens = np.diff(off)
            col = np.full(len(lens), np.nan)
            col[lens > i] = flat[off[:-1][lens > i] + i]
            out[f"{name}{s + i}"] = col[keep]
    return out


def test_million_rows_against_host_route():
    df = _run(1_250_000, 11)
    ctx = SimpleContext({"time_window_ns": 60.0, "df_events": {"time_window_ns": 100.0}, "n_channels": 3},
                        {"df": df}, _plugins())
    events = ctx.get_data("run", "df_events")
    paired = ctx.get_data("run", "df_paired")
    want = group_multi_channel_hits(df, 100.0, session=False)
    assert len(events) == len(want) > 1_000_000 and (want["n_hits"] > 1).any()
    scalar = ["event_id", "t_min", "t_max", "dt/ns", "n_hits"]
    pd.testing.assert_frame_equal(events[scalar], want[scalar], check_dtype=True)
    for col in ("channels", "areas", "heights", "timestamps"):
        off, flat = E.ragged_flat(want[col])
        E.assert_ragged_equal(events[col], off, flat, col)
    restated = _paired_restated(want, 60.0, 3, 6)
    assert list(paired.columns) == list(want.columns) + list(restated)
    assert 0 < len(paired) < len(want)
    for col, values in restated.items():
        np.testing.assert_array_equal(paired[col].to_numpy(), values, err_msg=col)


def test_equal_timestamps_grouped_as_multisets():
    df = _run(200_000, 12, tick_ps=400_000)  # many rows share a timestamp, several rows share a channel in an event
    assert df["timestamp"].duplicated().sum() > 10_000
    ctx = SimpleContext({"df_events": {"time_window_ns": 250.0}}, {"df": df}, _plugins())
    events = ctx.get_data("run", "df_events")
    want = group_multi_channel_hits(df, 250.0, session=False)
    pd.testing.assert_series_equal(events["n_hits"], want["n_hits"])
    got_rows = _event_rows(events)
    want_rows = _event_rows(want)
    np.testing.assert_array_equal(got_rows, want_rows)
    for ch in events["channels"].to_list()[:5000]:
        assert np.all(np.diff(ch) >= 0)


def _event_rows(events: pd.DataFrame) -> np.ndarray:
    """(event, channel, timestamp, area, height) of every row, sorted inside each event: the events as multisets."""
    off, ch = E.ragged_flat(events["channels"])
    ev = np.repeat(np.arange(len(off) - 1), np.diff(off))
    ts = E.ragged_flat(events["timestamps"])[1]
    ar = E.ragged_flat(events["areas"])[1]
    he = E.ragged_flat(events["heights"])[1]
    rows = np.stack([ev.astype(np.float64), ch.astype(np.float64), ts.astype(np.float64), ar, he], axis=1)
    return rows[np.lexsort((he, ar, ts, ch, ev))]


def test_grouping_scratch_is_linear_in_rows():
    """The pointer-jumping stage keeps two (n+1)-entry int32 levels: the whole pass holds ~112 bytes per row
    (inputs, sort keys and permutations included), where log2(n) levels would add 4 * 25 = 100 more at 2^25 rows."""
    n = (1 << 25) - 1000
    rng = np.random.default_rng(13)
    ts = np.cumsum(rng.integers(1, 2_000_000, n)).astype(np.int64)
    ch = rng.integers(0, 16, n).astype(np.int64)
    with DeviceSession(0) as sess:
        order, bounds = sess.group_multi_channel(ts, ch, 1e5)
        held = sess.scratch_bytes()
        assert sess.scratch_bytes() == held  # a query: nothing is freed
    assert len(order) == n and bounds[-1] == n and len(bounds) > n // 4
    assert held <= 128 * n, held / n
