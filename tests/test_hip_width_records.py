"""waveform_width on the resident records + wave_pool / wave_pool_filtered (wave_source="records"): k_waveform_width's
records instantiation against the reference's rows (tests/golden/c5_width_records.npz), against the dense route on the
same samples, and as a stage of the records-only S1/S2 chain.  Every comparison is exact unless it says otherwise."""

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests import width_records_util as W
from tests.test_replay_cpu import load_fixture
from waveformanalysis_amd import _lib, replay
from waveformanalysis_amd.device import DeviceSession, default_pool
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import (
    HipBasicFeaturesPlugin,
    HipS1S2ClassifierPlugin,
    HipWaveformWidthPlugin,
    hip_default,
)

pytestmark = pytest.mark.gpu

S1S2_CFG = {"s1_width_range": (0.0, 80.0), "s2_width_range": (80.0, 5000.0), "s1_area_range": None,
            "s2_area_range": (500.0, 1e12)}  # the ranges of replay.c5_chain


def _records_widths(hits, records, pool, use_filtered, options):
    pool_name = "wave_pool_filtered" if use_filtered else "wave_pool"
    ctx = SimpleContext({"wave_source": "records", "use_filtered": use_filtered, **options},
                        {"hit": hits, "records": records, pool_name: pool})
    return HipWaveformWidthPlugin().compute(ctx, "run")


@pytest.mark.parametrize("pool_key", sorted(W.POOLS))
def test_fixture_parity(pool_key):
    """Ragged records (lengths 0, 1, 7, 8, 13, 17, 49, 50, 51, 64, 65, 800, 1500; offsets of every alignment, the last
    record ending at the last sample of a pool whose size is no multiple of 8): every hit table x option set."""
    d = W.load()
    pool = d[W.POOLS[pool_key]]
    for table in W.TABLES:
        hits = d[f"hit_{table}"]
        for k, options in enumerate(d["options"]):
            got = _records_widths(hits, d["records"], pool, pool_key == "f32", options)
            G.assert_struct_equal(got, d[f"w_{table}_{pool_key}_{k}"], what=f"{table} {pool_key} options {k}")
            if table == "crafted" and k == 0:  # the comparison above is not one of empty tables
                n = len(hits)
                assert 4 * len(got) >= n and 4 * (n - len(got)) >= n, (len(got), n)
                assert np.count_nonzero(got["rise_time_samples"]) >= 10
                assert np.count_nonzero(got["fall_time_samples"]) >= 10
    sess = default_pool().session()
    assert sess.holds_pool(pool) and sess.holds_records(d["records"])  # one pool upload, one records upload


def test_session_call_checks_its_inputs():
    d = W.load()
    hits = d["hit_crafted"]
    pos, rid = hits["position"], hits["record_id"]
    with DeviceSession(0) as sess:
        sess.upload_pool(d["wave_pool"])
        with pytest.raises(_lib.WfaError, match="records not uploaded"):
            sess.waveform_width_records(_lib.SRC_RAW, pos, rid)
        sess.upload_records(d["records"])
        with pytest.raises(_lib.WfaError, match="wave_pool_filtered"):
            sess.waveform_width_records(_lib.SRC_F32, pos, rid)
        with pytest.raises(ValueError, match="WFA_SRC_RAW or WFA_SRC_F32"):
            sess.waveform_width_records(_lib.SRC_SG_FUSED, pos, rid)
        with pytest.raises(ValueError, match="float division by zero"):
            sess.waveform_width_records(_lib.SRC_RAW, pos, rid, sampling_rate=0.0)
        with pytest.raises(ValueError, match="same length"):
            sess.waveform_width_records(_lib.SRC_RAW, pos, rid[:-1])
        rows, valid = sess.waveform_width_records(_lib.SRC_RAW, pos[:0], rid[:0])
        assert len(rows) == 0 and len(valid) == 0
        sess.profile(True)
        rows, valid = sess.waveform_width_records(_lib.SRC_RAW, pos, rid)
        assert list(sess.profile_report()) == ["k_waveform_width_rec"]
        G.assert_struct_equal(rows[valid][["peak_position", "peak_height", "total_width"]],
                              d["w_crafted_u16_0"][["peak_position", "peak_height", "total_width"]])
        assert not rows[~valid].view(np.uint8).any()  # dropped hits: all-zero rows


def test_config5_records_route_equals_dense_route_and_reference():
    d, rec, pool = load_fixture()
    hits = d["hit"]
    assert len(hits) == 4499 and len(d["waveform_width"]) == 4447
    st = replay.st_waveforms_from_records(rec, pool)
    dense = HipWaveformWidthPlugin().compute(SimpleContext({}, {"hit": hits, "st_waveforms": st}), "run")
    got = _records_widths(hits, rec, pool, False, {})
    G.assert_struct_equal(got, dense, what="records route vs dense route")
    assert got.tobytes() == dense.tobytes()
    G.assert_struct_equal(got, d["waveform_width"], float_rtol=1e-6, what="records route vs reference")
    ctx = SimpleContext({"waveform_width": {"wave_source": "records"},
                         "basic_features": {"wave_source": "st_waveforms", "height_range": (40, 90), "area_range": (0, None)},
                         "s1_s2": S1S2_CFG},
                        {"hit": hits, "records": rec, "wave_pool": pool, "st_waveforms": st},
                        plugins=[HipWaveformWidthPlugin(), HipBasicFeaturesPlugin(), HipS1S2ClassifierPlugin()])
    G.assert_struct_equal(ctx.get_data("run", "s1_s2"), d["s1_s2"], float_rtol=1e-6, what="s1_s2 on the records route")


def test_records_only_chain_reaches_s1_s2():
    """wave_pool_filtered -> hit -> waveform_width -> s1_s2 (basic_features on the side) from records + wave_pool alone:
    one global wave_source, no st_waveforms anywhere."""
    case = G.load_peaks("peaks_positive")
    rec, pool = case["records"], case["wave_pool"]
    ctx = SimpleContext({"wave_source": "records", **S1S2_CFG}, {"records": rec, "wave_pool": pool}, plugins=hip_default())
    got = ctx.get_data("run", "s1_s2")

    hits = O.find_peak_hits(rec, O.filter_wave_pool(rec, pool))
    widths = W.oracle_widths(hits, rec, pool)
    want = O.s1_s2_classify(widths, O.basic_features(rec, pool), **S1S2_CFG)
    assert len(hits) >= 10 and len(want) >= 10
    G.assert_struct_equal(ctx.get_data("run", "hit"), hits, what="hit")
    G.assert_struct_equal(ctx.get_data("run", "waveform_width"), widths, what="waveform_width")
    G.assert_struct_equal(got, want, what="s1_s2")
    assert "st_waveforms" not in ctx._data and not any(name == "st_waveforms" for _run, name in ctx._results)
    sess = default_pool().session()
    assert sess.holds_pool(pool)  # the run's pool is still the resident one: the next records plugin uploads nothing
    assert not sess.ensure_pool(pool)
