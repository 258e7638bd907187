"""Every threshold-hit route against the oracle on records whose hit mask is decided exactly at the boundary
(tests/boundary_util.py): each target sample sits on  +-(b - y) >= thr  or one float64 step to either side of it, so a
bound that is one step off in any route gives a missing or extra hit here.

Each cell runs in a fresh session and asserts the kernels of its route ran, so a silent fallback cannot pass."""

import functools

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import boundary_util as B
from tests import golden_util as G
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DeviceSession
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipThresholdHitPlugin, HipWavePoolFilteredPlugin

pytestmark = pytest.mark.gpu

SETS = {
    # name: make_set arguments (uniform L % 32 == 0: the streaming kernel's span layout)
    "L64_base_10.3": dict(n=2048, L=64, threshold=10.3, seed=1),
    "L64_base_0.1": dict(n=2048, L=64, threshold=0.1, seed=2),
    "L64_pos_base_10.3": dict(n=2048, L=64, threshold=10.3, positive=True, seed=3),
    "L800_thr_sg7_3": dict(n=1024, L=800, mode="threshold", plan=(7, 3), seed=4),
    "L800_pos_thr": dict(n=1024, L=800, mode="threshold", positive=True, seed=5),
    # L % 16 != 0: padded shadow layout (L = 90 -> stride 96)
    "L90_base_10.3": dict(n=2048, L=90, threshold=10.3, seed=6),
    "L90_pos_thr_sg9_4": dict(n=2048, L=90, mode="threshold", plan=(9, 4), positive=True, seed=7),
    # fused baseline window (0, 40): the boundary is in the threshold
    "L128_fused": dict(n=2048, L=128, mode="threshold", fused_baseline=True, seed=8),
    "L96_pos_fused": dict(n=2048, L=96, mode="threshold", fused_baseline=True, positive=True, seed=9),
    # raw and materialised float32 sources (general route)
    "raw_base_10.3": dict(n=2048, L=90, source="raw", threshold=10.3, seed=10),
    "raw_base_10": dict(n=2048, L=64, source="raw", threshold=10.0, seed=11),
    "raw_pos_thr": dict(n=2048, L=100, source="raw", mode="threshold", positive=True, seed=12),
    "f32_thr": dict(n=2048, L=96, source="f32", mode="threshold", seed=13),
    "f32_pos_base_0.1": dict(n=2048, L=64, source="f32", threshold=0.1, positive=True, seed=14),
}
STREAM = ["L64_base_10.3", "L64_base_0.1", "L64_pos_base_10.3", "L800_thr_sg7_3", "L800_pos_thr"]
PADDED = ["L90_base_10.3", "L90_pos_thr_sg9_4"]
FUSED = ["L128_fused", "L96_pos_fused"]
SG_ALL = STREAM + PADDED


@functools.cache
def bset(name):
    if name.startswith("ragged"):
        lengths = np.random.default_rng(15).integers(40, 400, 1500)
        return B.make_set(0, 0, lengths=lengths, mode="threshold", seed=16,
                          source="raw" if name.endswith("raw") else "sg")
    return B.make_set(**SETS[name])


@functools.cache
def want(name):
    return bset(name).oracle()


def _session(bs, *, blank_baseline=False, **options):
    s = DeviceSession(0)
    for k, v in options.items():
        s.set_option(k, v)
    s.upload_pool(bs.pool)
    if bs.source == "f32":
        s.upload_filtered_pool(bs.filtered)
    rec = bs.records.copy()
    if blank_baseline:
        rec["baseline"] = np.nan
    s.upload_records(rec, bs.thresholds)
    s.set_sg_plan(*bs.plan)
    s.profile(True)
    return s


def _check(got, name, what):
    ref = want(name)
    assert len(ref) > 200, (name, len(ref))
    G.assert_struct_equal(got, ref, float_rtol=1e-6, what=f"{name} {what}")


def _ran(sess, *prefixes, absent=()):
    names = sorted(sess.profile_report())
    for p in prefixes:
        assert any(k.startswith(p) for k in names), (p, names)
    for p in absent:
        assert not any(k.startswith(p) for k in names), (p, names)


@pytest.mark.parametrize("span_records", [0, 51])
@pytest.mark.parametrize("name", STREAM + PADDED)
def test_streaming(name, span_records):
    bs = bset(name)
    opts = {"span_records": span_records} if span_records else {}
    with _session(bs, **opts) as s:
        _check(s.threshold_hits(_lib.SRC_SG_FUSED, 2, 2), name, f"streaming span_records={span_records}")
        _ran(s, "k_sg_runs32", "k_runs_to_desc", absent=("k_sg_mask", "k_hits<"))


@pytest.mark.parametrize("name", FUSED)
def test_streaming_fused_baseline(name):
    bs = bset(name)
    with _session(bs, blank_baseline=True) as s:
        _check(s.fused_baseline_filter_hits((0, B.BASELINE_WINDOW), 2, 2), name, "fused baseline")
        _ran(s, "k_sg_runs32<baseline>", absent=("k_sg_mask", "k_hits<"))


@pytest.mark.parametrize("no_speculate", [False, True])
@pytest.mark.parametrize("name", ["L64_base_10.3", "L800_pos_thr", "L90_base_10.3"])
def test_streaming_queued(name, no_speculate):
    """hits_enqueue / hits_wait after a waited pass (the queued pass runs on the speculative row bound)."""
    bs = bset(name)
    with _session(bs, no_speculate=no_speculate) as s:
        _check(s.threshold_hits(_lib.SRC_SG_FUSED, 2, 2), name, "waited")
        s.profile(True)
        s.hits_enqueue(_lib.SRC_SG_FUSED, (0, 0), 2, 2)
        n = s.hits_wait()
        _check(s._fill_hits(n), name, f"queued no_speculate={no_speculate}")
        _ran(s, "k_sg_runs32", "k_hit_rows_flat", absent=("k_sg_mask", "k_hits<"))
    with _session(bset(FUSED[0]), blank_baseline=True, no_speculate=no_speculate) as s:
        s.fused_baseline_filter_hits((0, B.BASELINE_WINDOW), 2, 2)
        s.profile(True)
        s.hits_enqueue(_lib.SRC_SG_FUSED, (0, B.BASELINE_WINDOW), 2, 2)
        _check(s._fill_hits(s.hits_wait()), FUSED[0], f"queued fused baseline no_speculate={no_speculate}")
        _ran(s, "k_sg_runs32<baseline>", "k_hit_rows_flat", absent=("k_sg_mask", "k_hits<"))


@pytest.mark.parametrize("name", SG_ALL + FUSED)
def test_bitmap_route(name):
    bs = bset(name)
    fused = name in FUSED
    with _session(bs, blank_baseline=fused, no_runs32=True) as s:
        got = s.fused_baseline_filter_hits((0, B.BASELINE_WINDOW), 2, 2) if fused else s.threshold_hits(_lib.SRC_SG_FUSED, 2, 2)
        _check(got, name, "bitmap")
        _ran(s, "k_sg_mask", "k_hit_runs", absent=("k_sg_runs32", "k_hits<"))


@pytest.mark.parametrize("name", SG_ALL + FUSED)
def test_general_fused_route(name):
    bs = bset(name)
    fused = name in FUSED
    with _session(bs, blank_baseline=fused, no_fast=True) as s:
        got = s.fused_baseline_filter_hits((0, B.BASELINE_WINDOW), 2, 2) if fused else s.threshold_hits(_lib.SRC_SG_FUSED, 2, 2)
        _check(got, name, "general")
        _ran(s, "k_hits<sg_fused,baseline>" if fused else "k_hits<sg_fused>", absent=("k_sg_runs32", "k_sg_mask"))


@pytest.mark.parametrize("name", ["raw_base_10.3", "raw_base_10", "raw_pos_thr", "f32_thr", "f32_pos_base_0.1"])
def test_general_raw_and_f32(name):
    bs = bset(name)
    src = _lib.SRC_RAW if bs.source == "raw" else _lib.SRC_F32
    with _session(bs) as s:
        _check(s.threshold_hits(src, 2, 2), name, bs.source)
        _ran(s, "k_hits<raw>" if bs.source == "raw" else "k_hits<f32>", absent=("k_sg_runs32", "k_sg_mask", "k_hits<sg"))


@pytest.mark.parametrize("name", ["ragged_sg", "ragged_raw"])
def test_ragged(name):
    """Mixed lengths (no span, no padded layout): short records' right extensions reach into the zero padding up to
    the batch's longest record (kat_padded_width)."""
    bs = bset(name)
    want_rows = want(name)
    assert np.any(want_rows["edge_end"] == bs.records["event_length"][want_rows["record_id"]])
    with _session(bs) as s:
        if bs.source == "raw":
            _check(s.threshold_hits(_lib.SRC_RAW, 2, 2), name, "ragged raw")
            _ran(s, "k_hits<raw>")
        else:
            _check(s.threshold_hits(_lib.SRC_SG_FUSED, 2, 2), name, "ragged sg")
            _ran(s, "k_sg_mask", "k_hit_runs", absent=("k_sg_runs32", "k_hits<"))


def test_plugin_channel_config_on_records_and_dense_input():
    """Per-channel thresholds resolved by HipThresholdHitPlugin land on the same boundary: records input (fused filter
    and raw) and the dense st_waveforms input."""
    from waveformanalysis_amd.dtypes import create_record_dtype

    bs = B.make_set(1000, 64, source="raw", mode="threshold", seed=17)
    keep = bs.pool.reshape(-1, 64).max(axis=1) < 32768  # the dense rows are int16
    cfg = {"threshold": 10.0, "channel_config": bs.channel_config()}
    rec = bs.records
    got = SimpleContext({"wave_source": "records", "hit_threshold": dict(cfg)},
                        {"records": rec, "wave_pool": bs.pool}, plugins=[HipThresholdHitPlugin()]).get_data("run", "hit_threshold")
    G.assert_struct_equal(got, bs.oracle(), float_rtol=1e-6, what="plugin records raw")

    sg = B.make_set(1000, 64, source="sg", mode="threshold", seed=18)
    got = SimpleContext({"wave_source": "records", "hit_threshold": {"threshold": 10.0, "channel_config": sg.channel_config(),
                                                                     "use_filtered": True, "fuse_filter": True}},
                        {"records": sg.records, "wave_pool": sg.pool},
                        plugins=[HipWavePoolFilteredPlugin(), HipThresholdHitPlugin()]).get_data("run", "hit_threshold")
    G.assert_struct_equal(got, sg.oracle(), float_rtol=1e-6, what="plugin records fused sg")

    idx = np.flatnonzero(keep)
    st = np.zeros(len(idx), dtype=create_record_dtype(64))
    for f in ("baseline", "polarity", "timestamp", "record_id", "dt", "event_length", "board", "channel"):
        st[f] = rec[f][idx]
    st["wave"] = bs.pool.reshape(-1, 64)[idx].astype(np.int16)
    dense_rec = np.zeros(len(idx), dtype=[("record_id", "i8"), ("event_length", "i4"), ("wave_offset", "i8")])
    dense_rec["record_id"], dense_rec["event_length"] = st["record_id"], 64
    got = SimpleContext({"hit_threshold": dict(cfg)}, {"st_waveforms": st, "records": dense_rec},
                        plugins=[HipThresholdHitPlugin()]).get_data("run", "hit_threshold")
    want_dense = O.threshold_hits_dense(st, np.full(len(idx), 64), thresholds=bs.thresholds[idx])
    assert len(want_dense) > 200
    G.assert_struct_equal(got, want_dense, float_rtol=1e-6, what="plugin dense")


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("fused_baseline", [False, True])
def test_streaming_minus_inf_threshold_hits_every_sample(positive, fused_baseline):
    """thr = -inf: sig >= -inf holds for every sample, one run per record.  k_sg_runs32 used to step its float32 bound
    past +inf into a NaN and mask nothing inside the record, while its edge rows (int_band) masked everything: two
    runs per record instead of one."""
    bs = B.make_set(256, 128, mode="threshold", positive=positive, seed=19, specials=False, fused_baseline=fused_baseline)
    thr = bs.thresholds.copy()
    thr[::3] = -np.inf
    rec = bs.records
    ref = bs.oracle(thresholds=thr)
    assert np.sum(ref["record_id"] % 3 == 0) == len(rec[::3])  # one row per -inf record
    with _session(bs, blank_baseline=fused_baseline) as s:
        s.upload_records(_blank(rec) if fused_baseline else rec, thr)
        s.profile(True)
        got = s.fused_baseline_filter_hits((0, B.BASELINE_WINDOW), 2, 2) if fused_baseline else \
            s.threshold_hits(_lib.SRC_SG_FUSED, 2, 2)
        G.assert_struct_equal(got, ref, float_rtol=1e-6, what="thr = -inf")
        _ran(s, "k_sg_runs32", absent=("k_sg_mask", "k_hits<"))


def _blank(rec):
    out = rec.copy()
    out["baseline"] = np.nan
    return out


# ---- a record-edge sample whose exact Savitzky-Golay value is 0 (tests/golden/sgedge_zero.npz) ----------------------
# Record 5 ends in 0 56 0 56 0 0 0: the degree-3 least-squares fit of those 7 samples is exactly 0 at the last one.
# scipy (the reference) evaluates that fit with LAPACK and returns rounding noise there: 1.48e-13 in the fixture, other
# values with other BLAS kernels for the same input.  The device's float64 edge row returns the exact 0.  Record 5's
# threshold sits on the reference's noise value, so the reference has one hit (at the record's last sample) that the
# exact value does not give.  The GPU agrees with itself -- materialised filter and every fused route -- and differs
# from the fixture only there; the two strict xfails keep that difference on record.
EDGE = 5 * 128 + 127
EDGE_CAUSE = ("exact SG edge value 0: the reference's least-squares edge fit returns BLAS-dependent rounding noise "
              "(~1e-13) there, the device returns the exact 0")


@functools.cache
def _edge_case():
    return G.load_case("sgedge_zero")


def _edge_session(**options):
    c = _edge_case()
    s = DeviceSession(0)
    for k, v in options.items():
        s.set_option(k, v)
    s.upload_pool(c["wave_pool"])
    s.upload_records(c["records"], G.hit_params(c)["thresholds"])
    s.set_sg_plan(7, 3)
    s.profile(True)
    return s


def test_sg_edge_zero_materialised_is_exact():
    c = _edge_case()
    with _edge_session() as s:
        got = s.savgol()
    assert got[EDGE] == 0.0
    rest = np.arange(len(got)) != EDGE
    np.testing.assert_array_equal(got[rest], c["wave_pool_filtered"][rest])


@pytest.mark.xfail(strict=True, reason=EDGE_CAUSE)
def test_sg_edge_zero_materialised_matches_reference():
    with _edge_session() as s:
        got = s.savgol()
    assert got[EDGE] == _edge_case()["wave_pool_filtered"][EDGE]


EDGE_ROUTES = {
    "streaming": ({}, ("k_sg_runs32",)),
    "bitmap": ({"no_runs32": True}, ("k_sg_mask", "k_hit_runs")),
    "general": ({"no_fast": True}, ("k_hits<sg_fused>",)),
}


@pytest.mark.parametrize("route", EDGE_ROUTES)
def test_sg_edge_zero_fused_routes_decide_like_the_filter(route):
    """Every fused route's edge rows decide the sample with the value the materialised filter gives (the exact 0)."""
    c = _edge_case()
    opts, kernels = EDGE_ROUTES[route]
    with _edge_session() as s:
        filt = s.savgol()
    hp = G.hit_params(c)
    want_rows = O.threshold_hits(c["records"], filt, **hp)
    assert len(want_rows) == len(c["hits_filt"]) - 1  # the reference's extra hit on its noise value
    with _edge_session(**opts) as s:
        got = s.threshold_hits(_lib.SRC_SG_FUSED, hp["left_extension"], hp["right_extension"])
        _ran(s, *kernels)
    G.assert_struct_equal(got, want_rows, float_rtol=1e-6, what=f"sgedge_zero {route}")


@pytest.mark.xfail(strict=True, reason=EDGE_CAUSE)
@pytest.mark.parametrize("route", EDGE_ROUTES)
def test_sg_edge_zero_fused_routes_match_reference(route):
    c = _edge_case()
    hp = G.hit_params(c)
    with _edge_session(**EDGE_ROUTES[route][0]) as s:
        got = s.threshold_hits(_lib.SRC_SG_FUSED, hp["left_extension"], hp["right_extension"])
    G.assert_struct_equal(got, c["hits_filt"], float_rtol=1e-6, what=f"sgedge_zero {route}")
