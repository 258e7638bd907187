"""The per-record feature kernels at the edges where their numpy-order promise is hardest to keep (tests/
features_edges_util.py builds the runs; test_features_edges_cpu.py proves they separate the summation orders):

  A  area sums over every length 0 .. 136 and the pairwise tree's split points up to 8192, from aligned area starts
     (k_basic_features_leaf) and an unaligned one (k_basic_features), on data whose sums depend on the order
  B  width over record lengths on the leaf route (24 .. 8192) and the general one (1, 7, 8, 9, 23, 801)
  C  quantiles whose targets tie with cumulative values: q_high = nextafter(1, 0), subnormal / tiny q_low, dyadic q on
     exact integer sums, q_total = 0 and single-term records, and a run that queues more records for k_width_ties
     than it has lanes
  D  python slices for height_range / area_range (negative, empty, start >= end, past the record) on uniform and
     ragged runs, raw and float32 pools, extremes on the edges of the height range and of the max|diff| lanes

Every case is bit-exact against the oracle, byte-identical across the routes that can run it (lane-per-leaf,
`no_span`, features_both), and asserts which kernel ran."""

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import features_edges_util as E
from tests import golden_util as G
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DeviceSession
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipBasicFeaturesPlugin

pytestmark = pytest.mark.gpu

HR = (40, 90)


@pytest.fixture(scope="module")
def sess():
    with DeviceSession(0) as s:
        s.set_option("no_span", False)
        yield s


def _ran(sess, call):
    """(result of call(), names of the kernels it launched)"""
    sess.profile(True)
    try:
        got = call()
        names = set(sess.profile_report())
    finally:
        sess.profile(False)
    return got, names


def _upload(sess, rec, pool, f32=None):
    sess.upload_pool(pool)
    if f32 is not None:
        sess.upload_filtered_pool(f32)
    sess.upload_records(rec, 10.0)


def _bf_routes(sess, source, hr, ar, want, leaf, what):
    """basic_features on its default route (the leaf kernel iff `leaf`) and with no_span: both == want, bit for bit."""
    got, names = _ran(sess, lambda: sess.basic_features(source, hr, ar))
    assert ("k_basic_features_leaf" if leaf else "k_basic_features") in names, (what, names)
    G.assert_struct_equal(got, want, what=what)
    sess.set_option("no_span", True)
    try:
        got2, names2 = _ran(sess, lambda: sess.basic_features(source, hr, ar))
    finally:
        sess.set_option("no_span", False)
    assert "k_basic_features" in names2 and "k_basic_features_leaf" not in names2, (what, names2)
    assert got2.tobytes() == got.tobytes(), what
    return got


def _wi_routes(sess, q_low, q_high, dt, want, leaf, what, bf_want=None):
    """width_integral on its default route, with no_span and through features_both: all == want, bit for bit."""
    got, names = _ran(sess, lambda: sess.width_integral(_lib.SRC_RAW, q_low, q_high, dt))
    assert ("k_width_integral_leaf" if leaf else "k_width_integral") in names, (what, names)
    G.assert_struct_equal(got, want, what=what)
    sess.set_option("no_span", True)
    try:
        got2, names2 = _ran(sess, lambda: sess.width_integral(_lib.SRC_RAW, q_low, q_high, dt))
    finally:
        sess.set_option("no_span", False)
    assert "k_width_integral" in names2 and "k_width_integral_leaf" not in names2, (what, names2)
    assert got2.tobytes() == got.tobytes(), what
    (ob, ow), names3 = _ran(sess, lambda: sess.features_both(HR, (0, None), q_low, q_high, dt))
    assert ("k_features_both_leaf" if leaf else "k_width_integral") in names3, (what, names3)
    assert ow.tobytes() == got.tobytes(), what + " (features_both)"
    if bf_want is not None:
        G.assert_struct_equal(ob, bf_want, what=what + " (features_both basic rows)")


# -- A: area sums over lengths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("polarity", E.POLARITIES)
def test_area_sum_length_sweep(sess, polarity):
    runs = E.sweep_runs(polarity)
    for L, (rec, pool) in runs.items():
        _upload(sess, rec, pool)
        for L_, c0, n in E.sweep_cases():
            if L_ != L:
                continue
            ar = (c0, c0 + n)
            want = O.basic_features(rec, pool, height_range=HR, area_range=ar)
            _bf_routes(sess, _lib.SRC_RAW, HR, ar, want, c0 % 8 == 0, f"{polarity} L {L} area {ar}")


def test_area_sum_past_numpy_reduce_block(sess):
    """Areas longer than numpy's 8192-element reduce block: the general kernel only (no leaf plan)."""
    rec, pool = E.wide(6, 20000, "unknown", seed=13)
    _upload(sess, rec, pool)
    for ar in ((0, None), (0, 8193), (8, 16392), (3, 19999)):
        want = O.basic_features(rec, pool, height_range=HR, area_range=ar)
        _bf_routes(sess, _lib.SRC_RAW, HR, ar, want, False, f"L 20000 area {ar}")


@pytest.mark.parametrize("polarity", ("unknown", "positive"))
def test_area_sum_float32_pool(sess, polarity):
    """SRC_F32 reads the filtered pool with the general kernel: a few lengths of the sweep on non-integer samples."""
    rec, pool = E.wide(128, 256, polarity, seed=14)
    rng = np.random.default_rng(15)
    f32 = (pool.astype(np.float32) * np.float32(0.731) + rng.normal(0, 0.5, pool.size).astype(np.float32))
    _upload(sess, rec, pool, f32)
    for c0 in (0, 3, 8):
        for n in (0, 1, 7, 8, 9, 16, 100, 128, 129, 136, 200):
            if c0 + n > 256:
                continue
            ar = (c0, c0 + n)
            want = O.basic_features(rec, f32, height_range=HR, area_range=ar)
            _bf_routes(sess, _lib.SRC_F32, HR, ar, want, False, f"f32 {polarity} area {ar}")


# -- B: width over record lengths ------------------------------------------------------------------------------------
LEAF_LENGTHS = tuple(range(24, 137, 8)) + (256, 1000, 1024, 4096, 8192)
GENERAL_LENGTHS = (1, 7, 8, 9, 23, 801)


@pytest.mark.parametrize("gen", ("wide", "pulsed_tail"))
def test_width_over_record_lengths(sess, gen):
    for L in LEAF_LENGTHS + GENERAL_LENGTHS:
        n_rec = 160 if L <= 1024 else 24
        rec, pool = getattr(E, gen)(n_rec, L, "unknown", seed=L)
        _upload(sess, rec, pool)
        want = O.width_integral(rec, pool, q_low=0.1, q_high=0.9, dt=2.0)
        bf_want = O.basic_features(rec, pool)
        _wi_routes(sess, 0.1, 0.9, 2.0, want, L in LEAF_LENGTHS, f"{gen} L {L}", bf_want=bf_want)


# -- C: quantile edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", sorted(E.QUANTILE_RUNS))
def test_width_quantile_edges(sess, run):
    rec, pool = E.QUANTILE_RUNS[run]()
    _upload(sess, rec, pool)
    for q_low, q_high in E.QUANTILES:
        want = O.width_integral(rec, pool, q_low=q_low, q_high=q_high, dt=0.3)
        _wi_routes(sess, q_low, q_high, 0.3, want, True, f"{run} q {q_low!r}, {q_high!r}")


@pytest.mark.parametrize("L,polarity", [(800, "unknown"), (64, "positive"), (800, "negative")])
def test_width_dyadic_quantiles_on_exact_ties(sess, L, polarity):
    rec, pool = E.integer_ties(300, L, polarity, seed=L)
    _upload(sess, rec, pool)
    for q_low, q_high in ((0.25, 0.75), (0.5, 0.75), (0.25, 0.5), (0.25, E.NEXTAFTER_ONE)):
        want = O.width_integral(rec, pool, q_low=q_low, q_high=q_high, dt=0.3)
        _wi_routes(sess, q_low, q_high, 0.3, want, True, f"ties L {L} {polarity} q {q_low}, {q_high}")


def test_width_tie_queue_longer_than_its_grid(sess):
    """q_high = nextafter(1, 0) on 40 000 wide 64-sample records: every record is queued for k_width_ties, more than
    its 256 x 64 lanes, so the grid-stride loop takes them in several turns; in about a quarter of them only numpy's
    order gives the right index."""
    rec, pool = E.wide(E.TIE_RECORDS, 64, "unknown", seed=26)
    _upload(sess, rec, pool)
    want = O.width_integral(rec, pool, q_low=0.1, q_high=E.NEXTAFTER_ONE, dt=0.3)
    _wi_routes(sess, 0.1, E.NEXTAFTER_ONE, 0.3, want, True, "tie queue")


def test_width_ragged_run(sess):
    rec, pool = E.ragged(seed=27)
    _upload(sess, rec, pool)
    for q_low, q_high in ((0.1, 0.9),) + E.QUANTILES:
        want = O.width_integral(rec, pool, q_low=q_low, q_high=q_high, dt=0.3)
        _wi_routes(sess, q_low, q_high, 0.3, want, False, f"ragged q {q_low!r}, {q_high!r}")


# -- D: slices and extremes ------------------------------------------------------------------------------------------
def _start(sl, L):
    return slice(*sl).indices(L)[0]


def _extremes_run(L=800, n_rec=64):
    """Uniform wide records (unknown and negative polarity: one span class) with 0 / 65535 next to each other on the
    lane and chunk edges of the max|diff| walk, and extremes on the first and last sample of the height range."""
    rec, pool = E.wide(n_rec, L, "unknown", seed=31)
    rec["polarity"][1::2] = "negative"
    W = pool[:n_rec * L].reshape(n_rec, L)
    W[:, 1:] = np.clip(W[:, 1:], 100, 65400)  # the planted pairs below are the largest differences
    for r, at in enumerate((0, 7, 103, 104, 207, L - 2, 399, 8 * (L // 16))):
        W[r, at], W[r, at + 1] = (0, 65535) if r % 2 else (65535, 0)
    W[8, HR[0]], W[8, HR[1] - 1] = 0, 65535
    W[9, HR[0]], W[9, HR[1] - 1] = 65535, 0
    W[10, L - 1], W[10, 0] = 0, 65535
    return rec, pool


@pytest.mark.parametrize("polarity", ("mixed", "positive"))
def test_slices_uniform(sess, polarity):
    L = 800
    rec, pool = _extremes_run(L)
    if polarity == "positive":
        rec["polarity"] = "positive"
    _upload(sess, rec, pool)
    for ar in E.slice_pairs(L):  # every area slice, height fixed
        want = O.basic_features(rec, pool, height_range=HR, area_range=ar)
        _bf_routes(sess, _lib.SRC_RAW, HR, ar, want, _start(ar, L) % 8 == 0, f"{polarity} area {ar}")
    for hr in E.slice_pairs(L):  # every height slice, area from an aligned start
        want = O.basic_features(rec, pool, height_range=hr, area_range=(0, None))
        _bf_routes(sess, _lib.SRC_RAW, hr, (0, None), want, True, f"{polarity} height {hr}")
    for hr, ar in (((-L - 5, L + 100), (-L, -1)), ((L - 1, None), (-41, 9)), ((9, 7), (L + 1, None)),
                   ((-1, None), (-L + 1, L)), ((None, None), (None, None)), ((40, 40), (8, 8)), ((0, 1), (L - 1, L))):
        want = O.basic_features(rec, pool, height_range=hr, area_range=ar)
        _bf_routes(sess, _lib.SRC_RAW, hr, ar, want, _start(ar, L) % 8 == 0, f"{polarity} height {hr} area {ar}")


def test_features_both_whole_record_through_a_slice(sess):
    """An area range that resolves to the whole record without being (0, None) still takes the fused kernel."""
    L = 800
    rec, pool = _extremes_run(L)
    _upload(sess, rec, pool)
    for ar in ((-L - 5, L + 100), (None, None), (-L, L)):
        (ob, ow), names = _ran(sess, lambda: sess.features_both(HR, ar, 0.1, 0.9, 0.3))
        assert "k_features_both_leaf" in names, (ar, names)
        G.assert_struct_equal(ob, O.basic_features(rec, pool, height_range=HR, area_range=ar), what=f"both bf {ar}")
        G.assert_struct_equal(ow, O.width_integral(rec, pool, dt=0.3), what=f"both wi {ar}")
    (ob, _ow), names = _ran(sess, lambda: sess.features_both(HR, (8, L + 100), 0.1, 0.9, 0.3))
    assert "k_features_both_leaf" not in names and "k_basic_features_leaf" in names, names
    G.assert_struct_equal(ob, O.basic_features(rec, pool, height_range=HR, area_range=(8, L + 100)), what="both (8, L+100)")


@pytest.mark.parametrize("source", ("raw", "f32"))
def test_slices_ragged(sess, source):
    rec, pool = E.ragged(seed=32)
    f32 = None
    if source == "f32":
        f32 = (pool.astype(np.float32) * np.float32(1.37) - np.float32(1000.25))
    _upload(sess, rec, pool, f32)
    src, data = (_lib.SRC_RAW, pool) if f32 is None else (_lib.SRC_F32, f32)
    for L in (800, 24):
        for ar in E.slice_pairs(L):
            want = O.basic_features(rec, data, height_range=HR, area_range=ar)
            _bf_routes(sess, src, HR, ar, want, False, f"ragged {source} area {ar}")
        for hr in E.slice_pairs(L):
            want = O.basic_features(rec, data, height_range=hr, area_range=(5, -3))
            _bf_routes(sess, src, hr, (5, -3), want, False, f"ragged {source} height {hr}")


def test_slices_uniform_float32(sess):
    L = 800
    rec, pool = _extremes_run(L)
    f32 = (pool.astype(np.float32) * np.float32(0.25) + np.float32(0.1))
    _upload(sess, rec, pool, f32)
    for ar in E.slice_pairs(L):
        want = O.basic_features(rec, f32, height_range=HR, area_range=ar)
        _bf_routes(sess, _lib.SRC_F32, HR, ar, want, False, f"f32 area {ar}")


def test_plugin_negative_slices(sess):
    rec, pool = _extremes_run(800)
    cfg = {"height_range": (-60, -10), "area_range": (-504, -3)}
    ctx = SimpleContext({"wave_source": "records", "basic_features": cfg}, {"records": rec, "wave_pool": pool},
                        plugins=[HipBasicFeaturesPlugin()])
    G.assert_struct_equal(ctx.get_data("run", "basic_features"),
                          O.basic_features(rec, pool, height_range=(-60, -10), area_range=(-504, -3)),
                          what="plugin negative slices")
