"""The boundary-case generator (tests/boundary_util.py) on the CPU: every "on" / "off" / "beyond" triple flips the
oracle's mask at its target sample, the sets reach the regimes and shapes the GPU route matrix relies on, and the
oracle reproduces the reference's own plugins on generator output (tests/golden/boundary_*.npz) bit for bit.  (The
oracle filters with the same scipy call as the reference, so the filter comparison only guards the oracle's plumbing;
the independent check is the hit tables.)"""

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import boundary_util as B
from tests import golden_util as G

CASES = {
    "sg_baseline": dict(n=600, L=64, threshold=10.3, seed=1),
    "sg_baseline_0.1_pos": dict(n=600, L=64, threshold=0.1, positive=True, seed=2),
    "sg_threshold_sg7_3": dict(n=300, L=128, mode="threshold", plan=(7, 3), seed=3),
    "sg_fused_pos": dict(n=300, L=96, mode="threshold", fused_baseline=True, positive=True, seed=4),
    "raw_baseline_10": dict(n=600, L=90, source="raw", threshold=10.0, seed=5),
    "raw_threshold": dict(n=600, L=100, source="raw", mode="threshold", seed=6),
    "f32_threshold_pos": dict(n=300, L=64, source="f32", mode="threshold", positive=True, seed=7),
}


@pytest.mark.parametrize("name", CASES)
def test_each_target_flips_the_oracle_mask(name):
    bs = B.make_set(**CASES[name])
    rows = B.check_flips(bs)
    # the flips change the tables: off drops rows or splits runs, beyond equals on at the targets
    assert len(rows[B.ON]) > 100 and len(rows[B.ON]) != len(rows[B.OFF])
    assert set(np.unique(bs.variant)) == {B.SPECIAL, B.ON, B.OFF, B.BEYOND}


def test_sets_reach_every_regime():
    total = {}
    for kw in CASES.values():
        for k, v in B.regime_counts(B.make_set(**kw)).items():
            total[k] = total.get(k, 0) + v
    assert all(v >= 10 for v in total.values()), total


def test_shape_edges_are_present():
    bs = B.make_set(**CASES["sg_baseline"])
    on = bs.oracle(*bs.with_variant(B.ON), left_extension=0, right_extension=0)
    L = 64
    start = on["position"] - np.rint(on["rise_time"]).astype(np.int64) // on["dt"]
    end = on["position"] + np.rint(on["fall_time"]).astype(np.int64) // on["dt"] + 1
    assert np.any((start <= 31) & (end > 32)), "no run across the 31/32 tile edge"
    assert np.any(start == 0) and np.any(end == L), "no run on a record edge"
    assert np.any((on["record_id"] % 64 == 63) & (end == L)) and np.any((on["record_id"] % 51 == 50) & (end == L))
    raw = B.make_set(**CASES["raw_baseline_10"])
    raw_on = raw.oracle(*raw.with_variant(B.ON), left_extension=0, right_extension=0)
    assert np.bincount(raw_on["record_id"]).max() >= 6  # the alternating records: six one-sample runs
    full = on[(start == 0) & (end == L)]
    assert len(full) > 10  # records that hit on every sample
    # with extensions: clipped at both record ends
    ext = bs.oracle()
    assert np.any(ext["edge_start"] == 0) and np.any(ext["edge_end"] == L)
    # special records: thresholds / baselines without a boundary
    specials = B.make_set(**CASES["raw_threshold"])
    thr = specials.thresholds[specials.variant == B.SPECIAL]
    assert np.isnan(thr).any() and np.isposinf(thr).any() and np.isneginf(thr).any() and (thr < 0).any()
    nan_bl = bs.records["baseline"][bs.variant == B.SPECIAL]
    assert np.isnan(nan_bl).all()


def test_ragged_padding_quirk_is_reached():
    lengths = np.random.default_rng(15).integers(40, 400, 300)
    bs = B.make_set(0, 0, lengths=lengths, mode="threshold", seed=16, source="raw")
    B.check_flips(bs)
    rows = bs.oracle()
    L = bs.records["event_length"][rows["record_id"]]
    assert np.any(rows["edge_end"] == L)  # clamped to the record, though the segment ran into the padding


def test_tile_63_needs_long_records():
    bs = B.make_set(**CASES["sg_threshold_sg7_3"])
    on = bs.oracle(*bs.with_variant(B.ON), left_extension=0, right_extension=0)
    start = on["position"] - np.rint(on["rise_time"]).astype(np.int64) // on["dt"]
    end = on["position"] + np.rint(on["fall_time"]).astype(np.int64) // on["dt"] + 1
    assert np.any((start <= 63) & (end > 64)), "no run across the 63/64 tile edge"


def test_a_boundary_that_is_not_one_is_reported():
    bs = B.make_set(**CASES["raw_threshold"])
    rec, thr = bs.with_variant(B.OFF)
    bs.alt[B.OFF] = (rec["baseline"], np.nextafter(thr, -np.inf))  # now it is the "on" threshold again
    with pytest.raises(AssertionError, match="not on the boundary"):
        B.check_flips(bs)


BOUNDARY_FIXTURES = [n for n in G.case_names() if n.startswith("boundary_")]


def test_boundary_fixtures_present():
    assert len(BOUNDARY_FIXTURES) >= 2


@pytest.mark.parametrize("name", BOUNDARY_FIXTURES)
def test_oracle_reproduces_reference_on_the_boundary(name):
    """Filter and hits byte for byte against the reference's WavePoolFilteredPlugin / ThresholdHitPlugin."""
    case = G.load_case(name)
    fp = G.filter_params(case)
    filt = O.filter_wave_pool(case["records"], case["wave_pool"], sg_window_size=fp["sg_window_size"],
                              sg_poly_order=fp["sg_poly_order"])
    assert filt.tobytes() == case["wave_pool_filtered"].tobytes()
    hp = G.hit_params(case)
    for key, src in (("hits_raw", case["wave_pool"]), ("hits_filt", filt)):
        got = O.threshold_hits(case["records"], src, **hp)
        assert len(got) > 50
        assert got.dtype == case[key].dtype and got.tobytes() == case[key].tobytes(), f"{name} {key}"


def test_sg_edge_zero_fixture():
    """tests/golden/sgedge_zero.npz: the reference's value at a record-edge sample whose exact filter value is 0 is
    rounding noise of its least-squares fit, and the threshold of that record sits on it.  Checked without calling
    scipy here (its noise there depends on the BLAS kernel of the machine)."""
    from fractions import Fraction

    from waveformanalysis_amd.sg_plan import hat_matrix

    case = G.load_case("sgedge_zero")
    edge = 5 * 128 + 127
    last7 = case["wave_pool"][edge - 6:edge + 1].tolist()
    assert last7 == [0, 56, 0, 56, 0, 0, 0]
    assert sum(h * Fraction(x) for h, x in zip(hat_matrix(7, 3)[6], last7)) == 0
    ref = float(case["wave_pool_filtered"][edge])
    assert ref != 0.0 and abs(ref) < 1e-12
    hp = G.hit_params(case)
    assert hp["thresholds"][5] == ref
    got = O.threshold_hits(case["records"], case["wave_pool_filtered"], **hp)
    assert got.tobytes() == case["hits_filt"].tobytes()
    exact = case["wave_pool_filtered"].copy()
    exact[edge] = 0.0
    assert len(O.threshold_hits(case["records"], exact, **hp)) == len(got) - 1
