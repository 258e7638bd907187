"""Premises of test_hip_features_edges.py, on the CPU: the runs it feeds the feature kernels do tell numpy's summation
orders from plausible wrong ones, so a kernel that reduced in another order would fail there.

The wrong orders are small numpy models (tests/features_edges_util.py): a sequential sum, a pairwise tree whose split
is not rounded down to a multiple of 8, a leaf whose 8 accumulators combine left to right, and the blocked cumulative
sum the lane-per-leaf width kernel locates crossings with.  The model of numpy's own tree is checked against np.sum:
if a numpy release changes its tree, this file says so first."""

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import features_edges_util as E


def _np_sum_rows(X):
    return np.array([np.sum(x) for x in X])


def _differ(a, b):
    return float(np.mean(a.view(np.int64) != b.view(np.int64)))


def _split_rounds(n):
    """numpy's tree of n elements has a split where n / 2 is not already a multiple of 8."""
    if n <= 128:
        return False
    n2 = n // 2
    return n2 % 8 != 0 or _split_rounds(n2 - n2 % 8) or _split_rounds(n - (n2 - n2 % 8))


@pytest.mark.parametrize("L", (256, 8192, 20000))
def test_tree_model_is_numpys_sum(L):
    rec, pool = E.wide(40 if L == 256 else 8, L, "unknown", seed=L)
    lengths = E.SWEEP_SHORT if L == 256 else (E.SWEEP_LONG if L == 8192 else (8193, 16384, 16392, 20000))
    for n in lengths:
        X = E.signal_rows(rec, pool, 0, n)
        assert E.pairwise(X).tobytes() == _np_sum_rows(X).tobytes(), n


@pytest.mark.parametrize("polarity", E.POLARITIES)
def test_sweep_runs_separate_summation_orders(polarity):
    """Unknown polarity (float64 terms with a k/40 baseline): for every area length n >= 8 of the sweep, from every
    start, at least 10 % of the records come out differently when summed sequentially; where numpy's tree rounds a
    split, at least 10 % differ without the rounding; a left-to-right combine of the leaf's 8 accumulators changes
    some record at every length and 10 % on average.
    Known polarities: the float32 terms add exactly in float64, so those runs test the terms, not the order."""
    runs = E.sweep_runs(polarity)
    combine, split = [], []
    for L, c0, n in E.sweep_cases():
        if n < 8:
            continue
        rec, pool = runs[L]
        X = E.signal_rows(rec, pool, c0, c0 + n)
        ref = _np_sum_rows(X)
        if polarity == "unknown":
            assert _differ(E.sequential(X), ref) >= 0.10, (L, c0, n)
            combine.append(_differ(E.pairwise(X, combine="sequential"), ref))
            if _split_rounds(n):
                split.append((_differ(E.pairwise(X, split8=False), ref), n))
        elif c0 == 0 and n in (136, 8192):
            assert _differ(E.sequential(X), ref) == 0.0, (L, n)
    if polarity == "unknown":
        assert min(combine) > 0.0 and np.mean(combine) >= 0.10, (min(combine), np.mean(combine))
        assert split and min(split)[0] >= 0.10, min(split)
        assert {n for _f, n in split} >= {130, 136, 1023, 4095, 4104, 8184}


def _width_stats(rec, pool, q):
    X = E.width_terms(rec, pool)
    t = q * E.pairwise(X)
    idx = E.searchsorted_rows(np.cumsum(X, axis=1), t)
    blocked = E.searchsorted_rows(E.blocked_cumsum(X), t)
    return X, idx, blocked


def test_quantile_runs_are_order_decided():
    """q_high = nextafter(1, 0): every record has a cumulative value within the kernel's tolerance of the target (the
    leaf kernel must hand it to numpy's order), some records cross nowhere (index L), and in at least 20 % the
    blocked order of the leaf kernel alone would give another index."""
    rec, pool = E.QUANTILE_RUNS["pulsed_800_unknown"]()
    X, idx, blocked = _width_stats(rec, pool, E.NEXTAFTER_ONE)
    live = E.pairwise(X) > 0
    assert np.mean(E.near_target(X, E.NEXTAFTER_ONE)[live]) >= 0.99
    assert np.sum(idx == X.shape[1]) >= 20
    assert np.mean(idx != blocked) >= 0.20
    want = O.width_integral(rec, pool, q_low=0.1, q_high=E.NEXTAFTER_ONE)
    np.testing.assert_array_equal(want["t_high_samples"][live], idx[live].astype(np.float32))
    # the special records: q_total = 0, and single terms inside / first / last
    assert E.pairwise(X)[3] == 0.0
    for r, at in ((4, 400), (5, 0), (6, 799)):
        assert np.flatnonzero(X[r]).tolist() == [at]


def test_tiny_quantile_targets():
    """q_low = 5e-324 / 1e-300: targets are subnormal / tiny but non-zero, and leading x = 0 terms lie in front of
    the crossing, which is the first non-zero term."""
    for run, lead in (("pulsed_64_lead_zeros", 13), ("pulsed_800_lead_zeros", 37)):
        rec, pool = E.QUANTILE_RUNS[run]()
        X = E.width_terms(rec, pool)
        tot = E.pairwise(X)
        live = tot > 0
        live[3:7] = False  # the special records (with_special_records) overwrite the leading zeros
        assert np.all(X[live, :lead] == 0.0)
        t = E.TINY_Q[0] * tot[live]
        assert np.all((t > 0) & (t < np.finfo(np.float64).tiny))
        idx = E.searchsorted_rows(np.cumsum(X[live], axis=1), t)
        first = np.argmax(X[live] > 0, axis=1)
        assert np.array_equal(idx, first) and np.all(idx >= lead)


def test_tie_queue_run_outgrows_the_tie_kernel_grid():
    """More than twice k_width_ties' 256 x 64 lanes are queued, and the blocked order alone gets at least 20 % of the
    records wrong, so records the grid-stride loop reaches only on a later turn decide the result too."""
    rec, pool = E.wide(E.TIE_RECORDS, 64, "unknown", seed=26)
    X, idx, blocked = _width_stats(rec, pool, E.NEXTAFTER_ONE)
    assert int(np.sum(E.near_target(X, E.NEXTAFTER_ONE))) > 2 * 256 * 64
    assert np.mean(idx != blocked) >= 0.20


@pytest.mark.parametrize("L,polarity", [(800, "unknown"), (64, "positive"), (800, "negative")])
def test_integer_ties_hit_dyadic_targets_on_plateaus(L, polarity):
    """Every record's cumulative sum equals q * total exactly for q = 1/4, 1/2, 3/4, at a sample followed by an x = 0
    term, so searchsorted side="left" and side="right" give different indices."""
    rec, pool = E.integer_ties(300, L, polarity, seed=L)
    X = E.width_terms(rec, pool)
    assert np.all(X == np.rint(X))
    tot = E.pairwise(X)
    assert np.array_equal(tot, X.sum(axis=1)) and np.all(tot > 0)
    C = np.cumsum(X, axis=1)
    for q in (0.25, 0.5, 0.75):
        for r in range(len(rec)):
            left = int(np.searchsorted(C[r], q * tot[r], side="left"))
            assert C[r, left] == q * tot[r], (r, q)
            assert int(np.searchsorted(C[r], q * tot[r], side="right")) > left + 1, (r, q)


def test_slice_values_cover_every_resolution():
    """The slice values of the D cases give empty and start >= end ranges, both residues of the area start mod 8 on
    the uniform run, starts and ends clipped at both record edges, and on the ragged run slices that resolve
    differently from record to record."""
    L = 800
    res = {slice(*p).indices(L)[:2] for p in E.slice_pairs(L)}
    assert (0, L) in res and (L, L) in res and (0, 0) in res
    assert any(s > e for s, e in res) and any(s % 8 == 0 for s, _e in res) and any(s % 8 for s, _e in res)
    per_len = {slice(-41, 9).indices(n)[:2] for n in E.RAGGED_LENGTHS}
    assert len(per_len) >= 5
