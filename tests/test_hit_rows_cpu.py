"""The hit-row inputs of tests/hit_rows_util.py, without a GPU: the oracle equals the independent plain-Python reference
on every generated set, and every family holds a minimum number of rows that show its rule, so a change to a generator
cannot hollow out tests/test_hip_hit_rows.py."""

import numpy as np
import pytest

from tests import hit_rows_util as U
from waveformanalysis_amd.sg_plan import build_plan

ALL = [hs.name for hs in U.all_sets()]


def _row_records(hs, rows):
    return rows["record_id"].astype(np.int64)  # record_id == record index


@pytest.mark.parametrize("name", ALL)
def test_oracle_equals_plain_python_reference(name):
    """Integer fields, height, rise / fall time and width exactly; the integral exactly on the raw sets and on the sets
    with dyadic baselines, where the float64 sum in index order is the rational sum (`sum_exact`: the order of the
    additions cannot matter), within one float32 ulp elsewhere.  Rows in (record, start) order."""
    hs = U.by_name(name)
    exact_integral = hs.source == "raw" or hs.dyadic
    for le, re in hs.ext:
        want, det = hs.exact(le, re)
        got = hs.oracle(le, re)
        assert len(want) >= 100, (name, le, re, len(want))
        U.assert_rows(got, want, exact_integral=exact_integral, what=f"{name} ({le}, {re})")
        if exact_integral:
            assert det["sum_exact"].all(), (name, le, re, int((~det["sum_exact"]).sum()))
        rid = _row_records(hs, want)
        assert np.all((np.diff(rid) > 0) | ((np.diff(rid) == 0) & (np.diff(det["start"]) > 0))), (name, le, re)
        assert np.sum(want["timestamp"] >= 2**53) >= 3 and np.sum(want["timestamp"] >= 2**62 - 2 * 10**9) >= 1, name
    assert set(np.unique(hs.records["dt"])) == {1, 2, 4}
    if hs.window is not None:  # the baseline is what the fused pass computes from the pool
        lo, hi = hs.window
        waves = hs.pool.reshape(len(hs.records), -1)
        np.testing.assert_array_equal(waves[:, lo:hi].sum(axis=1, dtype=np.int64) / float(hi - lo), hs.records["baseline"])


def test_numpy_order_equals_rational_sum_proof_has_a_counterexample():
    """The check above is not vacuous: with a baseline next to 262144 that is no dyadic fraction the float64 sum in
    index order is not the rational sum."""
    hs = U.by_name("D_raw_stream_neg")
    rec = hs.records.copy()
    ped = rec["baseline"].copy()
    rec["baseline"] = 262143.99
    thr = hs.thresholds + (rec["baseline"] - ped)
    _rows, det = U.hit_rows_exact(rec, hs.pool, thr, 5, 7, hs.width, details=True)
    assert 0 < det["sum_exact"].sum() < len(det["sum_exact"])


def test_round_f32_rounds_once_ties_to_even():
    from fractions import Fraction
    assert U._round_f32(Fraction(1, 3)) == np.float32(1.0 / 3.0)
    half = Fraction(1) + Fraction(1, 2**24)  # halfway between two float32 values: ties to even
    assert U._round_f32(half) == np.float32(1.0)
    assert U._round_f32(half + Fraction(1, 2**60)) == np.nextafter(np.float32(1.0), np.float32(2.0))


# ---- A ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.names("A"))
def test_family_a_windows_clamp_and_extensions_are_asymmetric(name):
    hs = U.by_name(name)
    L = hs.records["event_length"]
    clamp_left = clamp_right = one_sample = whole = 0
    for le, re in hs.ext:
        rows, det = hs.exact(le, re)
        rid = _row_records(hs, rows)
        clamp_left = max(clamp_left, int(np.sum(det["start"] - max(le, 0) < 0)))
        clamp_right = max(clamp_right, int(np.sum(det["end"] + max(re, 0) > hs.width)))
        one_sample = max(one_sample, int(np.sum(det["end"] - det["start"] == 1)))
        whole = max(whole, int(np.sum((det["start"] == 0) & (det["end"] == L[rid]))))
    assert clamp_left >= 50 and clamp_right >= 50 and one_sample >= 50 and whole >= 50, \
        (clamp_left, clamp_right, one_sample, whole)
    # exchanging the two extensions gives other rows
    for le, re in ((0, 5), (1, 9), (hs.ext[4])):
        a = hs.oracle(le, re)
        b = U.oracle_rows(hs.records, hs.src_pool, hs.thresholds, re, le, hs.max_len)
        differ = (a["edge_start"] != b["edge_start"]) | (a["edge_end"] != b["edge_end"]) | (a["integral"] != b["integral"])
        assert differ.sum() >= 200, (name, le, re, int(differ.sum()))
    # a negative extension is 0
    np.testing.assert_array_equal(hs.oracle(-3, 2), hs.oracle(0, 2))
    if hs.layout == "ragged":
        assert hs.max_len > L.max()
        wins = other = 0
        for le, re in hs.ext:
            rows, det = hs.exact(le, re)
            rid = _row_records(hs, rows)
            positive = hs.records["polarity"][rid] == "positive"
            reaches = det["seg_end"] > L[rid]
            wins = max(wins, int(np.sum(reaches & (rows["position"] >= L[rid]))))
            other = max(other, int(np.sum(reaches & positive & (rows["position"] < L[rid]))))
        assert wins >= 50 and other >= 50, (wins, other)


# ---- B ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.names("B"))
def test_family_b_position_leaves_the_run(name):
    hs = U.by_name(name)
    left = right = 0
    for le, re in hs.ext:
        rows, det = hs.exact(le, re)
        left = max(left, int(np.sum((rows["rise_time"] == 0) & (rows["position"] < det["start"]))))
        right = max(right, int(np.sum((rows["fall_time"] == 0) & (rows["position"] > det["end"] - 1))))
    assert left >= 50 and right >= 50, (name, left, right)


# ---- C ----------------------------------------------------------------------------------------------------------
def _tie_placements(hs):
    """How often a window's tied maxima fall on the two sides of each boundary (chunks, 64-sample steps, padding and
    runs: the first and the last of them; edge zones: any two)."""
    out = dict.fromkeys(("rows", "chunks", "step64", "left_edge", "right_edge", "real_pad", "pad_pad", "neighbour"), 0)
    for le, re in hs.ext:
        rows, det = hs.exact(le, re)
        last, _ = hs.exact(le, re, True)
        tied = det["ties"] > 1
        assert np.array_equal(tied, last["position"] != rows["position"]), (hs.name, le, re)
        assert np.array_equal(last["height"], rows["height"])
        rid = _row_records(hs, rows)
        L, off = hs.records["event_length"][rid], hs.records["wave_offset"][rid]
        p1, p2 = rows["position"], last["position"]
        own1 = (p1 >= det["start"]) & (p1 < det["end"])
        own2 = (p2 >= det["start"]) & (p2 < det["end"])
        counts = {
            "rows": tied,
            "chunks": tied & (p2 < L) & ((off + p1) >> 3 != (off + p2) >> 3),
            "step64": tied & ((p1 - det["seg_start"]) // 64 != (p2 - det["seg_start"]) // 64),
            "left_edge": tied & (det["tie_zones"] & 3 == 3),
            "right_edge": tied & (det["tie_zones"] & 6 == 6),
            "real_pad": tied & (p1 < L) & (p2 >= L),
            "pad_pad": tied & (p1 >= L),
            "neighbour": tied & (own1 != own2),
        }
        for k, m in counts.items():
            out[k] = max(out[k], int(m.sum()))
    return out


@pytest.mark.parametrize("name", U.names("C"))
def test_family_c_windows_hold_their_maximum_more_than_once(name):
    hs = U.by_name(name)
    got = _tie_placements(hs)
    assert got["rows"] >= 200, got
    for k in ("chunks", "step64", "left_edge", "right_edge", "neighbour"):
        assert got[k] >= 10, (name, k, got)
    if hs.layout == "ragged":
        assert got["real_pad"] >= 10 and got["pad_pad"] >= 10, (name, got)


# ---- D ----------------------------------------------------------------------------------------------------------
def _guard_in_y(hs):
    plan = build_plan(*hs.plan)
    return plan.guard / plan.den


@pytest.mark.parametrize("name", U.names("D"))
def test_family_d_signs_baselines_and_guard(name):
    hs = U.by_name(name)
    rec = hs.records
    b = rec["baseline"]
    positive = rec["polarity"] == "positive"
    y = hs.src_pool
    neg = zero = pos = under = over = tiny = 0
    for le, re in hs.ext:
        rows, det = hs.exact(le, re)
        rid = _row_records(hs, rows)
        n = z = p = u = t = 0
        for k, r in enumerate(rid):
            L, off = int(rec["event_length"][r]), int(rec["wave_offset"][r])
            idx = [i for i in range(det["seg_start"][k], min(det["seg_end"][k], L))
                   if not det["start"][k] <= i < det["end"][k]]
            w = y[off + np.asarray(idx, dtype=np.int64)].astype(np.float64)
            sig = (w - b[r]) if positive[r] else (b[r] - w)
            n, z, p = n + int(np.sum(sig < 0)), z + int(np.sum(sig == 0)), p + int(np.sum(sig > 0))
            t += bool(np.any((sig > 0) & (sig <= np.spacing(np.abs(w).astype(np.float32)))))
            if hs.source == "sg":
                win = y[off + det["seg_start"][k]:off + min(det["seg_end"][k], L)]
                u += bool(len(win)) and float(win.min()) < _guard_in_y(hs)
        neg, zero, pos, under, over = max(neg, n), max(zero, z), max(pos, p), max(under, u), max(over, len(rows) - u)
        tiny = max(tiny, t)
    assert neg >= 50 and pos >= 50, (name, neg, zero, pos)
    if hs.window is not None:
        assert np.all(b * 64 == np.rint(b * 64))  # the fused baseline: a mean of 32 or 64 samples, or an integer
    elif hs.dyadic:
        assert zero >= 50, (name, zero)
        assert np.sum(np.abs(b) >= 262144.0) >= 50 and np.sum((np.abs(b) > 262143.0) & (np.abs(b) < 262144.0)) >= 50
        assert np.sum(b == 0.0) >= 50 and np.sum(b < 0.0) >= 50
        assert np.all(b * 2**23 == np.rint(b * 2**23))
        if hs.source == "sg":  # an extension sample one float32 step on the positive side of the baseline
            assert tiny >= 20, (name, tiny)
    else:
        sb = np.where(positive, -b, b)
        f = sb.astype(np.float32).astype(np.float64)
        assert np.sum(f > sb) >= 50 and np.sum(f < sb) >= 50, (name, int(np.sum(f > sb)), int(np.sum(f < sb)))
        assert np.sum((np.abs(b) > 0) & (np.abs(b) < 1e-20)) >= 50
    if hs.source == "sg":  # hits under the integer guard (literal kernel) next to ordinary ones
        assert under >= 50 and over >= 50, (name, under, over)


# ---- E ----------------------------------------------------------------------------------------------------------
def test_family_e_hit_counts_straddle_a_wave():
    for n in (2 * U.FLAT_HITS - 1, 2 * U.FLAT_HITS, 2 * U.FLAT_HITS + 1):
        hs = U.by_name(f"E_sg5_count{n}")
        for le, re in hs.ext:
            assert len(hs.exact(le, re)[0]) == n
        # (64, 64): every window is the whole record, 2H edge samples per hit, more than 64 per wave
        _chunks, edges = U.flat_chunks(hs, U.E_L, U.E_L)
        assert np.all(edges == 2 * hs.H) and edges[:U.FLAT_HITS].sum() > 64


def test_family_e_chunk_batches():
    hs = U.by_name("E_sg5_cap")
    (le, re), = hs.ext
    assert (le, re) == (U.CAP_LE, U.CAP_RE)
    rows, _det = hs.exact(le, re)
    assert np.array_equal(rows["record_id"], np.arange(4 * U.FLAT_HITS))  # one hit per record: wave w = records 64w ..
    chunks, _edges = U.flat_chunks(hs, le, re)
    totals = chunks.reshape(4, U.FLAT_HITS).sum(axis=1)
    assert totals.tolist() == [U.FLAT_CAP - 1, U.FLAT_CAP, U.FLAT_CAP + 1, 40 * U.FLAT_HITS], totals
    for wave in (2, 3):  # a hit straddles the batch boundary
        first = np.concatenate([[0], np.cumsum(chunks[wave * 64:(wave + 1) * 64])])
        assert np.any((first[:-1] < U.FLAT_CAP) & (first[1:] > U.FLAT_CAP))


def test_family_e_short_records_have_hits_without_interior():
    hs = U.by_name("E_sg11_short")
    chunks, _edges = U.flat_chunks(hs, 0, 0)
    assert np.sum(chunks == 0) >= 50 and np.sum(chunks > 0) >= 50, (int(np.sum(chunks == 0)), int(np.sum(chunks > 0)))
    # the two kinds share waves
    assert all(0 < np.sum(chunks[w:w + 64] == 0) < 64 for w in range(0, 256, 64))
    _chunks, edges = U.flat_chunks(hs, U.E_L, U.E_L)
    assert np.all(edges == 2 * hs.H)


@pytest.mark.parametrize("name", ["E_sg5_ragged", "E_sg11_ragged"])
def test_family_e_ragged_lengths_and_offsets(name):
    hs = U.by_name(name)
    W = hs.plan[0]
    rec = hs.records
    assert {W - 1, W, W + 1, 2 * W} <= set(rec["event_length"].tolist())
    assert set((rec["wave_offset"] % 8).tolist()) == set(range(8))
    rows, det = hs.exact(0, 0)
    rid = _row_records(hs, rows)
    # flagged (shorter than the window) and unflagged descriptors share every wave
    short = rec["event_length"][rid] < W
    assert all(0 < short[w:w + 64].sum() < 64 for w in range(0, len(rows) - 63, 64))
    assert rid[0] == 0 and det["start"][0] == 0 and rec["wave_offset"][0] == 0
    last = len(rec) - 1
    assert rid[-1] == last and det["end"][-1] == rec["event_length"][last]
    assert rec["wave_offset"][last] + rec["event_length"][last] == len(hs.pool)


def test_family_e_literal_list_overflows():
    hs = U.by_name("E_sg5_litcap")
    (le, re), = hs.ext
    rows, det = hs.exact(le, re)
    assert len(rows) > U.LIT_CAP + 2 * U.FLAT_HITS
    assert len(hs.pool) < 4_300_000
    # every hit's window holds a filtered sample under the integer guard
    y = hs.filtered.reshape(-1, U.E_L)
    rid = _row_records(hs, rows)
    lo = np.array([y[r, s:e].min() for r, s, e in zip(rid, det["seg_start"], det["seg_end"])])
    assert np.sum(lo < _guard_in_y(hs)) > U.LIT_CAP + 2 * U.FLAT_HITS
