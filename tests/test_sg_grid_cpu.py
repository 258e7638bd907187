"""The Savitzky-Golay plan grid on the CPU: the oracle (scipy) and the plan tables against the exact reference of
tests/sg_reference.py, over every odd window 1..63 and orders up to W - 1."""

import functools
from fractions import Fraction

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import sg_reference as R
from waveformanalysis_amd.sg_plan import MAX_WINDOW, build_plan, hat_matrix, normalize_window

GRID = R.plan_grid()


@functools.cache
def _pools(W, P):
    out = [R.ragged_pool(W, P)]
    if W <= 48:
        out.append(R.uniform_pool(W, P))
    return out


@functools.cache
def _checked(W, P):
    """[(pool, expectation, scipy's output)] for the plan."""
    res = []
    for p in _pools(W, P):
        ref = O.filter_wave_pool(p.records(), p.pool, "SG", sg_window_size=W, sg_poly_order=P)
        res.append((p, R.expect(p, W, P), ref))
    return res


def test_grid_covers_the_issue_plan_set():
    Ws = {W for W, _ in GRID}
    assert Ws == set(range(1, MAX_WINDOW + 1, 2))
    for W in range(1, 24, 2):
        assert {P for w, P in GRID if w == W} == set(R.orders_for(W))
    assert max(P for _, P in GRID) >= 20
    assert len(GRID) > 150


@pytest.mark.parametrize("w,P", [(1, 0), (3, 1), (5, 2), (7, 3), (9, 8), (11, 2), (13, 11), (15, 6), (21, 18)])
def test_reference_rows_equal_the_plan_hat_matrix(w, P):
    H = hat_matrix(w, P)
    for i in range(w):
        assert R.hat_row_fraction(w, P, i) == H[i], (w, P, i)


@pytest.mark.parametrize("w,P", [(5, 2), (9, 4), (17, 16), (31, 7)])
def test_reference_rows_are_a_projection(w, P):
    """Each row reproduces polynomials of degree <= P exactly at its own position, and rows sum to 1."""
    for i in range(w):
        row = R.hat_row_fraction(w, P, i)
        assert sum(row) == 1
        for k in range(P + 1):
            assert sum(c * Fraction(j) ** k for j, c in enumerate(row)) == Fraction(i) ** k


def test_window_rule():
    for L in range(0, 70):
        for W, P in [(1, 0), (5, 2), (11, 4), (12, 2), (63, 8), (63, 61)]:
            Wn, Pn = normalize_window(W, P)
            w = R.effective_window(L, Wn, Pn)
            want = O.sg_window_length(L, Wn, Pn)
            assert w == (0 if want is None else want), (L, W, P)
    for W, P in R.EVEN_INPUTS:
        assert normalize_window(W, P) == (W + 1, P)
        assert build_plan(W, P).window == W + 1
    with pytest.raises(ValueError, match="exceeds the supported maximum 63"):
        build_plan(64, 2)
    with pytest.raises(ValueError):
        normalize_window(4, 5)


def test_rn_f32_rounds_once():
    assert R.rn_f32(Fraction(1, 3)) == np.float32(1 / 3)
    # halfway between two float32 values: ties to even, and just above: up
    one_ulp = Fraction(1, 2**23)
    assert R.rn_f32(1 + one_ulp / 2) == np.float32(1.0)
    assert R.rn_f32(1 + 3 * one_ulp / 2) == np.float32(1 + 2 * float(one_ulp))
    assert R.rn_f32(1 + one_ulp / 2 + Fraction(1, 2**80)) == np.float32(1 + float(one_ulp))
    # a value whose float64 rounding lands on a float32 tie: one rounding goes up, two would go to even
    q = 1 + one_ulp / 2 + Fraction(1, 2**60)
    assert np.float32(float(q)) == np.float32(1.0)
    assert R.rn_f32(q) == np.float32(1 + float(one_ulp))
    assert R.rn_f32(Fraction(-65535)) == np.float32(-65535)
    assert R.rn_f32(Fraction(1, 2**140)) == np.float32(2.0**-140)


@pytest.mark.parametrize("W,P", GRID)
def test_oracle_against_exact(W, P):
    """Copies are copies, and inside the parity set scipy's float32 edges are RN_f32(exact) wherever exact != 0."""
    for p, e, ref in _checked(W, P):
        np.testing.assert_array_equal(ref[e.copy], p.pool[e.copy].astype(np.float32))
        if R.in_parity_set(W, P):
            m = e.edge & np.array([q != 0 for q in e.exact])
            bad = np.flatnonzero(m & (ref != e.rn))
            assert len(bad) == 0, [(int(i), float(ref[i]), float(e.rn[i])) for i in bad[:5]]


def test_parity_rule_is_not_vacuous():
    """Outside the parity set, scipy's edges differ from RN_f32(exact) on the generated records of every plan with
    8 <= P <= W - 3 and W >= 13 of the grid (the rule is not looser than it needs to be there)."""
    outside = [(W, P) for W, P in GRID if not R.in_parity_set(W, P) and P <= W - 3 and W >= 13 and P >= 10]
    assert len(outside) >= 20
    for W, P in outside:
        n = 0
        for p, e, ref in _checked(W, P):
            m = e.edge & np.array([q != 0 for q in e.exact])
            n += int(np.sum(m & (ref != e.rn)))
        assert n > 0, (W, P)


TAB_PLANS = [(W, P) for W, P in GRID if W <= 33 or (W, P) in ((41, 20), (63, 8), (63, 12))]


@pytest.mark.parametrize("W,P", TAB_PLANS)
def test_plan_float_tables_are_the_rounded_exact_rows(W, P):
    """Every edge row of every table of the plan is the exact projection row rounded to float64, bit for bit (the device
    edge evaluation reads these), and the correlation weights are scipy's own coefficient bits, reversed."""
    from scipy.signal import savgol_coeffs

    plan = build_plan(W, P)
    H, stride = W // 2, plan.stride
    for t in range(plan.n_tables):
        w = 2 * t + 1
        if w <= P:
            continue
        h, base = w // 2, t * stride
        np.testing.assert_array_equal(plan.tab[base : base + w], savgol_coeffs(w, P)[::-1])
        for i in range(h):
            left = plan.tab[base + W + i * W : base + W + i * W + w]
            right = plan.tab[base + W + H * W + i * W : base + W + H * W + i * W + w]
            want_l = np.array([float(v) for v in R.hat_row_fraction(w, P, i)])
            want_r = np.array([float(v) for v in R.hat_row_fraction(w, P, w - h + i)])
            assert left.tobytes() == want_l.tobytes(), (W, P, w, "left", i)
            assert right.tobytes() == want_r.tobytes(), (W, P, w, "right", i)


INT_PLANS = [(W, P) for W, P in GRID if (W, P) not in R.LARGE_HIGH and W <= 33 or P <= 1]


@pytest.mark.parametrize("W,P", INT_PLANS)
def test_integer_plan_rows_and_worst_case(W, P):
    """The integer plan's numerators over den are the exact rows, and the worst-case sign pattern of every row stays
    below 2^31 (the int32 accumulator of the span kernels)."""
    plan = build_plan(W, P)
    if not plan.int_ok:
        return
    H = W // 2
    centre = [Fraction(int(v), plan.den) for v in plan.itab[:W][::-1]]
    assert centre == R.hat_row_fraction(W, P, H)
    for i in range(H):
        left = plan.itab[W + i * W : W + (i + 1) * W]
        right = plan.itab[W + H * W + i * W : W + H * W + (i + 1) * W]
        assert [Fraction(int(v), plan.den_edge) for v in left] == R.hat_row_fraction(W, P, i)
        assert [Fraction(int(v), plan.den_edge) for v in right] == R.hat_row_fraction(W, P, W - H + i)
    rows = {H: plan.itab[:W][::-1]}
    rows.update({i: plan.itab[W + i * W : W + (i + 1) * W] for i in range(H)})
    rows.update({W - H + i: plan.itab[W + H * W + i * W : W + H * W + (i + 1) * W] for i in range(H)})
    for r, win in R.worst_case_windows(W, P):
        acc = int(np.dot(rows[r].astype(np.int64), win.astype(np.int64)))
        assert abs(acc) < 2**31, (W, P, r, acc)
    # and the worst case is what the plan's own `fits` bound describes
    worst = max(sum(abs(int(v)) for v in row) for row in rows.values()) * R.X_MAX
    assert worst < 2**31


def test_integer_plans_exist_across_the_grid():
    ok = [(W, P) for W, P in INT_PLANS if build_plan(W, P).int_ok]
    assert any(W >= 33 for W, _ in ok) and any(P >= 10 for _, P in ok) and len(ok) >= 40


def test_plan_records_the_correlate1d_branch():
    """ndimage.correlate1d takes its anti-symmetric branch for scipy's near-identity weights of SG(5,4) and SG(9,8) (their
    noise is antisymmetric to within DBL_EPSILON, not symmetric); the plan must tell the device so."""
    from scipy.signal import savgol_coeffs

    eps = np.finfo(np.float64).eps
    for W, P in [(5, 4), (9, 8), (11, 2), (7, 6), (21, 20)]:
        plan = build_plan(W, P)
        fw = savgol_coeffs(W, P)[::-1]
        c = W // 2
        sym = all(abs(fw[c + i] - fw[c - i]) <= eps for i in range(1, c + 1))
        anti = all(abs(fw[c + i] + fw[c - i]) <= eps for i in range(1, c + 1))
        assert plan.symmetric[c] == (1 if sym else 2 if anti else 0), (W, P)
    assert build_plan(5, 4).symmetric[2] == 2 and build_plan(9, 8).symmetric[4] == 2


FIXTURES = ["sgbw_sg15_13", "sgbw_sg21_16", "sgbw_sg63_12", "sgbw_bw1", "sgbw_bw9", "sgbw_bw12"]


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_fixtures(name):
    """The reference's WavePoolFilteredPlugin / ThresholdHitPlugin outputs at the new corners (high-order SG edges,
    windows shrunk by short records, Butterworth orders above 8) equal the oracle's, bit for bit; and on the SG
    fixtures the parity rule holds: scipy's edges are RN_f32(exact) wherever the plan is in the parity set."""
    from tests import golden_util as G

    c = G.load_case(name)
    fp = G.filter_params(c)
    rec, pool = c["records"], c["wave_pool"]
    if fp["filter_type"] == "BW":
        from waveformanalysis_amd.filter_engine import design_bw

        sos, _, padlen = design_bw(fp["lowcut"], fp["highcut"], fp["fs"], fp["filter_order"])
        assert sos.shape[0] == fp["filter_order"] and np.any(rec["event_length"] <= padlen)
        want = O.filter_wave_pool(rec, pool, "BW", bw_sos=sos)
    else:
        W, P = fp["sg_window_size"], fp["sg_poly_order"]
        want = O.filter_wave_pool(rec, pool, "SG", sg_window_size=W, sg_poly_order=P)
        p = R.Pool(pool, rec["event_length"].astype(np.int64), rec["wave_offset"].astype(np.int64), [])
        e = R.expect(p, W, P)
        assert np.any(e.copy) or np.any(e.window[e.edge] < W)  # short records: copied or a shrunk window
        if R.in_parity_set(W, P):
            assert np.all(c["wave_pool_filtered"][e.edge] == e.rn[e.edge])
    np.testing.assert_array_equal(c["wave_pool_filtered"], want)
    hp = G.hit_params(c)
    G.assert_struct_equal(O.threshold_hits(rec, want, **hp), c["hits_filt"], float_rtol=0, what=name)
