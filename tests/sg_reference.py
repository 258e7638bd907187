"""Exact Savitzky-Golay reference and record generators for the plan-grid tests (tests/test_sg_grid_cpu.py,
tests/test_hip_sg_grid.py).

The reference filters a record with  savgol_filter(x_f32, w, P, mode="interp")  on its effective window w
(filtering.py:181-195): the degree-P least-squares polynomial of a w-sample window, evaluated at the window's centre
for interior samples and at the edge positions of the first / last w samples for the first / last w//2 samples.
Here that value is computed exactly, as a rational, and rounded once to float32.

The projection rows come from the discrete orthogonal (Gram) polynomials of the window, built with integer
arithmetic by the Stieltjes recurrence:  H[i][j] = sum_k q_k(i) q_k(j) / |q_k|^2.  This is a different derivation
from the plan's normal equations (waveformanalysis_amd/sg_plan.py), whose tables are what the tests check; nothing
here reads them.

Parity rule (`in_parity_set`): scipy evaluates the edge polynomial with np.polyfit, a least-squares solve whose
rounding error grows with the polynomial order.  Its float32 edge values equal RN_f32(exact) for the plans with
P <= PARITY_MAX_ORDER, except where the exact value is 0 (scipy then returns rounding noise, see
tests/golden/sgedge_zero.npz).  Above that order they depend on the LAPACK build and differ from the exact value.
"""

from __future__ import annotations

import dataclasses
import functools
import math
from fractions import Fraction

import numpy as np

MAX_WINDOW = 63
X_MAX = 65535
PARITY_MAX_ORDER = 6

# the plan grid: every odd window 1..63 with the orders below (restricted to P < W); windows above 23 take a subset of
# the orders and a handful of high-order plans, so that building the device plans stays within a few seconds
ORDERS = (0, 1, 2, 3, 4, 5, 6, 8, 10, 12)
LARGE_HIGH = ((25, 22), (27, 13), (31, 13), (31, 15), (33, 30), (41, 20), (63, 8), (63, 12), (63, 20))
EVEN_INPUTS = ((2, 0), (12, 2), (12, 5), (62, 3))  # raised by one by the plugin


def orders_for(W: int) -> list[int]:
    return sorted({p for p in (*ORDERS, W // 2, W - 3, W - 2, W - 1) if 0 <= p < W})


def plan_grid() -> list[tuple[int, int]]:
    plans = []
    for W in range(1, MAX_WINDOW + 1, 2):
        if W <= 23:
            plans += [(W, P) for P in orders_for(W)]
        else:  # two orders per window from the low end, rotating with W, plus P = W - 1 (a copy) for some
            low = [p for p in ORDERS if p <= 6]
            k = (W - 25) // 2
            plans += [(W, low[k % len(low)]), (W, low[(k + 3) % len(low)])]
    plans += list(LARGE_HIGH)
    plans += [(W, W - 1) for W in (33, 45)]
    return sorted(set(plans))


def in_parity_set(W: int, P: int) -> bool:
    """Plans whose scipy edge values equal RN_f32(exact) wherever the exact value is not 0."""
    return P <= PARITY_MAX_ORDER


def effective_window(L: int, W: int, P: int) -> int:
    """filtering.py:181-195: the window clamped to the record length and made odd; 0 when the filter copies."""
    w = min(W, L)
    if w % 2 == 0:
        w -= 1
    return 0 if w <= P else w


# ---- exact projection rows --------------------------------------------------------------------------------------
@functools.cache
def gram_basis(w: int, P: int) -> tuple[list[list[int]], list[int]]:
    """Integer vectors q_0..q_P orthogonal on the points 0..w-1, q_k a polynomial of degree k, and their norms."""
    x = list(range(w))
    q = [[1] * w]
    norms = [w]
    for k in range(P):
        qk = q[-1]
        xq = [xi * v for xi, v in zip(x, qk)]
        # q_{k+1} = x q_k - a q_k - b q_{k-1},  a = <x q_k, q_k>/|q_k|^2,  b = <x q_k, q_{k-1}>/|q_{k-1}|^2
        a = Fraction(sum(u * v for u, v in zip(xq, qk)), norms[-1])
        nxt = [Fraction(u) - a * v for u, v in zip(xq, qk)]
        if k > 0:
            b = Fraction(sum(u * v for u, v in zip(xq, q[-2])), norms[-2])
            nxt = [u - b * v for u, v in zip(nxt, q[-2])]
        den = math.lcm(*(v.denominator for v in nxt))
        ints = [int(v * den) for v in nxt]
        g = math.gcd(*ints)
        ints = [v // g for v in ints]
        q.append(ints)
        norms.append(sum(v * v for v in ints))
    return q, norms


@functools.cache
def hat_row(w: int, P: int, i: int) -> tuple[tuple[int, ...], int]:
    """Row i of the w x w least-squares projection, as integer numerators over one positive denominator."""
    q, norms = gram_basis(w, P)
    D = math.lcm(*norms)
    num = [0] * w
    for qk, nk in zip(q, norms):
        s = qk[i] * (D // nk)
        num = [a + s * v for a, v in zip(num, qk)]
    g = math.gcd(D, *num)
    return tuple(v // g for v in num), D // g


def hat_row_fraction(w: int, P: int, i: int) -> list[Fraction]:
    num, den = hat_row(w, P, i)
    return [Fraction(v, den) for v in num]


def row_abs_sum(w: int, P: int, i: int) -> Fraction:
    num, den = hat_row(w, P, i)
    return Fraction(sum(abs(v) for v in num), den)


# ---- exact values of a record ------------------------------------------------------------------------------------
def exact_record(x: np.ndarray, W: int, P: int) -> list[Fraction]:
    """Exact filtered value of every sample of one record (uint16 samples)."""
    L = len(x)
    w = effective_window(L, W, P)
    xs = [int(v) for v in x]
    if w == 0:
        return [Fraction(v) for v in xs]
    h = w // 2
    out = []
    cnum, cden = hat_row(w, P, h)
    for i in range(L):
        if i < h:
            num, den = hat_row(w, P, i)
            win = xs[:w]
        elif i >= L - h:
            num, den = hat_row(w, P, i - (L - w))
            win = xs[L - w :]
        else:
            num, den = cnum, cden
            win = xs[i - h : i + h + 1]
        out.append(Fraction(sum(a * b for a, b in zip(num, win)), den))
    return out


def sample_row(L: int, W: int, P: int, i: int) -> tuple[int, int]:
    """(effective window, hat row index) of sample i of a record of length L; (0, 0) for a copy."""
    w = effective_window(L, W, P)
    if w == 0:
        return 0, 0
    h = w // 2
    if i < h:
        return w, i
    if i >= L - h:
        return w, i - (L - w)
    return w, h


def rn_f32(q: Fraction) -> np.float32:
    """q rounded to the nearest float32, ties to even (one rounding, no float64 step)."""
    if q == 0:
        return np.float32(0.0)
    sign = -1 if q < 0 else 1
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, -126)  # subnormals share the exponent of the smallest normal
    scale = Fraction(2) ** (23 - e)
    m = a * scale
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(sign * float(Fraction(n) / scale))


def f32_ulp(v: float) -> float:
    v = abs(np.float32(v))
    return float(np.spacing(np.float32(v)))


def float_route_bound(w: int, P: int, i: int, x_max: int) -> float:
    """Bound on |f64 sum of e_k * x_k - exact| for a row e = RN_f64(exact row), summed left to right in float64:
    one rounding for each coefficient, product and addition, (w + 2) * 2^-53 * sum|row| * x_max (the +1 over w + 1
    covers the second-order terms)."""
    return float((w + 2) * Fraction(1, 2**53) * row_abs_sum(w, P, i) * x_max)


# ---- records ----------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Pool:
    pool: np.ndarray      # uint16
    lengths: np.ndarray   # int64
    offsets: np.ndarray   # int64
    kinds: list           # value pattern of each record

    def records(self):
        from waveformanalysis_amd.dtypes import RECORDS_DTYPE

        rec = np.zeros(len(self.lengths), dtype=RECORDS_DTYPE)
        rec["record_id"] = np.arange(len(rec))
        rec["event_length"] = self.lengths
        rec["wave_offset"] = self.offsets
        rec["timestamp"] = np.arange(len(rec)) * 1000
        rec["dt"] = 4
        rec["baseline"] = np.nan
        return rec

    def slices(self):
        for o, n in zip(self.offsets, self.lengths):
            yield int(o), int(n)


def _pattern(kind: str, L: int, rng) -> np.ndarray:
    t = np.arange(L)
    if kind == "pedestal":  # small values: |numerators| below the integer guard, the float64 chain decides
        v = rng.integers(0, 4, L)
    elif kind == "mid":
        v = 8000 + rng.integers(-300, 301, L)
    elif kind == "high":
        v = 65535 - rng.integers(0, 40, L)
    elif kind == "const":
        v = np.full(L, int(rng.integers(1, 65536)))
    elif kind == "alternate":
        v = np.where(t % 2 == 0, 0, 65535)
    elif kind == "pulse":  # pedestal with a pulse: negative edge numerators, large curvature
        v = 8000 - np.maximum(0, 6000 - 900 * np.abs(t - int(rng.integers(0, max(L, 1))))) + rng.integers(-3, 4, L)
    else:
        raise ValueError(kind)
    return np.clip(v, 0, X_MAX).astype(np.uint16)


KINDS = ("pedestal", "mid", "high", "const", "alternate", "pulse")


def record_lengths(W: int, P: int, long_length: int = 400) -> list[int]:
    """0, 1, 2, P, P+1, P+2, W-1, W, W+1, 2W+3 (even lengths shrink the window) and a long record."""
    return sorted({0, 1, 2, P, P + 1, P + 2, max(W - 1, 0), W, W + 1, 2 * W + 3, long_length} - {-1})


def worst_case_windows(W: int, P: int) -> list[tuple[int, np.ndarray]]:
    """(row, W samples): 65535 where the exact row is positive, 0 elsewhere, and the opposite sign, for the centre row
    and every edge row of the full window."""
    out = []
    for i in range(W):
        num, _ = hat_row(W, P, i)
        pos = np.array([X_MAX if v > 0 else 0 for v in num], dtype=np.uint16)
        neg = np.array([X_MAX if v < 0 else 0 for v in num], dtype=np.uint16)
        out += [(i, pos), (i, neg)]
    return out


def ragged_pool(W: int, P: int, seed: int = 0) -> Pool:
    """Every record length of `record_lengths` with every value pattern, plus the worst-case sign patterns, packed with
    gaps of 3 samples between records."""
    rng = np.random.default_rng(seed + 1000 * W + P)
    chunks, lengths, kinds = [], [], []
    for L in record_lengths(W, P):
        for kind in KINDS:
            chunks.append(_pattern(kind, L, rng))
            lengths.append(L)
            kinds.append(kind)
    if W > P:
        for i, win in worst_case_windows(W, P):
            chunks.append(win.copy())  # record length W: row i of the full window is sample i
            lengths.append(W)
            kinds.append(f"worst{i}")
    return _pack(chunks, lengths, kinds, gap=3)


def uniform_pool(W: int, P: int, L: int = 48, seed: int = 0) -> Pool:
    """Equal-length contiguous records (the span layout): each pattern, and the worst-case sign patterns placed at the
    record start (left edge rows), at the record end (right edge rows) and in the middle (centre row)."""
    assert L >= W
    rng = np.random.default_rng(seed + 7 + 1000 * W + P)
    chunks, kinds = [], []
    for kind in KINDS:
        for _ in range(3):
            chunks.append(_pattern(kind, L, rng))
            kinds.append(kind)
    if W > P:
        h = W // 2
        for i, win in worst_case_windows(W, P):
            x = _pattern("mid", L, rng)
            if i < h:
                x[:W] = win
            elif i > h:
                x[L - W :] = win
            else:
                c = L // 2
                x[c - h : c + h + 1] = win
            chunks.append(x)
            kinds.append(f"worst{i}")
    return _pack(chunks, [L] * len(chunks), kinds, gap=0)


def _pack(chunks, lengths, kinds, gap):
    offsets, parts, pos = [], [], 0
    fill = np.full(gap, 12345, dtype=np.uint16)
    for c in chunks:
        offsets.append(pos)
        parts += [c, fill]
        pos += len(c) + gap
    pool = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint16)
    return Pool(pool.astype(np.uint16), np.asarray(lengths, dtype=np.int64), np.asarray(offsets, dtype=np.int64), kinds)


# ---- per-pool expectations ---------------------------------------------------------------------------------------
@dataclasses.dataclass
class Expect:
    exact: list            # Fraction per pool sample (0 in the gaps)
    rn: np.ndarray         # float32 RN_f32(exact), 0.0 in the gaps
    edge: np.ndarray       # bool: an edge sample of a filtered record (scipy's polyfit branch)
    interior: np.ndarray   # bool: an interior sample of a filtered record (scipy's correlate branch)
    copy: np.ndarray       # bool: a sample of a record the filter copies
    bound: np.ndarray      # float64: float-route bound of the sample's row
    window: np.ndarray     # effective window of the sample's record (0: copy / gap)
    row: np.ndarray        # hat row index of the sample


def expect(p: Pool, W: int, P: int) -> Expect:
    n = len(p.pool)
    exact = [Fraction(0)] * n
    rn = np.zeros(n, dtype=np.float32)
    edge = np.zeros(n, dtype=bool)
    interior = np.zeros(n, dtype=bool)
    copy = np.zeros(n, dtype=bool)
    bound = np.zeros(n)
    window = np.zeros(n, dtype=np.int64)
    row = np.zeros(n, dtype=np.int64)
    for o, L in p.slices():
        x = p.pool[o : o + L]
        vals = exact_record(x, W, P)
        for i, q in enumerate(vals):
            exact[o + i] = q
            rn[o + i] = rn_f32(q)
            w, r = sample_row(L, W, P, i)
            window[o + i], row[o + i] = w, r
            if w == 0:
                copy[o + i] = True
                continue
            if r == w // 2 and (w // 2 <= i < L - w // 2):
                interior[o + i] = True
            else:
                edge[o + i] = True
            bound[o + i] = float_route_bound(w, P, r, int(x.max()))
    return Expect(exact, rn, edge, interior, copy, bound, window, row)


def within_bound(got: np.ndarray, e: Expect, idx: np.ndarray) -> np.ndarray:
    """|got - exact| <= bound + one float32 ulp of the exact value, per index (exact rational comparison)."""
    ok = np.ones(len(idx), dtype=bool)
    for k, i in enumerate(idx):
        q = e.exact[i]
        d = abs(Fraction(float(got[i])) - q)
        lim = Fraction(float(e.bound[i])) + Fraction(f32_ulp(float(e.rn[i])))
        ok[k] = d <= lim
    return ok
