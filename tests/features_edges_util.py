"""Record sets that put the per-record feature kernels (basic_features, waveform_width_integral) on the edges where a
reduction in a different order would give different bits, and small numpy models of those orders.

The kernels promise numpy's float64 results bit for bit: np.sum through numpy's pairwise tree (`pairwise`), np.cumsum +
np.searchsorted(side="left") sequentially.  Most synthetic data cannot tell the orders apart (integer samples around a
40-sample-mean baseline add exactly; float32 terms add exactly in float64), so the sets here are built to:
  wide          samples over the whole uint16 range, baseline = mean of the first 40: the order of the float64 additions
                shows in the last bits of most sums
  pulsed_tail   a noisy baseline, one large pulse and an above-baseline tail: the tail's x = 0 terms make the cumulative
                sum plateau, so targets near q -> 1 tie with many cumulative values
  integer_ties  integer samples, baseline 8000.0: every partial sum is exact and the cumulative sum hits q * total
                exactly for q = 0.25 / 0.5 / 0.75, at a sample followed by x = 0 terms (side="left" decides)
  ragged        records of many lengths (0 .. 1500) in one run, from an unaligned start

Every generator is deterministic in its seed and returns (records, wave_pool); the models take one row per record.
`test_features_edges_cpu.py` proves with the models that the sets do separate the orders; `test_hip_features_edges.py`
runs them through the kernels.
"""

from __future__ import annotations

import numpy as np

from waveformanalysis_amd.dtypes import RECORDS_DTYPE

BASELINE_SAMPLES = 40
RAGGED_LENGTHS = (0, 1, 2, 7, 8, 9, 23, 24, 39, 40, 41, 89, 90, 91, 127, 128, 129, 800, 1500)
POLARITIES = ("unknown", "negative", "positive")
U = 2.0 ** -53  # unit roundoff of float64


def _mean_baseline(w: np.ndarray) -> float:
    """np.mean over float64 of the first 40 samples (exact integer sum / count), 32767.5 for an empty record."""
    n = min(BASELINE_SAMPLES, len(w))
    return float(np.sum(w[:n], dtype=np.int64)) / n if n else 32767.5


def assemble(waves, polarity="unknown", baselines=None, lead=0):
    """(records, wave_pool) with the records back to back from sample `lead`; baseline = mean of the first 40 samples
    unless given; polarity: one string for all, or one per record."""
    n = len(waves)
    lens = np.array([len(w) for w in waves], dtype=np.int64)
    rec = np.zeros(n, dtype=RECORDS_DTYPE)
    rec["wave_offset"] = lead + np.concatenate(([0], np.cumsum(lens)[:-1])) if n else 0
    rec["event_length"] = lens
    rec["baseline"] = [_mean_baseline(w) for w in waves] if baselines is None else baselines
    rec["baseline_upstream"] = np.nan
    rec["polarity"] = polarity
    rec["record_id"] = np.arange(n)
    rec["timestamp"] = np.arange(n, dtype=np.int64) * 10_000 + 7
    rec["dt"] = 2
    rec["board"] = np.arange(n) % 3
    rec["channel"] = np.arange(n) % 16
    pool = np.concatenate([np.full(lead, 12345, np.uint16)] + [np.asarray(w, np.uint16) for w in waves] +
                          [np.full(8, 54321, np.uint16)])
    return rec, pool


def wide(n_rec: int, L: int, polarity: str = "unknown", seed: int = 0):
    """Uniform records of L samples drawn over 0 .. 65535."""
    rng = np.random.default_rng(1000 + seed)
    w = rng.integers(0, 65536, size=(n_rec, L), dtype=np.uint16)
    return assemble(list(w), polarity)


def pulsed_tail(n_rec: int, L: int, polarity: str = "unknown", seed: int = 0):
    """Noisy baseline near 8000, one large pulse (in the record's signal direction), then a tail above the baseline
    (below it for "positive"): x = max(signal, 0) is zero there."""
    rng = np.random.default_rng(2000 + seed)
    sgn = 1 if polarity == "positive" else -1  # sample direction of a pulse
    w = 8000 + rng.normal(0, 3, size=(n_rec, L))
    for r in range(n_rec):
        tail = int(rng.integers(1, max(2, L // 4)))
        lo = min(BASELINE_SAMPLES, L // 3)
        width = int(rng.integers(1, max(2, min(L // 6, L - tail - lo))))
        at = int(rng.integers(lo, max(lo + 1, L - tail - width)))
        w[r, at:at + width] += sgn * rng.uniform(200, 3000) * np.hanning(width + 2)[1:-1]
        w[r, L - tail:] -= sgn * rng.uniform(10, 40)
    return assemble(list(np.clip(np.rint(w), 0, 65535).astype(np.uint16)), polarity)


def integer_ties(n_rec: int, L: int, polarity: str = "unknown", seed: int = 0, parts: int = 4):
    """Integer samples around an integer baseline (8000.0): the signal is `parts` runs of positive integer terms with
    equal sums K, each followed by a plateau of x = 0 terms (samples on or beyond the baseline).  The cumulative sum
    equals j * K = (j / parts) * total exactly at the last term of run j."""
    rng = np.random.default_rng(3000 + seed)
    sgn = 1 if polarity == "positive" else -1
    seg = L // parts
    waves = []
    for _ in range(n_rec):
        s = np.zeros(L, dtype=np.int64)
        K = int(rng.integers(200, 5000))
        for j in range(parts):
            m = int(rng.integers(1, max(2, seg // 2)))  # terms of run j, then >= seg - m zero terms
            cuts = np.sort(rng.choice(np.arange(1, K), size=min(m - 1, K - 1), replace=False)) if m > 1 else []
            s[j * seg: j * seg + len(cuts) + 1] = np.diff(np.concatenate(([0], cuts, [K])))
        z = s == 0
        s[z] = -rng.integers(0, 6, size=int(z.sum()))  # zero or past the baseline: clipped to x = 0
        waves.append((8000 + sgn * s).astype(np.uint16))
    return assemble(waves, polarity, baselines=np.full(n_rec, 8000.0))


def ragged(seed: int = 0, lengths=RAGGED_LENGTHS, lead: int = 3):
    """Records of the given lengths over 0 .. 65535, polarities cycling unknown / negative / positive."""
    rng = np.random.default_rng(4000 + seed)
    waves = [rng.integers(0, 65536, size=L, dtype=np.uint16) for L in lengths]
    pol = [POLARITIES[i % 3] for i in range(len(lengths))]
    return assemble(waves, pol, lead=lead)


# -- the terms the reference sums -----------------------------------------------------------------------------------
def signal_rows(rec: np.ndarray, pool: np.ndarray, c0: int = 0, c1: int | None = None) -> np.ndarray:
    """float64 terms of uniform records over [c0, c1): float32 (wave - baseline), negated unless "positive", for known
    polarities; baseline - wave in float64 otherwise (oracle.basic_features's area terms)."""
    L = int(rec["event_length"][0])
    W = pool[int(rec["wave_offset"][0]): int(rec["wave_offset"][0]) + len(rec) * L].reshape(len(rec), L)
    W = W[:, c0:c1]
    b = rec["baseline"][:, None]
    known = np.isin(rec["polarity"], ("negative", "positive"))[:, None]
    pos = (rec["polarity"] == "positive")[:, None]
    s32 = W.astype(np.float32) - b.astype(np.float32)
    s32 = np.where(pos, s32, -s32).astype(np.float64)
    return np.where(known, s32, b - W.astype(np.float64))


def width_terms(rec: np.ndarray, pool: np.ndarray) -> np.ndarray:
    """x = max(signal, 0) of uniform records (oracle.width_integral)."""
    L = int(rec["event_length"][0])
    W = pool[int(rec["wave_offset"][0]): int(rec["wave_offset"][0]) + len(rec) * L].reshape(len(rec), L)
    b = rec["baseline"][:, None]
    known = np.isin(rec["polarity"], ("negative", "positive"))[:, None]
    pos = (rec["polarity"] == "positive")[:, None]
    s32 = W.astype(np.float32) - b.astype(np.float32)
    s32 = np.where(pos, s32, -s32).astype(np.float64)
    raw = W.astype(np.float64) - b
    return np.maximum(np.where(known, s32, np.where(pos, raw, -raw)), 0.0)


# -- models of summation orders (one row per record, every addition an elementwise float64 add) ---------------------
def _leaf(X: np.ndarray, combine: str) -> np.ndarray:
    n = X.shape[1]
    if n < 8:
        res = np.zeros(X.shape[0])
        for i in range(n):
            res = res + X[:, i]
        return res
    m = n - n % 8
    r = X[:, :8].copy()
    for i in range(8, m, 8):
        r = r + X[:, i:i + 8]
    if combine == "tree":
        res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    else:  # "sequential": r0 + r1 + ... + r7
        res = r[:, 0].copy()
        for j in range(1, 8):
            res = res + r[:, j]
    for i in range(m, n):
        res = res + X[:, i]
    return res


def _pw(X: np.ndarray, split8: bool, combine: str) -> np.ndarray:
    n = X.shape[1]
    if n <= 128:
        return _leaf(X, combine)
    n2 = n // 2
    if split8:
        n2 -= n2 % 8
    return _pw(X[:, :n2], split8, combine) + _pw(X[:, n2:], split8, combine)


def pairwise(X: np.ndarray, split8: bool = True, combine: str = "tree") -> np.ndarray:
    """np.sum of each row: 0.0 + the pairwise sums of numpy's 8192-element reduce blocks, in order.  split8=False /
    combine="sequential" are the wrong orders the premise tests compare against."""
    X = np.asarray(X, dtype=np.float64)
    total = np.zeros(X.shape[0])
    for a in range(0, X.shape[1], 8192):
        total = total + _pw(X[:, a:a + 8192], split8, combine)
    return total


def sequential(X: np.ndarray) -> np.ndarray:
    """Left-to-right sum of each row (np.cumsum's last value)."""
    X = np.asarray(X, dtype=np.float64)
    return np.cumsum(X, axis=1)[:, -1] if X.shape[1] else np.zeros(X.shape[0])


def blocked_cumsum(X: np.ndarray) -> np.ndarray:
    """Cumulative sums in the order the lane-per-leaf kernel forms them: each 8-sample chunk summed as a tree, a running
    prefix over the chunks, and inside a chunk the terms added one by one to the prefix in front of it."""
    X = np.asarray(X, dtype=np.float64)
    R, n = X.shape
    out = np.empty_like(X)
    pre = np.zeros(R)
    for a in range(0, n, 8):
        c = X[:, a:a + 8]
        run = pre.copy()
        for j in range(c.shape[1]):
            run = run + c[:, j]
            out[:, a + j] = run
        if c.shape[1] == 8:
            pre = pre + (((c[:, 0] + c[:, 1]) + (c[:, 2] + c[:, 3])) + ((c[:, 4] + c[:, 5]) + (c[:, 6] + c[:, 7])))
        else:
            pre = run
    return out


def searchsorted_rows(C: np.ndarray, t: np.ndarray) -> np.ndarray:
    """np.searchsorted(C[r], t[r], side="left") per row."""
    return np.array([int(np.searchsorted(C[r], t[r], side="left")) for r in range(C.shape[0])], dtype=np.int64)


def quantile_targets(X: np.ndarray, q: float) -> np.ndarray:
    return q * pairwise(X)


def near_target(X: np.ndarray, q: float) -> np.ndarray:
    """Records whose sequential cumulative sum has a value within 8 L 2^-53 target of q * total (the band inside
    which the leaf kernel leaves the decision to numpy's own order); only records with total > 0."""
    L = X.shape[1]
    t = quantile_targets(X, q)
    C = np.cumsum(X, axis=1)
    tol = 8.0 * L * U * t
    return (np.abs(C - t[:, None]) <= tol[:, None]).any(axis=1) & (t > 0)


# -- the runs the GPU tests use (the CPU premise tests check the same runs) -----------------------------------------
SWEEP_SHORT = tuple(range(0, 137))                                               # area lengths on 256-sample records
SWEEP_LONG = (255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4104, 8184, 8192)     # ... on 8192-sample records
SWEEP_STARTS = (0, 8, 64, 3)  # area starts: a multiple of 8 takes the lane-per-leaf kernel, 3 the general one
NEXTAFTER_ONE = float(np.nextafter(1.0, 0.0))
TINY_Q = (5e-324, 1e-300)
TIE_RECORDS = 40_000  # more than twice k_width_ties' 256 x 64 lanes


def sweep_runs(polarity: str):
    """{record length: (records, pool)} of wide data for the area-length sweep."""
    return {256: wide(128, 256, polarity, seed=11), 8192: wide(24, 8192, polarity, seed=12)}


def sweep_cases():
    """(record length, area start, area length) of the sweep, every area inside the record."""
    for L, lengths in ((256, SWEEP_SHORT), (8192, SWEEP_LONG)):
        for c0 in SWEEP_STARTS:
            for n in lengths:
                if c0 + n <= L:
                    yield L, c0, n


def with_special_records(rec: np.ndarray, pool: np.ndarray, lead_zeros: int = 0):
    """Copies in which record 3 has no positive term (q_total = 0) and records 4 / 5 / 6 a single one (inside, first
    and last sample); with lead_zeros > 0 every record starts with that many x = 0 terms.  Unknown / negative
    polarity (a sample above the baseline is x = 0)."""
    rec, pool = rec.copy(), pool.copy()
    L = int(rec["event_length"][0])
    W = pool[int(rec["wave_offset"][0]):][:len(rec) * L].reshape(len(rec), L)
    hi = np.uint16(min(65535, int(rec["baseline"].max()) + 500))
    if lead_zeros:
        W[:, :lead_zeros] = hi
    for r, at in ((3, None), (4, L // 2), (5, 0), (6, L - 1)):
        if r < len(rec):
            W[r] = hi
            if at is not None:
                W[r, at] = np.uint16(max(0, int(rec["baseline"][r]) - 700))
    return rec, pool


QUANTILE_RUNS = {  # name -> () -> (records, pool), uniform, width quantile edges
    "pulsed_800_unknown": lambda: with_special_records(*pulsed_tail(1000, 800, "unknown", seed=21)),
    "pulsed_800_negative": lambda: with_special_records(*pulsed_tail(600, 800, "negative", seed=22)),
    "wide_800": lambda: with_special_records(*wide(500, 800, "unknown", seed=23)),
    "pulsed_64_lead_zeros": lambda: with_special_records(*pulsed_tail(800, 64, "unknown", seed=24), lead_zeros=13),
    "pulsed_800_lead_zeros": lambda: with_special_records(*pulsed_tail(400, 800, "unknown", seed=25), lead_zeros=37),
}
QUANTILES = ((0.1, NEXTAFTER_ONE), (TINY_Q[0], 0.9), (TINY_Q[1], 0.9), (TINY_Q[0], NEXTAFTER_ONE))


def slice_values(L: int):
    """height_range / area_range bounds around the edges of an L-sample record (None: the slice's default)."""
    return (None, -L - 5, -L, -L + 1, -41, -1, 0, 1, 7, 8, 9, 40, L - 1, L, L + 1, L + 100)


def slice_pairs(L: int):
    vals = slice_values(L)
    return [(s, e) for s in vals for e in vals]
