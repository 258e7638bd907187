"""Inputs and an independent reference for the rows of the threshold-hit pass (reference: hit_finder.py:329-413).

The hit *mask* is pinned by tests/boundary_util.py.  The sets built here pin what a row then says about its run: the
window  [start - le, end + re)  clamped to  [0, max_len),  the first maximum inside it, the integral of the positive
part, rise / fall time with their clamp at 0, the edges clamped to the record, and the timestamp.  Families:

  A  window clamp and asymmetric extensions (runs from sample 0, to sample L, one sample wide, the whole record;
     ragged records whose windows reach the zero padding of a matrix wider than the longest record);
  B  a higher neighbouring run inside the extension window (the position leaves the hit's own run);
  C  ties for the maximum (saturated plateaus, mirrored overshoots of the filter, twin pulses, padding samples);
  D  the sign of the integral's terms and the baselines that decide which row kernel takes a hit;
  E  the shapes of k_hit_rows_flat's work lists (64 hits per wave, kFlatCap chunks per batch, the edge list, the
     literal list's capacity).

Every record's threshold is  +-(baseline - pedestal) + level  with the level between the pedestal and the pulse, so
any baseline (0, negative, 262144, not representable in float32) gives the same runs.

`hit_rows_exact` restates the rows in plain Python: scalar loops for the runs and the first maximum, the integral as a
`fractions.Fraction` sum rounded once.  tests/test_hit_rows_cpu.py holds the oracle to it and counts, per family, the
rows that show the family's rule.
"""

from __future__ import annotations

import dataclasses
import functools
from fractions import Fraction

import numpy as np

from oracle import wfa_oracle as O
from waveformanalysis_amd.dtypes import RECORDS_DTYPE, THRESHOLD_HIT_DTYPE

# k_hit_rows_flat's constants (wfa_kernels.hip) and the literal list's capacity (wfa_capi.hip)
FLAT_HITS = 64
FLAT_CAP = 2048
LIT_CAP = 65536
ADC_MAX = 16383


# ---- the independent reference ------------------------------------------------------------------------------------
def _round_f32(q: Fraction) -> np.float32:
    """The float32 nearest to the rational q (ties to even): one rounding."""
    x = np.float32(float(q))
    cands = [x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))]
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - q), int(c.view(np.uint32)) & 1))


def hit_rows_exact(records, source_pool, thresholds, le, re, max_len, last_max=False, details=False, halo=0):
    """Rows of hit_finder.py:329-413 without numpy's reductions.  Samples in [L, max_len) are 0 (the padded matrix).

    details=True: also a dict of per-row arrays: `start`, `end` (the run), `seg_start`, `seg_end`, `ties` (how often
    the window holds its maximum), `tie_zones` (where the tied maxima lie: 1 for i < halo, 2 for halo <= i < L - halo,
    4 for L - halo <= i < L, 8 for the padding, or-ed) and `sum_exact` (the float64 sum in index order equals the
    rational sum)."""
    le, re = max(0, int(le)), max(0, int(re))
    max_len = int(max_len)
    rows = []
    det = {k: [] for k in ("start", "end", "seg_start", "seg_end", "ties", "tie_zones", "sum_exact")}
    for r in range(len(records)):
        L = int(records["event_length"][r])
        off = int(records["wave_offset"][r])
        b = float(records["baseline"][r])
        thr = float(thresholds[r])
        positive = str(records["polarity"][r]) == "positive"
        dt = int(records["dt"][r])
        ts = int(records["timestamp"][r])
        y = [float(v) for v in source_pool[off:off + L]] + [0.0] * (max_len - L)
        sig = [(w - b) if positive else (b - w) for w in y]
        i = 0
        while i < L:
            if not sig[i] >= thr:
                i += 1
                continue
            start = i
            while i < L and sig[i] >= thr:
                i += 1
            end = i
            seg_start, seg_end = max(0, start - le), min(max_len, end + re)
            if seg_end <= seg_start:
                continue
            pos = seg_start
            for k in range(seg_start, seg_end):
                if sig[k] > sig[pos] or (last_max and sig[k] == sig[pos]):
                    pos = k
            total = Fraction(0)
            running = 0.0
            for k in range(seg_start, seg_end):
                if sig[k] > 0.0:
                    total += Fraction(sig[k])
                    running += sig[k]
            edge_start = min(seg_start, max(L, 0))
            edge_end = max(min(seg_end, max(L, 0)), edge_start)
            rows.append((pos, np.float32(sig[pos]), _round_f32(total), edge_start, edge_end,
                         np.float32(edge_end - edge_start), dt, np.float32(max(pos - start, 0) * dt),
                         np.float32(max(end - 1 - pos, 0) * dt), int(float(ts) + pos * (dt * 1e3)),
                         int(records["board"][r]), int(records["channel"][r]), int(records["record_id"][r])))
            det["start"].append(start)
            det["end"].append(end)
            det["seg_start"].append(seg_start)
            det["seg_end"].append(seg_end)
            tied = [k for k in range(seg_start, seg_end) if sig[k] == sig[pos]]
            det["ties"].append(len(tied))
            det["tie_zones"].append(sum({(8 if k >= L else 4 if k >= L - halo else 2 if k >= halo else 1) for k in tied}))
            det["sum_exact"].append(Fraction(running) == total)
    out = np.array(rows, dtype=THRESHOLD_HIT_DTYPE) if rows else np.zeros(0, dtype=THRESHOLD_HIT_DTYPE)
    if details:
        return out, {k: np.asarray(v, dtype=bool if k == "sum_exact" else np.int64) for k, v in det.items()}
    return out


def oracle_rows(records, source_pool, thresholds, le, re, max_len=0):
    """O.threshold_hits; for a matrix wider than the longest record, its body with the wider zero-padded matrix."""
    longest = int(records["event_length"].max())
    if max_len <= longest:
        return O.threshold_hits(records, source_pool, thresholds=thresholds, left_extension=le, right_extension=re)
    waves, valid = O.waves_padded(records, source_pool, dtype=np.float64)
    waves = np.pad(waves, ((0, 0), (0, max_len - longest)))
    valid = np.pad(valid, ((0, 0), (0, max_len - longest)))
    b2 = records["baseline"].astype(np.float64)[:, np.newaxis]
    positive = O.positive_mask_from_polarity(records)
    signal = np.where(positive[:, np.newaxis], waves - b2, b2 - waves)
    return O.hits_from_signal_matrix(
        signal, np.asarray(thresholds, dtype=np.float64), records["timestamp"].astype(np.int64),
        records["board"].astype(np.int16), records["channel"].astype(np.int16), records["record_id"].astype(np.int64),
        max(0, int(le)), max(0, int(re)), records["dt"].astype(np.int32), valid, records["event_length"].astype(np.int64))


# ---- a generated set ----------------------------------------------------------------------------------------------
@dataclasses.dataclass(eq=False)
class HitSet:
    name: str
    family: str
    records: np.ndarray
    pool: np.ndarray
    thresholds: np.ndarray
    source: str                 # "raw" or "sg"
    plan: tuple                 # Savitzky-Golay (window, order) of the "sg" source
    layout: str                 # "stream" (uniform, L % 32 == 0), "padded" (uniform, L % 16 != 0), "ragged"
    ext: tuple                  # the (left_extension, right_extension) pairs the set is run with
    max_len: int                # 0: the longest record
    dyadic: bool                # every baseline is a multiple of 2^-23: the integral is exact on every route
    window: tuple | None        # baseline window of the fused-baseline pass that gives records["baseline"]

    @functools.cached_property
    def filtered(self):
        if self.source == "raw":
            return None
        W, P = self.plan
        if self.layout != "ragged":
            L = int(self.records["event_length"][0])
            return O.filter_wave_pool_uniform(self.pool, L, sg_window_size=W, sg_poly_order=P)
        return O.filter_wave_pool(self.records, self.pool, sg_window_size=W, sg_poly_order=P)

    @property
    def src_pool(self):
        return self.pool if self.source == "raw" else self.filtered

    @property
    def width(self) -> int:
        return self.max_len or int(self.records["event_length"].max())

    @property
    def H(self) -> int:
        return self.plan[0] // 2

    @functools.cache
    def oracle(self, le, re):
        return oracle_rows(self.records, self.src_pool, self.thresholds, le, re, self.max_len)

    @functools.cache
    def exact(self, le, re, last_max=False):
        return hit_rows_exact(self.records, self.src_pool, self.thresholds, le, re, self.width, last_max=last_max,
                              details=True, halo=self.H)


def flat_chunks(hs: HitSet, le, re):
    """k_hit_rows_flat's view of every row of hs.exact(le, re): (chunks of the interior window, edge-list samples).
    Interior: window samples in [H, L - H), as aligned 8-sample chunks of the pool; the rest goes to the edge list."""
    rows, det = hs.exact(le, re)
    H = hs.H
    row_of = {int(i): k for k, i in enumerate(hs.records["record_id"])}
    chunks, edges = [], []
    for k in range(len(rows)):
        r = row_of[int(rows["record_id"][k])]
        L, off = int(hs.records["event_length"][r]), int(hs.records["wave_offset"][r])
        if hs.layout == "padded":  # the shadow copy: records at stride roundup16(L)
            off = r * ((L + 15) // 16 * 16)
        s0, s1 = int(det["seg_start"][k]), int(det["seg_end"][k])
        ilo, ihi = max(s0, H), min(s1, L - H)
        chunks.append(((off + ihi - 1) >> 3) - ((off + ilo) >> 3) + 1 if ihi > ilo else 0)
        edges.append(max(min(s1, H) - s0, 0) + max(s1 - max(s0, L - H), 0))
    return np.asarray(chunks), np.asarray(edges)


# ---- building blocks ----------------------------------------------------------------------------------------------
BIG_TS = (2**53 + 1, 2**53 + 123457, 2**60 + 3, 2**62 - 10**9 - 1, 2**62 + 777)


def _pack(name, family, waves, ped, level, baseline, positive, *, source, plan, layout, ext, max_extra=0, dyadic=True,
          window=None, gap_of=None) -> HitSet:
    """Records back to back (ragged: `gap_of(r)` unused samples of 0 / ADC_MAX in front of record r)."""
    n = len(waves)
    lengths = np.array([len(w) for w in waves], dtype=np.int64)
    gaps = np.array([gap_of(r) if gap_of else 0 for r in range(n)], dtype=np.int64)
    offs = np.cumsum(gaps + np.concatenate([[0], lengths[:-1]]))
    pool = np.zeros(int(offs[-1] + lengths[-1]), dtype=np.uint16)
    rec = np.zeros(n, dtype=RECORDS_DTYPE)
    rec["wave_offset"], rec["event_length"] = offs, lengths
    rec["timestamp"] = 10**12 + np.cumsum(lengths * 4000)
    for k, t in enumerate(BIG_TS):
        rec["timestamp"][(7 + 11 * k) % n] = t
    rec["dt"] = np.array([1, 2, 4])[np.arange(n) % 3]
    rec["record_id"] = np.arange(n)
    rec["board"], rec["channel"] = np.arange(n) // 1000, np.arange(n) % 1000
    positive = np.broadcast_to(np.asarray(positive, dtype=bool), (n,))
    rec["polarity"] = np.where(positive, "positive", np.where(np.arange(n) % 2 == 0, "unknown", "negative"))
    baseline = np.asarray(baseline, dtype=np.float64).copy()
    if window is not None:  # the fused baseline pass: mean of the raw samples [start, min(end, L))
        for r, w in enumerate(waves):
            e = min(window[1], len(w))
            n_win = e - window[0]
            if n_win & (n_win - 1):  # no power of two (the streaming kernel fuses the window (0, 40) only): take single
                k = window[0]        # counts off the window's samples until their mean is an integer
                for _ in range(int(np.sum(w[window[0]:e], dtype=np.int64)) % n_win):
                    while w[k] == 0:
                        k = window[0] + (k + 1 - window[0]) % n_win
                    w[k] -= 1
                    k = window[0] + (k + 1 - window[0]) % n_win
            baseline[r] = float(int(np.sum(w[window[0]:e], dtype=np.int64))) / float(e - window[0])
    rec["baseline"] = baseline
    pool[1::2] = ADC_MAX  # what the gaps hold
    for o, w in zip(offs, waves):  # (after the adjustment above: the pool holds what the baseline is the mean of)
        pool[o:o + len(w)] = w
    ped = np.asarray(ped, dtype=np.float64)
    thr = np.where(positive, ped - baseline, baseline - ped) + np.asarray(level, dtype=np.float64)
    return HitSet(name, family, rec, pool, thr, source, tuple(plan), layout, tuple(ext),
                  int(lengths.max()) + max_extra if max_extra else 0, dyadic, window)


def _wave(s, ped, positive, noise=None):
    w = ped + s if positive else ped - s
    if noise is not None:
        w = w + noise
    return np.clip(w, 0, ADC_MAX).astype(np.uint16)


def _flat(s, a, m, h):
    a, e = max(int(a), 0), min(int(a) + int(m), len(s))
    s[a:e] = np.maximum(s[a:e], h)


def _spike_level(source, plan):
    """Level fraction that leaves a one-sample run of a one-sample spike: between the filter's two largest taps."""
    if source == "raw":
        return 0.5
    from scipy.signal import savgol_coeffs
    c = np.sort(savgol_coeffs(plan[0], plan[1]))[::-1]
    return float(c[0] + c[1]) / 2


# (source, plan, layout, polarity): polarity True / False for the uniform layouts (one polarity class), None: mixed
VARIANTS = (
    ("raw", (5, 2), "stream", False),
    ("sg", (5, 2), "stream", False),
    ("sg", (11, 2), "stream", True),
    ("sg", (5, 2), "padded", True),
    ("sg", (11, 2), "padded", False),
    ("raw", (5, 2), "ragged", None),
    ("sg", (5, 2), "ragged", None),
    ("sg", (11, 2), "ragged", None),
)
# (padded: the streaming kernel takes strides that are multiples of 32; 122 -> stride 128)
L_STREAM, L_PADDED = 128, 122
RAGGED_LENGTHS = (24, 33, 47, 64, 90, 128, 41, 56, 107, 72, 25)


def _variant_name(family, source, plan, layout, positive):
    src = "raw" if source == "raw" else f"sg{plan[0]}"
    pol = {True: "pos", False: "neg", None: "mix"}[positive]
    return f"{family}_{src}_{layout}_{pol}"


def _geometry(layout, n):
    """(lengths, per-record positive or None, gap_of, max_extra)"""
    if layout == "stream":
        return np.full(n, L_STREAM), None, None, 0
    if layout == "padded":
        return np.full(n, L_PADDED), None, None, 0
    lengths = np.array([RAGGED_LENGTHS[(r * 7 + r // 11) % len(RAGGED_LENGTHS)] for r in range(n)])
    return lengths, np.isin(np.arange(n) % 5, (1, 3)), (lambda r: (r * 3) % 5 if r else 0), 13


def _pedestal(positive, rng):
    return int(rng.integers(1000, 5000)) if positive else int(rng.integers(3000, 9000))


def _dyadic_baseline(ped, r):
    return ped + (0.0, 0.5, 0.25, -0.375, 3.0, 0.125)[r % 6]


def _make(family, variant, n, shape_of, ext, *, baseline_of=_dyadic_baseline, dyadic=True, window=None, suffix="",
          seed=0):
    """shape_of(r, L, H, wmin, gmin, rng, positive) -> (signal shape s >= 0, level, noise or None, pedestal or None)."""
    source, plan, layout, pol = variant
    rng = np.random.default_rng(seed)
    lengths, mixed, gap_of, max_extra = _geometry(layout, n)
    H = plan[0] // 2 if source == "sg" else 2
    wmin, gmin = (plan[0], H + 1) if source == "sg" else (2, 1)
    waves, peds, levels, bases, positives = [], [], [], [], []
    for r in range(n):
        L = int(lengths[r])
        positive = bool(mixed[r]) if pol is None else pol
        s, level, noise, ped = shape_of(r, L, H, wmin, gmin, rng, positive)
        if ped is None:
            ped = _pedestal(positive, rng)
        waves.append(_wave(s, ped, positive, noise))
        peds.append(ped)
        levels.append(level)
        bases.append(baseline_of(ped, r))
        positives.append(positive)
    name = _variant_name(family, source, plan, layout, pol) + suffix
    return _pack(name, family, waves, peds, levels, bases, positives, source=source, plan=plan, layout=layout,
                 ext=ext(H, int(lengths.max())), max_extra=max_extra, dyadic=dyadic, window=window, gap_of=gap_of)


# ---- family A: window clamp and asymmetric extensions -----------------------------------------------------------
def _ext_a(H, L):
    return ((0, 0), (0, 5), (5, 0), (1, 9), (H - 1, H + 1), (H + 1, H - 1), (L, L), (-3, 2))


def _shape_a(spike):
    def shape(r, L, H, wmin, gmin, rng, positive):
        s = np.zeros(L, dtype=np.int64)
        h = int(rng.integers(40, 400))
        level, noise = 0.5 * h, None
        kind = r % 8
        if kind == 0:    # a run from sample 0
            _flat(s, 0, rng.integers(1, L // 2), h)
        elif kind == 1:  # a run that ends at L
            m = int(rng.integers(1, L // 2))
            _flat(s, L - m, m, h)
        elif kind == 2:  # one-sample run
            s[int(rng.integers(H + 1, L - H - 1))] = h
            level = spike * h
        elif kind == 3:  # the whole record
            s[:] = h + (np.arange(L) * 7) % 5
        elif kind == 4:
            m = int(rng.integers(2, L // 3))
            _flat(s, rng.integers(1, L - m - 1), m, h)
            noise = rng.integers(0, 3, L)
        elif kind == 5:  # two pulses
            m = max(L // 6, 2)
            _flat(s, 1, m, h)
            _flat(s, L - m - 2, m, h + 17)
        elif kind == 6:  # one-sample run at either end of the record
            s[0 if r % 16 < 8 else L - 1] = h
            level = spike * h
        else:            # asymmetric triangle
            c = int(rng.integers(2, L - 2))
            t = np.arange(L)
            s = np.maximum(h - np.where(t < c, (c - t) * (h // 3 + 1), (t - c) * (h // 7 + 1)), 0)
            noise = rng.integers(0, 3, L)
        return s, level, noise, None
    return shape


# ---- family B: a higher neighbouring run inside the window ------------------------------------------------------
def _ext_b(H, L):
    return ((2 * H + 8, 2 * H + 8), (3, 2 * H + 8), (2 * H + 8, 3), (1, 1))


def _shape_b(r, L, H, wmin, gmin, rng, positive):
    s = np.zeros(L, dtype=np.int64)
    low = int(rng.integers(40, 200))
    high = 2 * low + int(rng.integers(1, 50))
    heights = ((low, high), (high, low), (low, high, low), (high, low, high))[r % 4]
    m = [wmin + int(rng.integers(0, 4)) for _ in heights]
    g = [gmin + int(rng.integers(0, 4)) for _ in heights[1:]]
    total = sum(m) + sum(g)
    if total + 2 > L:  # short ragged record: two narrow pulses
        heights, m, g = heights[:2], m[:2], g[:1]
        total = sum(m) + sum(g)
    a = int(rng.integers(0, max(L - total, 0) + 1))
    for k, hk in enumerate(heights):
        _flat(s, a, m[k], hk)
        a += m[k] + (g[k] if k < len(g) else 0)
    return s, 0.5 * low, None, None


# ---- family C: ties for the maximum ---------------------------------------------------------------------------
def _ext_c(H, L):
    return ((3, 3), (0, 9), (L, L))


def _shape_c(r, L, H, wmin, gmin, rng, positive):
    s = np.zeros(L, dtype=np.int64)
    h = int(rng.integers(60, 300))
    kind, q = r % 6, r // 6
    if kind == 0:    # saturated plateau of 2..40 samples (0 for the negative class, ADC_MAX for the positive one)
        m = min(2 + q % 39, L - 1)
        _flat(s, (q * 5) % (L - m + 1), m, ADC_MAX + 500)
        h = 3000
    elif kind == 1:  # twin pulses: the hit's own run and a neighbouring run hold the same maximum
        m, g = wmin + q % 6, gmin + 1 + q % 7
        _flat(s, (q * 3) % max(L - 2 * m - g, 1), m, h)
        _flat(s, (q * 3) % max(L - 2 * m - g, 1) + m + g, m, h)
    elif kind == 2:  # a wide symmetric pulse: its tied samples lie on either side of a 64-sample step of the window
        m = min(58 + q % 23, L - 2)
        _flat(s, (q * 7) % (L - m + 1), m, h)
    elif kind == 3:  # symmetric about c + 0.5: two equal central samples, swept over the 8-sample chunk boundaries
        c = q % (L - 1)
        t = np.arange(L)
        s = np.maximum(h - (h // 9 + 1) * (np.abs(2 * t - (2 * c + 1)) // 2), 0)
    elif kind == 4:  # the whole record at the rail: every sample ties, and so does the zero padding behind 0
        s[:] = ADC_MAX + 500
        h = 3000
    else:            # a record that ends, or begins, at the rail
        m = min(2 * wmin + 2 + q % 5, L - 1)
        _flat(s, L - m if q % 2 else 0, m, ADC_MAX + 500)
        h = 3000
    return s, 0.5 * h, None, None


# ---- family D: integral sign, baselines, integer guard ----------------------------------------------------------
DYADIC_BASELINES = ("ped", "ped+0.5", "ped+0.25", 0.0, -3.5, 262143.5, 262144.0, -262143.75)
# (a window's float64 sum stays exact for these at the family's pedestals and pulse heights: every term is a multiple
# of ulp(baseline) >= 2^-42 and the sum is below 2^11; the CPU file checks it row by row on the raw sets)
ARBITRARY_BASELINES = ("ped+0.3", "ped+0.7", 1e-30, "ped+1/3")


def _baseline_d(table):
    def base(ped, r):
        if r % 3 == 0 and table is ARBITRARY_BASELINES:
            return ped + 0.5  # the near-zero records of _shape_d keep a dyadic baseline
        v = table[(r // 2) % len(table)]
        if isinstance(v, str):
            return ped + {"ped": 0.0, "ped+0.5": 0.5, "ped+0.25": 0.25, "ped+0.3": 0.3, "ped+0.7": 0.7,
                          "ped+1/3": 1.0 / 3.0}[v]
        return v
    return base


def _ext_d(H, L):
    return ((2, 2), (5, 7), (0, 0))


def _shape_d(r, L, H, wmin, gmin, rng, positive):
    """Small pulses (the float64 sum of a window stays exact for any baseline of this family: see the CPU file);
    pedestal noise of -2..2 on the first half only, so that the second half holds samples equal to the pedestal."""
    s = np.zeros(L, dtype=np.int64)
    h = int(rng.integers(20, 60))
    m = wmin + int(rng.integers(0, 5))
    a = int(rng.integers(0, L - m + 1))
    _flat(s, a, m, h)
    noise = np.zeros(L, dtype=np.int64)
    noise[: L // 2] = rng.integers(-2, 3, L // 2)
    noise[s > 0] = 0
    ped = None
    if r % 3 == 0:  # near-zero samples: the filtered value is under the integer guard somewhere in the window
        ped = 2 if positive else h
        noise = np.where(noise < 0, 0, noise) if positive else noise
    return s, 0.5 * h, noise, ped


def _sign_edge(hs: HitSet, every=8, phase=5):
    """On every 8th record of a Savitzky-Golay set, move the baseline onto the float32 next to the filtered sample in
    front of (or behind) the first run, on the side that leaves that sample the smallest signal > 0 a float32 sample can
    have: k_hit_rows_flat's sign test  t <= tb  decides it with t == tb.  The threshold moves with the baseline, the
    runs stay."""
    rows, det = hit_rows_exact(hs.records, hs.filtered, hs.thresholds, 0, 0, hs.width, details=True)
    first = {}
    for k, r in enumerate(rows["record_id"]):
        first.setdefault(int(r), k)
    rec = hs.records
    for r in range(phase, len(rec), every):
        if r % 3 == 0 or r not in first:
            continue
        k = first[r]
        i = det["start"][k] - 1 if det["start"][k] > 0 else det["end"][k]
        if i >= rec["event_length"][r]:
            continue
        y = hs.filtered[rec["wave_offset"][r] + i]
        positive = rec["polarity"][r] == "positive"
        b_old, t_old = float(rec["baseline"][r]), float(hs.thresholds[r])
        b_new = float(np.nextafter(y, np.float32(-np.inf if positive else np.inf)))
        rec["baseline"][r] = b_new
        hs.thresholds[r] = (t_old + b_old) - b_new if positive else (t_old - b_old) + b_new
    return hs


# ---- family E: the shapes of the flat kernel's work lists -------------------------------------------------------
def _one_pulse(m_of, a_of, h=120):
    def shape(r, L, H, wmin, gmin, rng, positive):
        s = np.zeros(L, dtype=np.int64)
        _flat(s, a_of(r, L), m_of(r), h)
        return s, 0.5 * h, None, 5000
    return shape


CAP_L = 512
CAP_M0 = 10            # run length of an ordinary hit
CAP_START = 200
CAP_LE = 72            # window start 128: a multiple of 8, record offsets are multiples of 512
# kFlatCap chunks per batch over kFlatHits hits per wave: 32 chunks = 256 window samples per hit fill a batch exactly
CAP_RE = 8 * (FLAT_CAP // FLAT_HITS) - CAP_LE - CAP_M0


def e_cap(plan=(5, 2)):
    """Four waves of 64 one-hit records (512 samples).  The window of a run [200, 200 + m) is [128, 200 + m + CAP_RE):
    m = 10 gives 32 chunks.  Wave 0: hit 20 has m = 2 (31 chunks), the wave totals kFlatCap - 1.  Wave 1: kFlatCap
    exactly.  Wave 2: hit 20 has m = 18 (33 chunks), total kFlatCap + 1, the wave's last hit straddles the batch
    boundary.  Wave 3: every m = 74 (40 chunks), hit 51 straddles it in its middle."""
    def m_of(r):
        wave, k = r // FLAT_HITS, r % FLAT_HITS
        if wave == 3:
            return CAP_M0 + 64
        if k == 20:
            return (CAP_M0 - 8, CAP_M0, CAP_M0 + 8)[wave]
        return CAP_M0
    return _make_uniform("E", plan, CAP_L, 4 * FLAT_HITS, _one_pulse(m_of, lambda r, L: CAP_START), ((CAP_LE, CAP_RE),),
                         "_cap")


def _make_uniform(family, plan, L, n, shape_of, ext, suffix, positive=False, baseline_of=_dyadic_baseline, ped=None):
    rng = np.random.default_rng(1)
    H = plan[0] // 2
    waves, peds, levels, bases = [], [], [], []
    for r in range(n):
        s, level, noise, p = shape_of(r, L, H, plan[0], H + 1, rng, positive)
        waves.append(_wave(s, p, positive, noise))
        peds.append(p)
        levels.append(level)
        bases.append(baseline_of(p, r))
    layout = "stream" if L % 32 == 0 else "padded"
    return _pack(f"{family}_sg{plan[0]}{suffix}", family, waves, peds, levels, bases, positive, source="sg", plan=plan,
                 layout=layout, ext=ext)


E_L = 64


def e_short(plan=(11, 2)):
    """64-sample records (the shortest the streaming kernel takes): narrow pulses at the head and the tail (the window
    lies inside an edge zone: no interior chunk) next to pulses in the middle; (64, 64): every window is the whole
    record."""
    def a_of(r, L):
        return (0, 28, L - 2, 17)[r % 4]
    return _make_uniform("E", plan, E_L, 4 * FLAT_HITS + 1, _one_pulse(lambda r: (2, plan[0], 2, plan[0] + 2)[r % 4], a_of),
                         ((0, 0), (E_L, E_L)), "_short")


def e_count(n_hits, plan=(5, 2)):
    """n_hits 64-sample records, one hit each; (64, 64) puts every window over the whole record: 2H edge samples per hit,
    more than 64 per wave."""
    return _make_uniform("E", plan, E_L, n_hits, _one_pulse(lambda r: plan[0] + r % 3, lambda r, L: 8 + r % 37),
                         ((2, 2), (E_L, E_L)), f"_count{n_hits}")


def e_ragged(plan=(5, 2)):
    """Lengths W - 1, W, W + 1, 2W interleaved (records shorter than the window are flagged for the literal kernel and
    share a wave with the others) among longer ones; record offsets at every value mod 8; the first record's hit starts
    at pool sample 0 and the last record's hit ends at the pool's last sample."""
    W = plan[0]
    cycle = (2 * W, W - 1, W, W + 1, 2 * W, 41, 56, 67)
    n = 64 * 6
    rng = np.random.default_rng(2)
    waves, peds, levels, bases, positives = [], [], [], [], []
    for r in range(n):
        L = cycle[r % len(cycle)]
        s = np.zeros(L, dtype=np.int64)
        h = 100 + r % 50
        m = min(W + r % 3, L)
        a = 0 if r == 0 else (L - m if r == n - 1 else int(rng.integers(0, L - m + 1)))
        _flat(s, a, m, h)
        positive = r % 3 == 1
        ped = 4000 + r
        waves.append(_wave(s, ped, positive))
        peds.append(ped)
        levels.append(0.5 * h)
        bases.append(_dyadic_baseline(ped, r))
        positives.append(positive)
    return _pack(f"E_sg{W}_ragged", "E", waves, peds, levels, bases, positives, source="sg", plan=plan, layout="ragged",
                 ext=((0, 0), (3, 3), (1, 9)))


def e_litcap(plan=(5, 2)):
    """More than kLitCap hits under the integer guard in one pass: 64-sample records around a pedestal of 6 with two dips
    to 0 (a filtered dip holds exact zeros), two hits each."""
    n = (LIT_CAP + 4 * FLAT_HITS + 3) // 2 + 1

    def shape(r, L, H, wmin, gmin, rng, positive):
        s = np.zeros(L, dtype=np.int64)
        _flat(s, 6 + r % 11, plan[0] + 1 + r % 4, 6)
        _flat(s, 38 + r % 13, plan[0] + 1 + r % 3, 6)
        return s, 3.0, None, 6
    return _make_uniform("E", plan, E_L, n, shape, ((2, 2),), "_litcap")


# ---- the sets -------------------------------------------------------------------------------------------------
N_UNIFORM, N_RAGGED = 1024, 768


def _n(variant):
    return N_RAGGED if variant[2] == "ragged" else N_UNIFORM


@functools.cache
def family_sets(family):
    out = []
    for i, v in enumerate(VARIANTS):
        spike = _spike_level(v[0], v[1])
        if family == "A":
            out.append(_make("A", v, _n(v), _shape_a(spike), _ext_a, seed=100 + i))
        elif family == "B":
            out.append(_make("B", v, _n(v), _shape_b, _ext_b, seed=200 + i))
        elif family == "C":
            out.append(_make("C", v, _n(v), _shape_c, _ext_c, seed=300 + i))
        elif family == "D":
            hs = _make("D", v, _n(v), _shape_d, _ext_d, baseline_of=_baseline_d(DYADIC_BASELINES), seed=400 + i)
            out.append(_sign_edge(hs) if v[0] == "sg" else hs)
            # (ragged: positive polarity only.  With the other one a padding sample's signal is the baseline itself, and
            # two of them already take the window's sum past the 53 bits that keep it exact)
            va = v if v[2] != "ragged" else (v[0], v[1], v[2], True)
            out.append(_make("D", va, _n(v), _shape_d, _ext_d, baseline_of=_baseline_d(ARBITRARY_BASELINES), dyadic=False,
                             suffix="_arb", seed=450 + i))
    if family == "E":
        out = [e_count(2 * FLAT_HITS - 1), e_count(2 * FLAT_HITS), e_count(2 * FLAT_HITS + 1), e_cap(), e_short(),
               e_ragged(), e_ragged((11, 2)), e_litcap()]
    return tuple(out)


@functools.cache
def fused_sets():
    """Uniform sets whose baselines are what the fused baseline pass computes: the mean of the first 32 / 64 samples
    (dyadic; bitmap and general routes), and of the first 40, the one window the streaming kernel fuses, with the window's
    samples adjusted until that mean is an integer."""
    return (_make("B", VARIANTS[2], N_UNIFORM, _shape_b, _ext_b, window=(0, 32), suffix="_fused32", seed=501),
            _make("C", VARIANTS[1], N_UNIFORM, _shape_c, _ext_c, window=(0, 64), suffix="_fused64", seed=502),
            _make("D", VARIANTS[1], N_UNIFORM, _shape_d, _ext_d, window=(0, 40), suffix="_fused40", seed=503),
            _make("A", VARIANTS[2], N_UNIFORM, _shape_a(_spike_level("sg", (11, 2))), _ext_a, window=(0, 40),
                  suffix="_fused40", seed=504))


FAMILIES = ("A", "B", "C", "D", "E")


@functools.cache
def all_sets():
    return tuple(hs for f in FAMILIES for hs in family_sets(f)) + fused_sets()


@functools.cache
def by_name(name):
    return {hs.name: hs for hs in all_sets()}[name]


def names(family=None, **where):
    return [hs.name for hs in all_sets()
            if (family is None or hs.family == family) and all(getattr(hs, k) == v for k, v in where.items())]


# ---- comparison ---------------------------------------------------------------------------------------------------
EXACT_FIELDS = tuple(n for n in THRESHOLD_HIT_DTYPE.names if n != "integral")


def assert_rows(got, want, *, exact_integral, what):
    """Every field but `integral` exactly (height as float32 bits); `integral` exactly, or within one float32 ulp of the
    reference.  -> number of integrals that are not bit-identical."""
    assert got.dtype == want.dtype and len(got) == len(want), f"{what}: {len(got)} rows, want {len(want)}"
    for name in EXACT_FIELDS:
        g, w = got[name], want[name]
        bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32)) if g.dtype == np.float32 else np.flatnonzero(g != w)
        assert len(bad) == 0, (f"{what}: field {name}: {len(bad)} of {len(want)} rows differ, first row {bad[0]}: "
                               f"got {got[bad[0]]}, want {want[bad[0]]}")
    g, w = got["integral"], want["integral"]
    differ = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
    if exact_integral:
        assert len(differ) == 0, (f"{what}: integral: {len(differ)} of {len(want)} rows differ, first row {differ[0]}: "
                                  f"got {g[differ[0]]!r}, want {w[differ[0]]!r}")
    else:
        far = np.flatnonzero(np.abs(g.astype(np.float64) - w.astype(np.float64)) > np.spacing(np.abs(w)).astype(np.float64))
        assert len(far) == 0, f"{what}: integral: {len(far)} rows beyond one float32 ulp, first row {far[0]}"
    return len(differ)
