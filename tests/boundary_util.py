"""Records whose hit mask is decided exactly at the threshold boundary (reference: hit_finder.py:329-366).

The reference masks  signal >= thr  with  signal = +-(baseline - y)  in float64, y the raw uint16 sample or the float32
filtered one.  A set built here gives every record one target sample and puts the record's baseline or threshold
exactly on the boundary of that sample ("on"), one float64 step to the side where the sample no longer hits ("off"),
or one step to the other side ("beyond").  Records cycle through the three variants, through waveform shapes that
put the runs on tile edges, record edges and span edges, and through regimes of  v = +-b - thr  (|v| < 1, v near
65 535, exact and inexact subtraction, |thr| > |b|, thr = 0).  A few records carry thresholds or baselines with no
boundary at all (NaN, +-inf, negative).

`check_flips` proves on the CPU, with the oracle, that each target sample is inside a run in the "on" and "beyond"
variants and outside every run in the "off" variant: a set whose boundary is not where it claims fails there.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from oracle import wfa_oracle as O
from waveformanalysis_amd.dtypes import RECORDS_DTYPE

ON, OFF, BEYOND, SPECIAL = 0, 1, 2, -1
KINDS = ("peak", "flat_top", "tile_31", "tile_63", "head", "tail", "all", "alternate")
REGIMES = ("mid", "low", "high", "zero")  # "zero": threshold-driven records with b == y at the target (thr = 0)
BASELINE_WINDOW = 40


@dataclasses.dataclass
class BoundarySet:
    records: np.ndarray        # RECORDS_DTYPE, record_id == index
    pool: np.ndarray           # uint16 wave_pool
    filtered: np.ndarray | None  # float32 pool the decision reads (SG output or the f32 source); None: raw samples
    thresholds: np.ndarray     # float64, one per record (the variant the record carries)
    target: np.ndarray         # sample index of the boundary sample, -1 for special records
    variant: np.ndarray        # ON / OFF / BEYOND / SPECIAL
    alt: dict                  # variant -> (baselines, thresholds) with every record at that variant
    source: str                # "raw", "f32", "sg"
    plan: tuple[int, int]
    mode: str                  # "baseline" or "threshold"
    fused_baseline: bool

    @property
    def positive(self) -> np.ndarray:
        return O.positive_mask_from_polarity(self.records)

    def y(self) -> np.ndarray:
        return self.pool.astype(np.float64) if self.filtered is None else self.filtered.astype(np.float64)

    def with_variant(self, k: int) -> tuple[np.ndarray, np.ndarray]:
        rec = self.records.copy()
        rec["baseline"], thr = self.alt[k]
        return rec, thr.copy()

    def oracle(self, records=None, thresholds=None, left_extension=2, right_extension=2) -> np.ndarray:
        rec = self.records if records is None else records
        thr = self.thresholds if thresholds is None else thresholds
        src = self.pool if self.filtered is None else self.filtered
        return O.threshold_hits(rec, src, thresholds=thr, left_extension=left_extension,
                                right_extension=right_extension)

    def channel_config(self) -> dict:
        """The per-record thresholds as the plugins' channel_config (every record has its own board:channel)."""
        rec = self.records
        return {f"{int(b)}:{int(c)}": {"threshold": float(t)}
                for b, c, t in zip(rec["board"], rec["channel"], self.thresholds)}


def _shape(kind, L, A, rng):
    """Signal shape s >= 0 (raw units, integer) of one record and the rank of its target sample (1 = largest)."""
    s = np.zeros(L, dtype=np.int64)
    t = np.arange(L)
    if kind == "peak":
        c = int(rng.integers(3, L - 3))
        s = np.maximum(A - 3 * A // 8 * np.abs(t - c), 0)
        return s, 1
    if kind == "flat_top":
        c, w = int(rng.integers(2, L - 8)), int(rng.integers(2, 5))
        s = np.maximum(A - A // 3 * np.maximum(np.maximum(c - t, t - (c + w - 1)), 0), 0)
        return s, 1  # first of the equal maxima
    if kind in ("tile_31", "tile_63"):
        c = 31 if kind == "tile_31" else 63
        c = min(c, L - 3)
        s = np.maximum(A - A // 6 * np.abs(2 * t - (2 * c + 1)) // 2, 0)  # symmetric around c + 0.5
        return s, 4
    if kind == "head":
        return np.maximum(A - A // 5 * t, 0), 3
    if kind == "tail":
        return np.maximum(A - A // 5 * (L - 1 - t), 0), 3
    if kind == "all":
        return A // 2 + (t % 7), L  # the smallest sample: on the boundary every sample hits
    if kind == "alternate":
        c = int(rng.integers(0, L - 12))
        s[c:c + 12:2] = A
        return s, 1
    raise ValueError(kind)


def _key(x: float) -> int:
    """Order-preserving integer of a float64 (consecutive floats -> consecutive integers)."""
    i = int(np.float64(x).view(np.int64))
    return i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF)


def _unkey(k: int) -> float:
    return float(np.int64(k if k >= 0 else (-k) | -0x8000000000000000).view(np.float64))


def _solve_baseline(y, thr, positive):
    """Smallest b (largest for positive) with  fl(+-(b - y)) >= thr:  (on, off, beyond) baselines.

    Bisection over the float64 values between a baseline that misses and one that hits (near b = 0 the float64 spacing
    of b is far finer than that of b - y, so many neighbouring baselines give the same signal)."""
    sig = lambda b: (y - b) if positive else (b - y)  # noqa: E731
    b = (y - thr) if positive else (y + thr)
    span = 1.0 + abs(b) * 1e-6
    hit, miss = (b - span, b + span) if positive else (b + span, b - span)
    assert sig(hit) >= thr and not sig(miss) >= thr, (y, thr)
    kh, km = _key(hit), _key(miss)
    while abs(kh - km) > 1:
        mid = (kh + km) // 2
        if sig(_unkey(mid)) >= thr:
            kh = mid
        else:
            km = mid
    step = 1 if kh > km else -1  # from the miss side to the hit side
    return _unkey(kh), _unkey(km), _unkey(kh + step)


def make_set(n, L, *, source="sg", plan=(11, 2), mode="baseline", positive=False, threshold=10.3, seed=0,
             fused_baseline=False, lengths=None, specials=True) -> BoundarySet:
    """n records of L samples (or the given ragged `lengths`), back to back.

    mode "baseline": one global `threshold`, the boundary sits in each record's baseline.
    mode "threshold": each record keeps its natural baseline (the mean of its first 40 samples, which is what the fused
    baseline window computes) and gets its own threshold; board/channel are unique per record.
    """
    rng = np.random.default_rng(seed)
    if lengths is None:
        lengths = np.full(n, L, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    n = len(lengths)
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    pool = np.zeros(int(lengths.sum()), dtype=np.uint16)
    ranks = np.zeros(n, dtype=np.int64)
    regimes = []
    for r in range(n):
        Lr = int(lengths[r])
        kind = KINDS[(r // 3) % len(KINDS)]
        if r % 64 == 63 or r % 51 == 50:
            kind = "tail"  # a run that ends the last record of a span (64 records, and 51 under span_records)
        if Lr < 80 and kind == "tile_63":
            kind = "tile_31"
        regime = REGIMES[(r // (3 * len(KINDS))) % (len(REGIMES) if mode == "threshold" else 3)]
        A = int(rng.integers(12, 400))
        s, rank = _shape(kind, Lr, A, rng)
        noise = rng.integers(0, 3, Lr) if regime != "low" else 0
        if regime == "low":
            # negative: the pulse is clipped at 0 over its top half, so y is 0 there and the filter dips below it
            ped = 0 if positive else int(s.max()) // 2
        elif regime == "high":
            ped = 65535 - int(s.max()) - 3 if positive else 65532
        else:
            ped = int(rng.integers(3000, 9000))
        w = ped + s + noise if positive else ped - s + noise
        pool[offs[r]:offs[r] + Lr] = np.clip(w, 0, 65535).astype(np.uint16)
        ranks[r] = min(rank, Lr)
        regimes.append(regime)

    rec = np.zeros(n, dtype=RECORDS_DTYPE)
    rec["wave_offset"], rec["event_length"] = offs, lengths
    rec["timestamp"] = 10**12 + np.cumsum(lengths * 4000)
    rec["dt"] = np.array([1, 2, 4])[np.arange(n) % 3]
    rec["record_id"] = np.arange(n)
    rec["board"], rec["channel"] = np.arange(n) // 1000, np.arange(n) % 1000
    rec["polarity"] = "positive" if positive else np.where(np.arange(n) % 2 == 0, "unknown", "negative")
    # the natural baseline: mean of the first 40 samples (tot / 40, the fused baseline window's value)
    rec["baseline"] = [pool[o:o + min(int(m), BASELINE_WINDOW)].sum(dtype=np.int64) / float(BASELINE_WINDOW)
                       for o, m in zip(offs, lengths)]

    if source == "raw":
        filtered = None
    else:
        W, P = plan
        filtered = O.filter_wave_pool(rec, pool, sg_window_size=W, sg_poly_order=P)
        if source == "f32":  # a materialised float32 pool that is not integer-valued on unfiltered samples either
            filtered = (filtered + np.float32(0.375)).astype(np.float32)
    y_pool = pool.astype(np.float64) if filtered is None else filtered.astype(np.float64)

    target = np.full(n, -1, dtype=np.int64)
    variant = np.full(n, SPECIAL, dtype=np.int64)
    bl = {k: rec["baseline"].astype(np.float64).copy() for k in (ON, OFF, BEYOND)}
    th = {k: np.full(n, float(threshold)) for k in (ON, OFF, BEYOND)}
    special_thr = (0.0, np.inf, -np.inf, np.nan, -7.5)
    for r in range(n):
        o, Lr = int(offs[r]), int(lengths[r])
        y = y_pool[o:o + Lr]
        b0 = float(rec["baseline"][r])
        if specials and r % 37 == 36:
            if mode == "threshold":
                t = special_thr[(r // 37) % len(special_thr)]
                for k in th:
                    th[k][r] = t
            elif not fused_baseline:
                for k in bl:
                    bl[k][r] = np.nan
            continue
        sig_order = np.argsort(-y if positive else y, kind="stable")  # largest signal first, first index on ties
        t = int(sig_order[ranks[r] - 1])
        target[r] = t
        variant[r] = r % 3
        yt = float(y[t])
        if mode == "baseline":
            bl[ON][r], bl[OFF][r], bl[BEYOND][r] = _solve_baseline(yt, float(threshold), positive)
        else:
            if regimes[r] == "zero" and not fused_baseline:
                b0 = yt  # fl(b - y) == 0: the thresholds are 0 and the smallest subnormals either side
                for k in bl:
                    bl[k][r] = b0
            on = (yt - b0) if positive else (b0 - yt)
            th[ON][r], th[OFF][r], th[BEYOND][r] = on, np.nextafter(on, np.inf), np.nextafter(on, -np.inf)
    rec["baseline"] = [bl[int(max(v, 0))][r] for r, v in enumerate(variant)]
    thresholds = np.array([th[int(max(v, 0))][r] for r, v in enumerate(variant)])
    for r in np.flatnonzero(variant == SPECIAL):  # the specials carry their value in every variant
        rec["baseline"][r] = bl[ON][r]
        thresholds[r] = th[ON][r]
    return BoundarySet(rec, pool, filtered, thresholds, target, variant,
                       {k: (bl[k], th[k]) for k in (ON, OFF, BEYOND)}, source, tuple(plan), mode, fused_baseline)


def covered(hits: np.ndarray, n: int, target: np.ndarray) -> np.ndarray:
    """Per record: is its target sample inside one of the runs the rows describe (start/end from rise/fall time)?"""
    out = np.zeros(n, dtype=bool)
    dt = hits["dt"].astype(np.int64)
    pos = hits["position"].astype(np.int64)
    start = pos - np.rint(hits["rise_time"]).astype(np.int64) // dt
    end = pos + np.rint(hits["fall_time"]).astype(np.int64) // dt + 1
    rid = hits["record_id"].astype(np.int64)
    t = target[rid]
    inside = (t >= start) & (t < end)
    out[rid[inside]] = True
    return out


def check_flips(bs: BoundarySet) -> dict:
    """Every target: inside a run for ON and BEYOND, outside every run for OFF (the oracle decides).  Returns the
    oracle's rows (no extensions) of each all-records variant."""
    rows = {}
    want = {ON: True, OFF: False, BEYOND: True}
    has = bs.target >= 0
    assert has.sum() > 0
    for k, expect in want.items():
        rec, thr = bs.with_variant(k)
        rows[k] = bs.oracle(rec, thr, left_extension=0, right_extension=0)  # pos inside its own run
        cov = covered(rows[k], len(rec), bs.target)
        bad = np.flatnonzero(has & (cov != expect))
        assert len(bad) == 0, f"variant {k}: records {bad[:10].tolist()} are not on the boundary"
    return rows


def regime_counts(bs: BoundarySet) -> dict:
    """How many boundary records fall in each regime of v = +-b - thr (the generator's coverage, for the self-check)."""
    rec = bs.records
    b = rec["baseline"].astype(np.float64)
    thr = bs.thresholds
    pos = bs.positive
    v = np.where(pos, -(b + thr), b - thr)
    has = bs.target >= 0
    with np.errstate(invalid="ignore"):
        exact = np.where(pos, (-v - b) == thr, (b - v) == thr) & (np.abs(b) >= np.abs(thr))
        return {
            "small_v": int(np.sum(has & (np.abs(v) < 1))),
            "v_near_65535": int(np.sum(has & (np.abs(v) > 65000))),
            "exact": int(np.sum(has & exact & (np.abs(v) >= 1))),
            "inexact": int(np.sum(has & ~exact)),
            "thr_above_b": int(np.sum(has & (np.abs(thr) > np.abs(b)))),
            "thr_zero": int(np.sum(has & (thr == 0))),
        }
