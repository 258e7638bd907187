"""Inputs of the S1/S2 peak chain edge tests: a synthetic run whose peak table crosses the block sizes of the chain's
kernels and whose first, last and a long stretch of peaks are dropped by the width stage; range sets whose bounds sit
on values the run produces (and one float32 / float64 step beside them); the one comparison the tests use.

Everything is generated from fixed seeds; nothing is read from disk except the recorded reference labels
(tests/golden/s1s2_edges.npz, made by tests/golden/make_s1s2_edges_golden.py)."""

from __future__ import annotations

import functools
import json
import os

import numpy as np

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests import width_records_util as W
from waveformanalysis_amd.dtypes import RECORDS_DTYPE, S1_S2_CLASSIFIER_DTYPE

FIXTURE = os.path.join(G.GOLDEN, "s1s2_edges.npz")
HIT = dict(height=45.0, prominence=1.0, width=1, distance=2)  # hit options of both layouts
PEAK_COUNTS = (1, 127, 128, 129, 1024, 1025)  # k_peak_chain's block is 128 peaks, the scan tile over `keep` 1024
SLOTS = tuple(f"{c}_{q}_range" for c in ("s1", "s2") for q in ("width", "area", "height"))
# configuration 2: the one range of the other class, on a column the slot does not cut on
WIDE_HEIGHT, WIDE_AREA = (1000.0, 2000.0), (10000.0, 30000.0)
UNITS = ("ns", "samples")
STRICT_TEXT = "No S1/S2 criteria configured; set ranges or disable strict."
UNIFORM_L = 128
SHORT_LENGTHS = (0, 1, 49, 50, 51, 2, 7, 33)


# ---- the run ------------------------------------------------------------------------------------------------------
def _pulse(amp: int, rise: int, fall: int) -> np.ndarray:
    """`rise` samples up to amp, `fall` samples back to 0 (integers); negative amp: a dip of the same shape mirrored in
    time, so that its recovery is the steep edge the detector finds."""
    up = np.rint(abs(amp) * np.arange(1, rise + 1) / rise)
    down = np.rint(abs(amp) * (fall - np.arange(1, fall + 1)) / fall)
    p = np.concatenate([up, down]).astype(np.int64)
    return p if amp > 0 else -p[::-1]


def _plan(layout: str):
    """Per record: (length, [pulse kinds]).  Kinds: "+" kept pulse, "-" dip (found, then dropped), "0" step whose peak
    sample equals the baseline mean (dropped), "1" its twin one ADC count higher (kept)."""
    rng = np.random.default_rng(20261021 + (layout == "uniform"))
    plan = []

    def add(kinds, n=1):
        for _ in range(n):
            k = list(kinds(rng)) if callable(kinds) else list(kinds)
            need = 60 + 36 * len(k)
            L = UNIFORM_L if layout == "uniform" else int(rng.integers(max(need, 100), 201))
            plan.append((L, k))

    def mixed(rng):
        return [["+"], ["+", "+"], ["-"], ["+", "-"], ["-", "+"], ["-", "-"]][int(rng.integers(6))]

    if layout == "uniform":
        add("-")
        add(mixed, 60)
        add("0"), add("1")
        add("-", 3)
        add("++", 20)
        add(mixed, 60)
        add("-")
        return plan
    add("-")                      # the first peak of the table: dropped
    add(mixed, 70)
    add("+", 16), add("-", 8), add("+", 8), add("-", 8)   # one peak per record around 127 .. 129
    add("0"), add("1")
    add("-", 140)                 # a run of dropped peaks longer than a block
    add("++", 24)                 # two kept rows share one feature row
    while sum(len(k) for _L, k in plan) < 1006:
        add(mixed)
    add("+", 12), add("-", 12), add("+", 6), add("-", 6)  # one peak per record around 1024 .. 1025
    add(mixed, 12)
    add("-")                      # the last peak of the table: dropped
    for k, L in enumerate(SHORT_LENGTHS):  # records too short to hold a pulse, spread over the mixed stretches
        plan.insert(5 + 9 * k, (L, []))
    return plan


@functools.lru_cache(maxsize=None)
def edge_run(layout: str):
    """(records, wave_pool, hit options) of the "ragged" or the "uniform" edge run; arrays are read-only."""
    assert layout in ("ragged", "uniform")
    plan = _plan(layout)
    rng = np.random.default_rng([7, len(plan)])
    R = len(plan)
    rec = np.zeros(R, dtype=RECORDS_DTYPE)
    k = np.arange(R)
    rec["record_id"] = k
    rec["timestamp"] = 2**62 - 10**12 + k * 10**6 + (k % 7)
    rec["board"] = np.asarray([0, 1, 32767, 3, -32768])[k % 5]
    rec["channel"] = np.asarray([0, 32767, 5, -1, 63, 2, 1])[k % 7]
    rec["dt"] = np.asarray([2, 1, 4])[k % 3]
    rec["polarity"] = "positive"
    rec["baseline_upstream"] = np.nan
    chunks, at = [], 0
    for r, (L, kinds) in enumerate(plan):
        gap = 0 if layout == "uniform" else 1 + (3 * r + 2) % 7
        chunks.append(rng.integers(0, 16384, gap).astype(np.uint16))  # whatever no record covers
        at += gap
        base = 8000 + int(rng.integers(0, 400))
        wave = np.full(L, base, dtype=np.int64)
        room = (L - 56) // max(len(kinds), 1)
        for j, kind in enumerate(kinds):
            start = 56 + j * room + int(rng.integers(0, 3))
            amp = int(rng.integers(600, 2400))
            if kind in "01":
                # a step to a flat top (wider than half the filter window: the filtered derivative peaks on the step,
                # at the sample in front of it), the same shape for both twins
                p = np.concatenate([np.full(8, 1500), _pulse(1500, 1, 12)[1:]])
                wave[start - 1] += int(kind)
            else:
                fall = int(rng.integers(6, min(24, room - 10)))
                p = _pulse(amp if kind == "+" else -amp, int(rng.integers(4, 8)), fall)
            assert start + len(p) <= L, (layout, r, L, kinds)
            wave[start:start + len(p)] += p
        rec["wave_offset"][r], rec["event_length"][r] = at, L
        rec["baseline"][r] = base
        chunks.append(wave.astype(np.uint16))
        at += L
    pool = np.concatenate(chunks)
    assert len(pool) < 200_000
    rec.setflags(write=False)
    pool.setflags(write=False)
    return rec, pool, HIT


def twin_records(layout: str):
    """(index of the record whose peak sample equals its baseline mean, index of its twin one count higher)."""
    kinds = [k for _L, k in _plan(layout)]
    return kinds.index(["0"]), kinds.index(["1"])


# ---- the oracle chain (as s1s2_chain_util.oracle_tables) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def filtered_pool(layout: str):
    rec, pool, _kw = edge_run(layout)
    out = O.filter_wave_pool(rec, pool)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_hits(layout: str):
    rec, _pool, hit_kw = edge_run(layout)
    hits = O.find_peak_hits(rec, filtered_pool(layout), **hit_kw)
    hits.setflags(write=False)
    return hits


def subset(layout: str, lo: int, hi: int):
    """Records [lo, hi) of the run as a table of their own (record_id from 0), on the run's pool."""
    rec = edge_run(layout)[0][lo:hi].copy()
    rec["record_id"] = np.arange(len(rec))
    return rec


@functools.lru_cache(maxsize=None)
def oracle_tables(layout: str, lo: int = 0, hi: int | None = None, interpolation: bool = True,
                  width_filtered: bool = False, features_filtered: bool = False, height_range=(40, 90),
                  area_range=(0, None)):
    """(hit table, width rows, feature rows) of the oracle chain on records [lo, hi) of a run."""
    rec, pool, _kw = edge_run(layout)
    hi = len(rec) if hi is None else hi
    hits = oracle_hits(layout)
    hits = hits[(hits["record_id"] >= lo) & (hits["record_id"] < hi)].copy()
    hits["record_id"] -= lo
    sub = subset(layout, lo, hi)
    filt = filtered_pool(layout)
    widths = W.oracle_widths(hits, sub, filt if width_filtered else pool, interpolation=interpolation)
    feats = O.basic_features(sub, filt if features_filtered else pool, height_range=height_range, area_range=area_range)
    for a in (hits, widths, feats):
        a.setflags(write=False)
    return hits, widths, feats


def oracle_rows(layout: str, class_kw: dict, **table_kw) -> np.ndarray:
    """O.s1_s2_classify(**class_kw) on the tables of oracle_tables(layout, **table_kw)."""
    _h, widths, feats = oracle_tables(layout, **table_kw)
    return O.s1_s2_classify(widths, feats, **class_kw)


def kept_mask(layout: str) -> np.ndarray:
    """Per peak of the run's hit table: does the width stage keep it (widths on the raw pool)?"""
    hits, widths, _f = oracle_tables(layout)
    key = lambda t, pos: set(zip(t["record_id"].tolist(), t[pos].tolist()))  # noqa: E731
    kept = key(widths, "peak_position")
    return np.asarray([(r, p) in kept for r, p in zip(hits["record_id"].tolist(), hits["position"].tolist())])


def prefix_lengths(layout: str) -> dict:
    """{peak count: number of leading records that hold exactly that many peaks} for PEAK_COUNTS."""
    hits = oracle_hits(layout)
    per_record = np.bincount(hits["record_id"], minlength=len(edge_run(layout)[0]))
    total = np.cumsum(per_record)
    out = {}
    for n in PEAK_COUNTS:
        at = np.flatnonzero(total == n)
        assert at.size, (n, "no record prefix with this peak count")
        out[n] = int(at[0]) + 1
    return out


def dropped_stretch(layout: str) -> tuple:
    """(lo, hi): the longest range of records with at least one peak in total whose peaks are all dropped."""
    hits = oracle_hits(layout)
    R = len(edge_run(layout)[0])
    kept_in = np.bincount(hits["record_id"][kept_mask(layout)], minlength=R) > 0
    best, lo = (0, 0), 0
    for r in range(R + 1):
        if r == R or kept_in[r]:
            if r - lo > best[1] - best[0]:
                best = (lo, r)
            lo = r + 1
    return best


# ---- the range sets -------------------------------------------------------------------------------------------------
def _column(slot: str, unit: str) -> str:
    return {"width": "width_samples" if unit == "samples" else "width_ns", "area": "area", "height": "height"}[
        slot.split("_")[1]]


def middle_value(rows: np.ndarray, column: str, rank: int = 0) -> float:
    """A value of the column that is neither its smallest nor its largest: the one attained by the most rows (rank 0),
    the next most (rank 1), ...; ties go to the smaller value.  The float64 of the stored float32."""
    values, counts = np.unique(rows[column], return_counts=True)
    assert len(values) >= 3 + rank, column
    values, counts = values[1:-1], counts[1:-1]
    return float(values[np.argsort(-counts, kind="stable")[rank]])


def median_value(rows: np.ndarray, column: str) -> float:
    """The value of the row in the middle of the sorted column."""
    return float(np.sort(rows[column])[len(rows) // 2])


def _ranges(m: float) -> list:
    f32_up = float(np.nextafter(np.float32(m), np.float32(np.inf)))
    f32_dn = float(np.nextafter(np.float32(m), np.float32(-np.inf)))
    return [
        ("ge_m", (m, None)), ("le_m", (None, m)), ("eq_m", (m, m)),
        ("ge_next32", (f32_up, None)), ("le_prev32", (None, f32_dn)),
        ("ge_next64", (float(np.nextafter(m, np.inf)), None)), ("le_prev64", (None, float(np.nextafter(m, -np.inf)))),
        ("empty", (f32_up, f32_dn)),
        ("inf", (float("-inf"), float("inf"))), ("nan_nan", (float("nan"), float("nan"))), ("nan_lo", (float("nan"), None)),
    ]


def other_class(slot: str) -> dict:
    cls = "s2" if slot.startswith("s1") else "s1"
    return {f"{cls}_area_range": WIDE_AREA} if "height" in slot else {f"{cls}_height_range": WIDE_HEIGHT}


def slot_sets(rows: np.ndarray, slot: str, unit: str = "ns") -> dict:
    """{name: class options} of one slot: every range of the table, alone (configuration 1) and beside one range of
    the other class (configuration 2).  unit "samples": a width slot takes m from total_width_samples; an area or
    height slot keeps its ranges and gets a width range of its own class in samples beside them, so that the unit
    decides there too."""
    is_width = "width" in slot
    # (total_width is total_width_samples / 0.5, the same rows share a value in both: the samples sets take another one)
    m = middle_value(rows, _column(slot, unit if is_width else "ns"), rank=int(is_width and unit == "samples"))
    extra = {"width_unit": "samples"} if unit == "samples" else {}
    if unit == "samples" and not is_width:
        at_m = rows[_column(slot, "ns")] == np.float32(m)  # (the widest row at m: every row at m stays in)
        extra[f"{slot[:2]}_width_range"] = (None, float(rows["width_samples"][at_m].max()))
    out = {}
    for name, r in _ranges(m):
        base = {slot: r, **extra}
        out[f"{slot}/{unit}/{name}/alone"] = base
        out[f"{slot}/{unit}/{name}/both"] = {**base, **other_class(slot)}
    return out


POLICIES = ("unknown", "prefer_s1", "prefer_s2", "prefer_both")  # (the last one is none of the reference's three)


def conflict_sets(rows: np.ndarray) -> dict:
    """s1 width (lo, m), s2 width (m, hi): the rows at m match both classes."""
    m = middle_value(rows, "width_ns")
    lo, hi = float(rows["width_ns"].min()) - 1.0, float(rows["width_ns"].max()) + 1.0
    return {f"conflict/{p}": dict(s1_width_range=(lo, m), s2_width_range=(m, hi), conflict_policy=p) for p in POLICIES}


def bound_sets(rows: np.ndarray) -> dict:
    """Every named set: six slots in both units and the conflict sets.  `rows`: the oracle's kept
    rows (any labels)."""
    out = {}
    for slot in SLOTS:
        for unit in UNITS:
            out.update(slot_sets(rows, slot, unit))
    out.update(conflict_sets(rows))
    return out


def to_json(sets: dict) -> bytes:
    """The sets as JSON (tuples as lists; NaN / Infinity as python's json writes them)."""
    return json.dumps(sets, sort_keys=True).encode()


def from_json(blob: bytes) -> dict:
    return {name: {k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()}
            for name, kw in json.loads(bytes(blob).decode()).items()}


def same_sets(a: dict, b: dict) -> bool:
    return to_json(a) == to_json(b)


_golden: dict = {}


def golden() -> dict:
    """The recorded reference: tables `widths_i` / `features` (i = 1 with, 0 without interpolation), `sets_i` and
    `labels_i[name]`, `strict_text`."""
    if not _golden:
        z = np.load(FIXTURE, allow_pickle=False)
        _golden["features"] = z["features"]
        _golden["strict_text"] = bytes(z["strict_text"]).decode()
        for i in (0, 1):
            _golden[f"widths_{i}"] = z[f"widths_{i}"]
            sets = from_json(z[f"sets_{i}"])
            _golden[f"sets_{i}"] = sets
            labels = z[f"labels_{i}"]
            assert labels.shape == (len(sets), len(z[f"widths_{i}"])) and labels.dtype == np.int8
            _golden[f"labels_{i}"] = dict(zip(sorted(sets), labels))
    return _golden


# ---- the comparison -------------------------------------------------------------------------------------------------
def assert_chain_equal(got: np.ndarray, want_rows: np.ndarray, what: str) -> None:
    """dtype, length and bytes; a mismatch names the first differing field and row."""
    assert isinstance(got, np.ndarray) and got.dtype == S1_S2_CLASSIFIER_DTYPE, (what, getattr(got, "dtype", type(got)))
    assert want_rows.dtype == S1_S2_CLASSIFIER_DTYPE, what
    assert len(got) == len(want_rows), f"{what}: {len(got)} rows, expected {len(want_rows)}"
    if got.tobytes() == want_rows.tobytes():
        return
    for name in S1_S2_CLASSIFIER_DTYPE.names:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want_rows[name])
        bad = np.flatnonzero(a.view(f"u{a.itemsize}") != b.view(f"u{b.itemsize}"))
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{what}: field {name!r} differs in {bad.size} rows, first at row {i}: "
                                 f"got {a[i]!r}, expected {b[i]!r}")
    raise AssertionError(f"{what}: bytes differ outside the fields")
