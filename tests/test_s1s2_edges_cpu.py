"""The S1/S2 edge run and its range sets (tests/s1s2_edges_util.py) without a GPU: the run holds every case the GPU
test relies on, the oracle and the host classifier give the recorded reference labels on every set, and the one
comparison of the GPU test notices each of a list of subtly wrong chains (numpy models, never run on a device)."""

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import s1s2_edges_util as E
from waveformanalysis_amd.dtypes import S1_S2_CLASSIFIER_DTYPE
from waveformanalysis_amd.plugins import s1_s2 as P


# ---- 1. the run -----------------------------------------------------------------------------------------------------
def test_ragged_layout_and_columns():
    rec, pool, _kw = E.edge_run("ragged")
    L, off = rec["event_length"].astype(np.int64), rec["wave_offset"].astype(np.int64)
    assert 650 <= len(rec) <= 800 and L.min() == 0 and L.max() <= 200 and len(pool) < 200_000
    assert {0, 1, 49, 50, 51} <= set(L.tolist())
    gaps = off - np.concatenate(([0], (off + L)[:-1]))
    assert set(gaps.tolist()) == set(range(1, 8)) and off[-1] + L[-1] == len(pool)
    assert np.array_equal(rec["record_id"], np.arange(len(rec)))
    assert np.all(np.diff(rec["timestamp"]) > 0) and 2**61 < rec["timestamp"].min() and rec["timestamp"].max() < 2**62
    assert {-32768, 32767} <= set(rec["board"].tolist()) and 32767 in rec["channel"] and -1 in rec["channel"]
    assert len(set(rec["dt"].tolist())) == 3
    again = E.edge_run.__wrapped__("ragged")
    assert again[0].tobytes() == rec.tobytes() and again[1].tobytes() == pool.tobytes()


def test_uniform_layout():
    rec, pool, _kw = E.edge_run("uniform")
    assert np.all(rec["event_length"] == E.UNIFORM_L) and len(pool) == len(rec) * E.UNIFORM_L
    assert np.array_equal(rec["wave_offset"], np.arange(len(rec)) * E.UNIFORM_L)
    hits, widths, _f = E.oracle_tables("uniform")
    keep = E.kept_mask("uniform")
    assert len(hits) > 129 and 0 < len(widths) < len(hits) and not keep[0] and not keep[-1]


def test_ragged_run_holds_every_case():
    rec, pool, _kw = E.edge_run("ragged")
    hits, widths, feats = E.oracle_tables("ragged")
    keep = E.kept_mask("ragged")
    assert len(hits) > 1025 and keep.sum() == len(widths) and len(feats) == len(rec)
    # block sizes: record prefixes with exactly these peak counts, one peak per record around them
    prefix = E.prefix_lengths("ragged")
    per_record = np.bincount(hits["record_id"], minlength=len(rec))
    for n in E.PEAK_COUNTS:
        assert per_record[:prefix[n]].sum() == n
    for lo, hi in ((prefix[127] - 2, prefix[129] + 2), (prefix[1024] - 2, prefix[1025] + 2)):
        assert np.all(per_record[lo:hi] == 1), per_record[lo:hi]
    assert prefix[1] == 1
    # drop patterns
    assert not keep[0] and not keep[-1]
    run = best = 0
    for k in keep:
        run = 0 if k else run + 1
        best = max(best, run)
    assert best >= 130
    lo, hi = E.dropped_stretch("ragged")
    sub_hits, sub_widths, _f = E.oracle_tables("ragged", lo, hi)
    assert len(sub_hits) >= 130 and len(sub_widths) == 0
    kept_per_record = np.bincount(widths["record_id"], minlength=len(rec))
    assert (kept_per_record == 2).sum() >= 20
    # a kept row behind peak 1024 (the second scan tile) and in every block of 128
    assert keep[1024:].any() and all(keep[b:b + 128].any() or b == 128 for b in range(0, 1024, 128))
    # distinct values
    rows = E.oracle_rows("ragged", {})
    for col in ("total_width", "total_width_samples"):
        assert len(np.unique(widths[col])) >= 8
    for col in ("height", "area"):
        assert len(np.unique(rows[col])) >= 8
    _h, w0, _f = E.oracle_tables("ragged", interpolation=False)
    assert np.unique(w0["total_width"], return_counts=True)[1].max() >= 2
    assert len(w0) == len(widths) and w0.tobytes() != widths.tobytes()


def test_sample_equal_to_the_baseline_mean_is_dropped_and_its_twin_kept():
    rec, pool, _kw = E.edge_run("ragged")
    hits, widths, _f = E.oracle_tables("ragged")
    zero, one = E.twin_records("ragged")
    for r, top in ((zero, 0.0), (one, 1.0)):
        mine = hits[hits["record_id"] == r]
        assert len(mine) == 1
        off, L = int(rec["wave_offset"][r]), int(rec["event_length"][r])
        wave = pool[off:off + L]
        assert float(wave[int(mine["position"][0])]) - float(np.mean(wave[:50])) == top  # strict >: 0 is dropped
        assert (widths["record_id"] == r).sum() == int(top > 0)
    kept = widths[widths["record_id"] == one]
    assert kept["peak_height"][0] == 1.0


# ---- 2. the sets and the recorded reference ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return E.golden()


@pytest.fixture(scope="module")
def oracle_labelled(golden):
    """{(i, name): the oracle's rows} for every recorded set, computed once and left unchanged."""
    out = {}
    for i in (0, 1):
        _h, widths, feats = E.oracle_tables("ragged", interpolation=bool(i))
        for name, kw in golden[f"sets_{i}"].items():
            rows = O.s1_s2_classify(widths, feats, **kw)
            rows.setflags(write=False)
            out[i, name] = rows
    return out


def test_fixture_holds_the_runs_tables_and_sets(golden):
    for i in (0, 1):
        _h, widths, feats = E.oracle_tables("ragged", interpolation=bool(i))
        assert golden[f"widths_{i}"].tobytes() == widths.tobytes() and golden["features"].tobytes() == feats.tobytes()
        sets = E.bound_sets(E.oracle_rows("ragged", {}, interpolation=bool(i)))
        assert E.same_sets(sets, golden[f"sets_{i}"]) and len(sets) == 6 * 2 * 11 * 2 + 4
        assert sorted(golden[f"labels_{i}"]) == sorted(sets)
    assert golden["strict_text"] == E.STRICT_TEXT


def test_oracle_and_host_classifier_give_the_reference_labels(golden, oracle_labelled):
    seen = set()
    for (i, name), rows in oracle_labelled.items():
        widths, feats = golden[f"widths_{i}"], golden["features"]
        want = golden[f"labels_{i}"][name]
        assert np.array_equal(rows["label"], want), (i, name)
        host = P.classify(widths, feats, **golden[f"sets_{i}"][name])
        E.assert_chain_equal(host, rows, f"plugins.s1_s2.classify, {name}")
        plain = O.s1_s2_classify(widths, feats)
        for col in S1_S2_CLASSIFIER_DTYPE.names[1:]:
            assert rows[col].tobytes() == plain[col].tobytes(), (name, col)
        seen |= set(want.tolist())
    assert seen == {0, 1, 2}
    for classify in (O.s1_s2_classify, P.classify):
        with pytest.raises(ValueError) as err:
            classify(golden["widths_1"], golden["features"], strict=True, s1_width_range=(None, None))
        assert str(err.value) == golden["strict_text"]


def test_guards_on_the_oracle_labels(golden, oracle_labelled):
    for i in (0, 1):
        lab = lambda name: oracle_labelled[i, name]["label"]  # noqa: E731
        rows = oracle_labelled[i, "conflict/unknown"]
        for slot in E.SLOTS:
            cls = 1 if slot.startswith("s1") else 2
            for unit in E.UNITS:
                sets = {name: kw for name, kw in golden[f"sets_{i}"].items() if name.startswith(f"{slot}/{unit}/")}
                assert len(sets) == 22
                col = rows[E._column(slot, unit if "width" in slot else "ns")]
                m = sets[f"{slot}/{unit}/ge_m/alone"][slot][0]
                # what the same class asks beside the slot's own range (a width range in samples: area / height slots)
                beside = np.ones(len(rows), bool)
                if unit == "samples" and "width" not in slot:
                    beside = rows["width_samples"] <= sets[f"{slot}/{unit}/ge_m/alone"][f"{slot[:2]}_width_range"][1]
                at_m = (col == np.float32(m)) & beside
                assert at_m.any() and col.min() < m < col.max() and float(np.float32(m)) == m
                # configuration 2: where the other class matches
                q, (lo, hi) = (rows["area"], E.WIDE_AREA) if "height" in slot else (rows["height"], E.WIDE_HEIGHT)
                other = (q >= lo) & (q <= hi)
                for cfg in ("alone", "both"):
                    key = lambda r: f"{slot}/{unit}/{r}/{cfg}"  # noqa: E731
                    # inclusive bounds: the rows at m are in; one float32 or one float64 step further they are out
                    for r in ("ge_m", "le_m", "eq_m"):
                        assert np.all(lab(key(r))[at_m] == (np.where(other[at_m], 0, cls) if cfg == "both" else cls))
                    for r in ("ge_next32", "le_prev32", "ge_next64", "le_prev64", "empty"):
                        assert np.all(lab(key(r))[at_m] != cls)
                    for a, b in (("ge_m", "ge_next32"), ("ge_m", "ge_next64"), ("le_m", "le_prev32"), ("le_m", "le_prev64")):
                        assert np.flatnonzero(lab(key(a)) != lab(key(b))).tolist() == np.flatnonzero(at_m).tolist()
                    assert np.array_equal(lab(key("eq_m")) == cls, at_m & ~(other & (cfg == "both")))
                    assert not np.any(lab(key("empty")) == cls)
                assert set(lab(f"{slot}/{unit}/ge_m/alone").tolist()) == {0, cls}
                assert set(lab(f"{slot}/{unit}/ge_m/both").tolist()) == {0, 1, 2}
                assert set(lab(f"{slot}/{unit}/empty/both").tolist()) == {0, 3 - cls}
        alone = [lab(f"{slot}/ns/ge_m/alone") for slot in E.SLOTS]
        for a in range(6):
            for b in range(a + 1, 6):
                assert not np.array_equal(alone[a], alone[b]), (E.SLOTS[a], E.SLOTS[b])
        # the conflict sets: the rows at m match both classes
        kw = golden[f"sets_{i}"]["conflict/unknown"]
        at_m = rows["width_ns"] == np.float32(kw["s1_width_range"][1])
        assert at_m.sum() >= (2 if i == 0 else 1) and kw["s1_width_range"][1] == kw["s2_width_range"][0]
        for policy, label in zip(E.POLICIES, (0, 1, 2, 0)):
            got = lab(f"conflict/{policy}")
            assert np.all(got[at_m] == label) and set(got[~at_m].tolist()) == {1, 2}
        # the samples twins: another label vector than the ns set, and another one than the same numbers read as ns
        _h, widths, feats = E.oracle_tables("ragged", interpolation=bool(i))
        for slot in E.SLOTS:
            for r in ("ge_m", "le_m", "eq_m"):
                name = f"{slot}/samples/{r}/alone"
                if "width" in slot:
                    assert not np.array_equal(lab(name), lab(name.replace("samples", "ns")))
                as_ns = O.s1_s2_classify(widths, feats, **{**golden[f"sets_{i}"][name], "width_unit": "ns"})
                assert not np.array_equal(lab(name), as_ns["label"])


# ---- 3. sensitivity: the comparison fails for subtly wrong chains ------------------------------------------------------
MUTANTS = ("exclusive_lower", "exclusive_upper", "float32_compare", "area_height_swapped", "s1_s2_swapped",
           "bound_bits_swapped", "nan_bound_out_of_range", "both_match_is_s1", "record_id_base_not_added",
           "shifted_behind_row_1024", "last_kept_row_lost", "width_unit_ignored")
BASES = (0, 1, 2**40 + 3)


def model_chain(hits, keep, widths, feats, class_kw, record_id_base=0, mutant=None):
    """The device chain in numpy, from the arguments DeviceSession.peak_chain packs (twelve float64 bounds, one bit
    per bound set): labels per kept peak, rows into per-peak slots, kept slots compacted in peak order."""
    kw = dict(class_kw)
    unit, policy = kw.pop("width_unit", "ns"), kw.pop("conflict_policy", "unknown")
    if mutant == "width_unit_ignored":
        unit = "ns"
    ranges = P.class_ranges(**kw)
    bounds, mask = np.zeros(12), 0
    for k, r in enumerate(ranges):
        for j in (0, 1):
            if r is not None and r[j] is not None:
                bounds[2 * k + j] = r[j]
                mask |= 1 << (2 * k + j)
    if mutant == "s1_s2_swapped":
        bounds = np.concatenate([bounds[6:], bounds[:6]])
        mask = (mask >> 6) | ((mask & 0x3F) << 6)
    if mutant == "bound_bits_swapped":
        mask = ((mask & 0x555) << 1) | ((mask & 0xAAA) >> 1)
    rid = widths["record_id"].astype(np.int64)
    h32, a32 = feats["height"][rid], feats["area"][rid]
    if mutant == "area_height_swapped":
        h32, a32 = a32, h32
    w32 = widths["total_width_samples"] if unit == "samples" else widths["total_width"]
    f = np.float32 if mutant == "float32_compare" else np.float64

    def in_range(k, v32):
        b = (mask >> (2 * k)) & 3
        v = v32.astype(f)
        ok = np.ones(len(v), bool)
        if b == 0:
            return ok
        ok &= ~np.isnan(v)
        lo, hi = f(bounds[2 * k]), f(bounds[2 * k + 1])
        with np.errstate(invalid="ignore"):
            if b & 1:
                ok &= ~(v <= lo if mutant == "exclusive_lower" else v < lo)
                if mutant == "nan_bound_out_of_range" and np.isnan(lo):
                    ok[:] = False
            if b & 2:
                ok &= ~(v >= hi if mutant == "exclusive_upper" else v > hi)
                if mutant == "nan_bound_out_of_range" and np.isnan(hi):
                    ok[:] = False
        return ok

    s1 = in_range(0, w32) & in_range(1, a32) & in_range(2, h32) if mask & 0x03F else np.zeros(len(rid), bool)
    s2 = in_range(3, w32) & in_range(4, a32) & in_range(5, h32) if mask & 0xFC0 else np.zeros(len(rid), bool)
    both = {"prefer_s1": 1, "prefer_s2": 2}.get(policy, 0)
    if mutant == "both_match_is_s1":
        both = 1
    kept = np.zeros(len(rid), dtype=S1_S2_CLASSIFIER_DTYPE)
    kept["label"] = np.where(s1 & s2, both, np.where(s1, 1, np.where(s2, 2, 0)))
    kept["width_ns"], kept["width_samples"] = widths["total_width"], widths["total_width_samples"]
    kept["height"], kept["area"] = feats["height"][rid], feats["area"][rid]
    for col in ("timestamp", "board", "channel"):
        kept[col] = widths[col]
    kept["record_id"] = rid + (0 if mutant == "record_id_base_not_added" else record_id_base)
    kept["peak_position"] = widths["peak_position"]
    # slots and compaction
    slots = np.zeros(len(hits), dtype=S1_S2_CLASSIFIER_DTYPE)
    slots[keep] = kept
    start = np.cumsum(keep) - keep
    if mutant == "shifted_behind_row_1024":
        start[1024:] += 1
    n = int(keep.sum())
    out = np.zeros(n - (mutant == "last_kept_row_lost"), dtype=S1_S2_CLASSIFIER_DTYPE)
    for i in np.flatnonzero(keep):
        if start[i] < len(out):
            out[start[i]] = slots[i]
    return out


def _survives(golden, oracle_labelled, mutant):
    """True when no comparison of the GPU test's kind fails for this chain."""
    for i in (0, 1):
        hits, widths, feats = E.oracle_tables("ragged", interpolation=bool(i))
        keep = E.kept_mask("ragged")
        for name, kw in golden[f"sets_{i}"].items():
            for base in BASES if name == "conflict/unknown" else (0,):
                want = oracle_labelled[i, name]
                if base:
                    want = want.copy()
                    want["record_id"] += base
                try:
                    E.assert_chain_equal(model_chain(hits, keep, widths, feats, kw, base, mutant), want, name)
                except AssertionError:
                    return False
    return True


def test_the_unmutated_model_passes_every_comparison(golden, oracle_labelled):
    assert _survives(golden, oracle_labelled, None)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_comparison_fails_for_a_wrong_chain(golden, oracle_labelled, mutant):
    assert not _survives(golden, oracle_labelled, mutant), mutant


def test_assert_chain_equal_names_the_field():
    rows = E.oracle_rows("ragged", {}).copy()
    E.assert_chain_equal(rows.copy(), rows, "same")
    for col in S1_S2_CLASSIFIER_DTYPE.names:
        bad = rows.copy()
        bad[col][7] = rows[col][7] - 1 if rows[col][7] > 0 else rows[col][7] + 1
        with pytest.raises(AssertionError, match=f"field '{col}' differs in 1 rows, first at row 7"):
            E.assert_chain_equal(bad, rows, "one field")
    with pytest.raises(AssertionError, match="rows, expected"):
        E.assert_chain_equal(rows[:-1].copy(), rows, "short")
    with pytest.raises(AssertionError):
        E.assert_chain_equal(rows.astype(np.dtype(rows.dtype.descr, align=True)), rows, "aligned dtype")
