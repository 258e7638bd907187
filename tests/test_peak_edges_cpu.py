"""The inputs of tests/test_hip_peak_edges.py, checked without a GPU: every named rule is really hit, the oracle agrees
with scipy.signal.find_peaks itself (numpy.argsort pinned to the stable kind), every embedding reproduces its detection
signal bit for bit, and the oracle's rows have a second derivation straight from scipy's output."""

import numpy as np
import pytest
from scipy.signal import find_peaks

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests import peak_edges_util as U

MIN_HITS = 20
LAYOUTS = U.layouts()


def _all_signals(fam):
    for lay in LAYOUTS:
        for deriv in (False, True):
            for x in U.signals_for(fam, lay, deriv):
                yield lay, deriv, x


@pytest.fixture(scope="module")
def coverage():
    """{rule: hits over the whole generated set}, and per family whether its predicate held on every long signal."""
    total = dict.fromkeys(U.RULES, 0)
    small = {2: 0, 3: 0, 4: 0}
    predicate_fails = []
    for fam in U.FAMILIES:
        for lay, deriv, x in _all_signals(fam):
            if len(x) in small and not fam.float_values:
                small[len(x)] += 1
            hit_own = False
            for opt in fam.options:
                got = U.analyse(x, **opt)
                for k, v in got.items():
                    total[k] += v
                hit_own |= any(got[r] > 0 for r in fam.rules)
            if len(x) >= 60 and not hit_own:
                predicate_fails.append((fam.name, lay.name, deriv))
    return total, small, predicate_fails


def test_every_builder_predicate_holds(coverage):
    assert coverage[2] == []


@pytest.mark.parametrize("rule", U.RULES)
def test_rule_is_hit(coverage, rule):
    assert coverage[0][rule] >= MIN_HITS, (rule, coverage[0][rule])


def test_tiny_records_present(coverage):
    assert all(v >= MIN_HITS for v in coverage[1].values()), coverage[1]


@pytest.mark.parametrize("fam", U.FAMILIES, ids=lambda f: f.name)
def test_oracle_equals_scipy(fam):
    """O.find_peaks_staged == scipy.signal.find_peaks with the stable argsort on every signal and option set; on
    tie-free signals == plain scipy too."""
    n_free = 0
    for _lay, _deriv, x in _all_signals(fam):
        x = np.asarray(x, dtype=np.float64)
        for opt in fam.options:
            try:
                peaks, l_ips, r_ips = O.find_peaks_staged(x, opt["height"], opt["threshold"], opt["distance"],
                                                          opt["prominence"], opt["width"])
            except ValueError:
                assert len(x) == 0
                continue
            want, props = U.scipy_find_peaks_stable(x, **opt)
            np.testing.assert_array_equal(peaks, want)
            np.testing.assert_array_equal(l_ips, props["left_ips"])
            np.testing.assert_array_equal(r_ips, props["right_ips"])
            if U.candidates_tie_free(x, opt["height"], opt["threshold"], opt["distance"]):
                n_free += 1
                plain, pprops = find_peaks(x, **opt)
                np.testing.assert_array_equal(peaks, plain)
                np.testing.assert_array_equal(l_ips, pprops["left_ips"])
                np.testing.assert_array_equal(r_ips, pprops["right_ips"])
    assert n_free > 0 or fam.name in ("ties", "tied_noise")


def test_plain_scipy_depends_on_the_platform_where_values_tie():
    """Documents (does not assert) how often plain scipy differs from the pinned rule on this host."""
    rng = np.random.default_rng(11)
    differs = agrees_stable = 0
    for _ in range(600):
        x = rng.integers(0, 4, 200).astype(np.float64)
        kw = dict(height=1.0, distance=int(rng.integers(3, 9)))
        want = O.find_peaks_staged(x, 1.0, None, kw["distance"], 0.0, 0)[0]
        agrees_stable += int(np.array_equal(U.scipy_find_peaks_stable(x, **kw, prominence=0.0, width=0)[0], want))
        differs += int(not np.array_equal(find_peaks(x, **kw, prominence=0.0, width=0)[0], want))
    assert agrees_stable == 600, f"stable-patched scipy agrees in {agrees_stable}/600; plain scipy differs in {differs}/600"


@pytest.mark.parametrize("with_nine", [False, True])
def test_slot_boundary_inputs(with_nine):
    """The two uploads of the slot-boundary test: 7 or 8 candidates per record, and exactly one record of 4096 with 9."""
    for n in (36, 37, 39, 40):
        counts = np.array([U.count_candidates(x) for x in U.slot_signals(n, 4096, with_nine)])
        assert counts.min() == 7 and (counts == 7).sum() > 1000 and (counts == 8).sum() > 1000
        assert (counts > 8).sum() == int(with_nine) and counts.max() == 8 + int(with_nine)


def _forms(fam, lay, deriv):
    """(name, dets, heights_on, meta, oracle call, streaming, ext name) of every form the layout and family allow."""
    sig = U.signals_for(fam, lay, deriv)
    out = []
    for pol in ("negative", "positive", "unknown"):
        rec, pool = U.embed_records(sig, lay, deriv, pol, fam.float_values)
        pools = [pool] if fam.float_values else [pool, U.f32_twin(pool)]
        for p in pools:
            dets = U.det_records(rec, p, deriv)
            on = [-O._normalized_signal_f32(r, p[int(r["wave_offset"]):int(r["wave_offset"]) + int(r["event_length"])],
                                            r["baseline"]).astype(np.float64) for r in rec]
            out.append((f"records {pol} {p.dtype}", dets, on, rec,
                        lambda kw, rec=rec, p=p: O.find_peak_hits(rec, p, use_derivative=deriv, **kw), False))
        if lay.mixed_polarity:
            break
    for wdt in ((np.float32,) if fam.float_values else (np.int16, np.float32)):
        st = U.embed_dense(sig, lay, deriv, wdt, fam.float_values)
        on = [row["wave"][:int(row["event_length"])] for row in st]
        out.append((f"dense {np.dtype(wdt)}", U.det_dense(st, deriv), on, st,
                    lambda kw, st=st: O.find_peak_hits_dense(st, use_derivative=deriv, **kw), False))
        if lay.uniform:
            on64 = [np.asarray(row["wave"], dtype=np.float64) for row in st]
            out.append((f"stream {np.dtype(wdt)}", U.det_dense(st, deriv, streaming=True), on64, st,
                        lambda kw, st=st: O.signal_peaks_rows(st, st, use_derivative=deriv, **kw), True))
    return sig, out


@pytest.mark.parametrize("fam", U.FAMILIES, ids=lambda f: f.name)
@pytest.mark.parametrize("lay", [LAYOUTS[0], LAYOUTS[3], LAYOUTS[6], LAYOUTS[7]], ids=lambda l: l.name)
def test_embeddings_and_expected_rows(fam, lay):
    """Each form's own detection signal IS x (bit for bit), and the oracle's rows equal rows assembled from
    scipy_find_peaks_stable plus the plugin's row lines."""
    for deriv in (False, True):
        sig, forms = _forms(fam, lay, deriv)
        for name, dets, on, meta, oracle, streaming in forms:
            float_inexact = fam.float_values and deriv  # running sums of float32(0.1 k) round: x is what the form gives
            for x, d in zip(sig, dets):
                assert d.dtype == np.float64 and len(d) == len(x)
                if not float_inexact:
                    np.testing.assert_array_equal(d, np.asarray(x, dtype=np.float64), err_msg=name)
            for opt in fam.options[:2]:
                for method, ext in (("minmax", 1), ("diff", 4)):
                    kw = dict(opt, height_method=method)
                    kw["minmax_window_expand" if streaming else "height_window_extension"] = ext
                    want = U.rows_from_scipy(dets, on, meta, opt, method, ext, streaming=streaming)
                    G.assert_struct_equal(oracle(kw), want, what=f"{fam.name} {lay.name} {name} {kw}")


# ------------------------------------------------------------------------------------------------
# waveform_width
# ------------------------------------------------------------------------------------------------
def ww_literal(hits, data, rise_low=0.1, rise_high=0.9, fall_high=0.9, fall_low=0.1, sampling_rate=0.5,
               interpolation=True):
    """waveform_width.py:139-374 as a literal per-hit loop in numpy scalars -> (rows, kept mask, {edge: count})."""
    edges = dict.fromkeys(U.WW_EDGES, 0)

    def crossing(seg, level, rising, tag):
        if len(seg) == 0:
            return None
        idx = np.where(seg >= level)[0] if rising else np.where(seg <= level)[0]
        if len(idx) == 0:
            return None
        k = idx[0]
        edges[tag + "_level_on_sample"] += int(k > 0 and seg[k] == level)
        if rising and k == 0:
            edges["rise_crossing_at_0"] += 1
        if interpolation and k > 0:
            left, right = seg[k - 1], seg[k]
            if abs(right - left) < 1e-10:
                edges["flat_crossing"] += 1
                return float(k)
            return float(k - 1) + (level - left) / (right - left)
        return float(k)

    rows, kept = [], np.zeros(len(hits), dtype=bool)
    ids = data["record_id"]
    for n, h in enumerate(hits):
        rid, pos = int(h["record_id"]), h["position"]
        match = np.where(ids == rid)[0]
        if len(match) == 0:
            continue
        edges["duplicate_record_id"] += int(len(match) > 1)
        wave = data[match[0]]["wave"]
        corrected = wave - np.mean(wave[:50])
        if pos >= len(corrected):
            edges["position_past_end"] += 1
            continue
        top = corrected[pos]
        if top <= 0:
            edges["top_zero" if top == 0 else "top_negative"] += 1
            continue
        edges["position_0"] += int(pos == 0)
        edges["position_last"] += int(pos == len(corrected) - 1)
        r_lo = crossing(corrected[:pos], top * rise_low, True, "rise")
        r_hi = crossing(corrected[:pos], top * rise_high, True, "rise")
        f_hi = crossing(corrected[pos:], top * fall_high, False, "fall")
        f_lo = crossing(corrected[pos:], top * fall_low, False, "fall")
        edges["fall_high_absent_low_found"] += int(f_hi is None and f_lo is not None)
        rise_s = rise_t = fall_s = fall_t = tot_s = tot_t = 0.0
        if r_lo is not None and r_hi is not None:
            rise_s = r_hi - r_lo
            rise_t = rise_s / sampling_rate
        if f_hi is not None and f_lo is not None:
            f_hi += pos
            f_lo += pos
            fall_s = f_lo - f_hi
            fall_t = fall_s / sampling_rate
        if r_lo is not None and f_lo is not None:
            tot_s = f_lo - r_lo
            tot_t = tot_s / sampling_rate
        kept[n] = True
        rows.append((rise_t, fall_t, tot_t, rise_s, fall_s, tot_s, int(pos), top, int(h["timestamp"]), int(h["board"]),
                     int(h["channel"]), rid))
    out = np.zeros(len(rows), dtype=O.WAVEFORM_WIDTH_DTYPE)
    for k, row in enumerate(rows):
        for name, v in zip(O.WAVEFORM_WIDTH_DTYPE.names, row):
            out[name][k] = v  # numpy scalar -> float32 field, as the reference's result_array[i] = ... does
    return out, kept, edges


def ww_cases():
    for L in U.WW_LENGTHS:
        for kind in ("int16", "float32", "tiny"):
            for seed in (0, 1):
                yield L, kind, seed


def test_waveform_width_oracle_against_literal_loop_and_edge_coverage():
    total = dict.fromkeys(U.WW_EDGES, 0)
    for L, kind, seed in ww_cases():
        st, hits = U.ww_rows(L, kind, seed)
        for opt in U.WW_OPTIONS:
            want, _kept, edges = ww_literal(hits, st, **opt)
            G.assert_struct_equal(O.waveform_width(hits, st, **opt), want, what=f"L {L} {kind} {opt}")
            for k, v in edges.items():
                total[k] += v
    assert all(v >= MIN_HITS for v in total.values()), total
