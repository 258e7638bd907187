"""find_peaks route and waveform_width on the GPU at scipy's tie, plateau and base edges.

Inputs: tests/peak_edges_util.py (tests/test_peak_edges_cpu.py proves that they hit every named rule and that the
oracle equals scipy.signal.find_peaks itself on them).  Bar, as everywhere in this stage: rows equal the oracle's
exactly, every candidate route gives the same bytes, and the profile shows that the intended kernel ran.

Thinned against the full cross product (DESIGN.md "Pinned find_peaks rules"): every family runs on every layout, source
and branch with both derivative settings and all of its own option sets; (height_method, window extension) takes
(minmax, 1) and (diff, 4) everywhere, (minmax, 4) and (minmax, 0) on the family's first option set; the alternative routes
are compared on the first (method, extension) of each option set; the records polarity rotates over the layouts except on
the first aligned and the ragged layout, which take all three.
"""

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests import peak_edges_util as U
from waveformanalysis_amd import _lib, dense
from waveformanalysis_amd.device import DeviceSession
from waveformanalysis_amd.dtypes import BASIC_FEATURES_DTYPE
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import (
    HipHitFinderPlugin,
    HipS1S2ClassifierPlugin,
    HipSignalPeaksStreamPlugin,
    HipWaveformWidthPlugin,
)
from waveformanalysis_amd.plugins.waveform_width import first_row_of_record_id

pytestmark = pytest.mark.gpu

LAYOUTS = U.layouts()
POLARITIES = ("negative", "positive", "unknown")
FILL = "k_find_peaks<fill candidates>"


@pytest.fixture(scope="module")
def sess():
    s = DeviceSession(0)
    yield s
    s.close()


def _run_routes(sess, src, dense_rows, kw, lay, all_routes, what):
    """One find_peaks pass with the profile on: the intended kernels ran; with all_routes, every other candidate route
    that applies to the layout gives the same bytes (and is the kernel it claims to be)."""
    sess.profile(True)
    got = sess.find_peaks(src, dense_rows=dense_rows, **kw)
    names = set(sess.profile_report())
    first = "k_find_peaks_hot" if lay.aligned else "k_find_peaks_slots"
    assert first in names, (what, names)
    assert ("k_peak_select" in names) == (kw["distance"] > 2), (what, names)
    assert ("k_peak_compact" in names) != (FILL in names), (what, names)
    if all_routes:
        others = [("no_span", "k_find_peaks_slots"), ("no_peak_slots", "k_find_peaks<count candidates>")]
        if lay.aligned:
            others.insert(0, ("no_peak_hot", "k_find_peaks_staged"))
        for option, kernel in others:
            sess.set_option(option, True)
            try:
                sess.profile(True)
                other = sess.find_peaks(src, dense_rows=dense_rows, **kw)
                assert kernel in set(sess.profile_report()), (what, option)
            finally:
                sess.set_option(option, False)
            assert other.tobytes() == got.tobytes(), (what, option)
    sess.profile(False)
    return got


def _grid(fam):
    """(option set index, find_peaks keywords without the extension, extension, compare the routes)"""
    for i, opt in enumerate(fam.options):
        yield i, dict(opt, height_method="minmax"), 1, True
        yield i, dict(opt, height_method="diff"), 4, False
        if i == 0:
            yield i, dict(opt, height_method="minmax"), 4, False
            if opt["width"] >= 2:  # width >= 2: round(right_ip) > round(left_ip), no zero-size window
                yield i, dict(opt, height_method="minmax"), 0, False


def _check(sess, src, dense_rows, lay, fam, deriv, want_of, what, cache):
    n_rows = 0
    for i, kw, ext, routes in _grid(fam):
        key = (i, kw["height_method"], ext)
        if key not in cache:
            cache[key] = want_of(kw, ext)
        want = cache[key]
        got = _run_routes(sess, src, dense_rows, dict(kw, use_derivative=deriv, height_window_extension=ext), lay, routes, (what, key))
        G.assert_struct_equal(got, want, what=f"{what} {key}")
        n_rows += len(want)
    return n_rows


@pytest.mark.parametrize("fam", U.FAMILIES, ids=lambda f: f.name)
@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: l.name)
def test_find_peaks_edges(sess, fam, lay):
    li = LAYOUTS.index(lay)
    n_rows = 0
    for deriv in (False, True):
        sig = U.signals_for(fam, lay, deriv)
        # --- records branch -------------------------------------------------------------------------------
        pols = POLARITIES if li in (0, 6) else (POLARITIES[(li + int(deriv)) % 3],)
        for pol in pols:
            rec, pool = U.embed_records(sig, lay, deriv, pol, fam.float_values)
            cache = {}
            want_of = lambda kw, ext: O.find_peak_hits(rec, pool, use_derivative=deriv, height_window_extension=ext, **kw)  # noqa: E731
            for src, p in ((_lib.SRC_F32, pool),) if fam.float_values else ((_lib.SRC_RAW, pool), (_lib.SRC_F32, U.f32_twin(pool))):
                assert np.array_equal(p.astype(np.float64), pool.astype(np.float64))  # the twin holds the same numbers
                sess.upload_pool(p)
                sess.upload_records(rec, 0.0)
                n_rows += _check(sess, src, 0, lay, fam, deriv, lambda kw, ext: want_of(kw, ext), f"{fam.name} {lay.name} records {pol} src {src} deriv {deriv}",
                                 cache)
        # --- dense rows (dense_rows=1) and the streaming detector's float64 rows (dense_rows=2) --------------------
        for wdt in ((np.float32,) if fam.float_values else (np.int16, np.float32)):
            st = U.embed_dense(sig, lay, deriv, wdt, fam.float_values)
            pool, src, L = dense.dense_pool(st)
            sess.upload_pool(pool)
            rec = dense.dense_records(st, L, keep_record_id=True, truncate_to_event_length=True)
            rec["dt"] = st["dt"]
            sess.upload_records(rec, 0.0)
            n_rows += _check(sess, src, 1, lay, fam, deriv,
                             lambda kw, ext: O.find_peak_hits_dense(st, use_derivative=deriv, height_window_extension=ext, **kw),
                             f"{fam.name} {lay.name} dense {np.dtype(wdt)} deriv {deriv}", {})
            if not lay.uniform:
                continue
            n_rows += _check(sess, src, 2, lay, fam, deriv,
                             lambda kw, ext: O.signal_peaks_rows(st, st, use_derivative=deriv, minmax_window_expand=ext, **kw),
                             f"{fam.name} {lay.name} stream {np.dtype(wdt)} deriv {deriv}", {})
            if fam.name == "width":  # a float `width`: the exact value and its neighbours one ulp either side
                for w in U.STREAM_WIDTHS:
                    kw = dict(fam.options[1], width=w, height_method="diff", use_derivative=deriv)
                    got = sess.find_peaks(src, dense_rows=2, height_window_extension=2, **kw)
                    G.assert_struct_equal(got, O.signal_peaks_rows(st, st, minmax_window_expand=2, **kw), what=f"stream width {w!r}")
    assert n_rows > 0


@pytest.mark.parametrize("L", [40, 37])
def test_slot_boundary(sess, L):
    """7 and 8 candidates per record fit the per-record slots (k_peak_compact); one record with 9 among 4096 sends the
    whole launch to the fill walk.  Same rows either way, and as the two-walk route gives them."""
    lay = U.uniform_layout(L, 4096)
    kw = dict(height=1.0, threshold=None, distance=1, prominence=0.0, width=0, height_method="diff", height_window_extension=1)
    for deriv in (False, True):
        for with_nine, route, other in ((False, "k_peak_compact", FILL), (True, FILL, "k_peak_compact")):
            sig = U.slot_signals(L - int(deriv), 4096, with_nine)
            counts = np.array([U.count_candidates(x) for x in sig])
            assert counts.max() == (9 if with_nine else 8) and (counts == 9).sum() == int(with_nine) and counts.min() == 7
            rec, pool = U.embed_records(sig, lay, deriv, "negative")
            want = O.find_peak_hits(rec, pool, use_derivative=deriv, **kw)
            assert len(want) == counts.sum()
            for src, p in ((_lib.SRC_RAW, pool), (_lib.SRC_F32, U.f32_twin(pool))):
                sess.upload_pool(p)
                sess.upload_records(rec, 0.0)
                sess.profile(True)
                got = sess.find_peaks(src, use_derivative=deriv, **kw)
                names = set(sess.profile_report())
                assert route in names and other not in names, names
                assert ("k_find_peaks_hot" if lay.aligned else "k_find_peaks_slots") in names, names
                G.assert_struct_equal(got, want, what=f"L {L} deriv {deriv} nine {with_nine} src {src}")
                for option in ("no_peak_slots", "no_span", "no_peak_hot"):
                    sess.set_option(option, True)
                    try:
                        assert sess.find_peaks(src, use_derivative=deriv, **kw).tobytes() == got.tobytes(), option
                    finally:
                        sess.set_option(option, False)
    sess.profile(False)


def test_zero_width_window_is_numpys_error(sess):
    """ext = 0 around a peak whose rounded intersection points coincide: the reference raises numpy's ValueError."""
    fam, lay = U.FAMILY["prominence"], LAYOUTS[3]
    rec, pool = U.embed_records(U.signals_for(fam, lay, False), lay, False)
    sess.upload_pool(pool)
    sess.upload_records(rec, 0.0)
    kw = dict(fam.options[0], use_derivative=False, height_window_extension=0)
    with pytest.raises(ValueError, match="zero-size array"):
        O.find_peak_hits(rec, pool, **kw)
    with pytest.raises(ValueError, match="zero-size array"):
        sess.find_peaks(_lib.SRC_RAW, **kw)


@pytest.mark.parametrize("fam", U.FAMILIES, ids=lambda f: f.name)
@pytest.mark.parametrize("lay", [LAYOUTS[1], LAYOUTS[4], LAYOUTS[6]], ids=lambda l: l.name)
def test_hit_finder_plugin(fam, lay):
    """The same cases through HipHitFinderPlugin: records, st_waveforms and filtered_waveforms sources."""
    for deriv in (False, True):
        sig = U.signals_for(fam, lay, deriv)
        rec, pool = U.embed_records(sig, lay, deriv, "negative", fam.float_values)
        f32 = U.f32_twin(pool)
        st16 = None if fam.float_values else U.embed_dense(sig, lay, deriv, np.int16)
        st32 = U.embed_dense(sig, lay, deriv, np.float32, fam.float_values)
        for opt in fam.options[:2]:
            cfg = dict(opt, use_derivative=deriv, height_method="minmax", height_window_extension=1)
            for filtered in (True,) if fam.float_values else (False, True):
                data = {"records": rec, "wave_pool_filtered": f32}
                if not fam.float_values:
                    data["wave_pool"] = pool
                ctx = SimpleContext({"wave_source": "records", "hit": dict(cfg, use_filtered=filtered)}, data,
                                    plugins=[HipHitFinderPlugin()])
                G.assert_struct_equal(ctx.get_data("run", "hit"), O.find_peak_hits(rec, f32 if filtered else pool, **cfg),
                                      what=f"records filtered={filtered} {cfg}")
            for source, st in (("st_waveforms", st16), ("filtered_waveforms", st32)):
                if st is None:
                    continue
                ctx = SimpleContext({"hit": dict(cfg, use_filtered=False, wave_source=source)}, {source: st},
                                    plugins=[HipHitFinderPlugin()])
                G.assert_struct_equal(ctx.get_data("run", "hit"), O.find_peak_hits_dense(st, **cfg), what=f"{source} {cfg}")


@pytest.mark.parametrize("name", ["ties", "tied_noise", "width"])
@pytest.mark.parametrize("lay", [LAYOUTS[0], LAYOUTS[3]], ids=lambda l: l.name)
def test_signal_peaks_stream_plugin(name, lay):
    """The tied families through HipSignalPeaksStreamPlugin, chunk by chunk against O.signal_peaks_rows."""
    fam = U.FAMILY[name]
    for deriv in (False, True):
        sig = U.signals_for(fam, lay, deriv)
        st = U.embed_dense(sig, lay, deriv, np.int16)
        st["timestamp"] = 10**6 * np.arange(len(st))  # (chunk bounds are float picoseconds: keep them small here)
        f32 = U.embed_dense(sig, lay, deriv, np.float32)
        f32["timestamp"] = st["timestamp"]
        for opt in fam.options:
            cfg = dict(opt, use_derivative=deriv, height_method="diff")
            outs = list(HipSignalPeaksStreamPlugin().compute(SimpleContext(cfg, {"st_waveforms": st, "filtered_waveforms": f32}),
                                                             "run", streaming_config={"parallel": False, "break_threshold_ps": 0}))
            want = []
            for ch in np.unique(st["channel"]):
                rows, frows = st[st["channel"] == ch], f32[st["channel"] == ch]
                cuts = np.concatenate([[0], np.flatnonzero(np.diff(rows["dt"])) + 1, [len(rows)]])
                for a, b in zip(cuts[:-1], cuts[1:]):
                    part = O.signal_peaks_rows(rows[a:b], frows[a:b], **cfg)
                    if len(part):
                        want.append(part)
            assert len(outs) == len(want) and len(want) > 0
            for chunk, part in zip(outs, want):
                G.assert_struct_equal(chunk.data, part, what=f"{name} {lay.name} {cfg}")


# ------------------------------------------------------------------------------------------------
# waveform_width and s1_s2
# ------------------------------------------------------------------------------------------------
WW_CASES = [(L, kind, seed) for L in U.WW_LENGTHS for kind in ("int16", "float32", "tiny") for seed in (0, 1)]


@pytest.mark.parametrize("L,kind,seed", WW_CASES)
def test_waveform_width_edges(sess, L, kind, seed):
    st, hits = U.ww_rows(L, kind, seed)
    name = "st_waveforms" if kind == "int16" else "filtered_waveforms"
    pool, src, row_len = dense.dense_pool(st)
    assert row_len == L
    row = first_row_of_record_id(st["record_id"], hits["record_id"])
    keep = U.ww_valid_mask(hits, st)
    assert 0 < keep.sum() < len(keep)
    # hits in front of the row: numpy would index from the end; the kernel drops them and the plugin refuses them
    position = np.concatenate([hits["position"], [-1, -L, -L - 1]])
    row_neg = np.concatenate([row, row[keep][:3]])
    for opt in U.WW_OPTIONS:
        want = O.waveform_width(hits, st, **opt)
        got = SimpleContext({"waveform_width": dict(opt, use_filtered=kind != "int16")}, {name: st, "hit": hits},
                            plugins=[HipWaveformWidthPlugin()]).get_data("run", "waveform_width")
        G.assert_struct_equal(got, want, what=f"plugin L {L} {kind} {opt}")
        sess.upload_pool(pool)
        rows, valid = sess.waveform_width(src, position, row_neg, len(st), L, **opt)
        np.testing.assert_array_equal(valid[:len(hits)], keep)
        assert not valid[len(hits):].any()
        for f in ("rise_time", "fall_time", "total_width", "rise_time_samples", "fall_time_samples", "total_width_samples",
                  "peak_position", "peak_height"):
            np.testing.assert_array_equal(rows[:len(hits)][keep][f], want[f], err_msg=f"session L {L} {kind} {opt} {f}")
    bad = hits.copy()
    bad["position"][0] = -1
    with pytest.raises(Exception, match="positions >= 0"):
        SimpleContext({"waveform_width": {"use_filtered": kind != "int16"}}, {name: st, "hit": bad},
                      plugins=[HipWaveformWidthPlugin()]).get_data("run", "waveform_width")


@pytest.mark.parametrize("L,kind", [(51, "int16"), (150, "float32"), (800, "int16")])
def test_s1_s2_bounds_equal_to_produced_values(L, kind):
    """Ranges whose bounds ARE produced widths / heights / areas: the bounds are inclusive on both sides."""
    st, hits = U.ww_rows(L, kind, 0)
    name = "st_waveforms" if kind == "int16" else "filtered_waveforms"
    rng = np.random.default_rng(L)
    feats = np.zeros(200, dtype=BASIC_FEATURES_DTYPE)
    feats["height"], feats["area"] = rng.integers(1, 9, 200) * 0.5, rng.integers(1, 9, 200) * 1.25
    widths = SimpleContext({"waveform_width": {"use_filtered": kind != "int16"}}, {name: st, "hit": hits},
                           plugins=[HipWaveformWidthPlugin()]).get_data("run", "waveform_width")
    G.assert_struct_equal(widths, O.waveform_width(hits, st))
    for unit, col in (("ns", "total_width"), ("samples", "total_width_samples")):
        vals = np.unique(widths[col])
        assert len(vals) >= 4
        lo, mid, hi = float(vals[1]), float(vals[len(vals) // 2]), float(vals[-2])
        cfg = dict(width_unit=unit, s1_width_range=(lo, mid), s2_width_range=(mid, hi), s1_height_range=(1.0, 2.5),
                   s2_area_range=(2.5, 7.5), conflict_policy="prefer_s2")
        got = SimpleContext({"s1_s2": cfg}, {"waveform_width": widths, "basic_features": feats},
                            plugins=[HipS1S2ClassifierPlugin()]).get_data("run", "s1_s2")
        G.assert_struct_equal(got, O.s1_s2_classify(widths, feats, **cfg), what=f"{unit}")
        w = widths[col].astype(np.float64)
        h, a = feats["height"][widths["record_id"]], feats["area"][widths["record_id"]]
        s1 = (w >= lo) & (w <= mid) & (h >= 1.0) & (h <= 2.5)
        s2 = (w >= mid) & (w <= hi) & (a >= 2.5) & (a <= 7.5)
        np.testing.assert_array_equal(got["label"], np.where(s2, 2, np.where(s1, 1, 0)))
        for on_bound in (w == lo, w == mid, w == hi, (h == 1.0) | (h == 2.5), (a == 2.5) | (a == 7.5)):
            assert on_bound.any()
