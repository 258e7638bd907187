"""The S1/S2 peak chain on the device (wfa_peak_chain_count / _fill, DeviceSession.peak_chain, HipS1S2Stream) at the
edges tests/s1s2_edges_util.py builds: range bounds on values the run produces and one float32 / float64 step beside
them, every slot of the six ranges, one-sided, empty, infinite and NaN bounds, the conflict policies on rows that
match both classes, peak tables of 1, 127, 128, 129, 1024 and 1025 rows, a table whose peaks are all dropped, the
feature ranges, the four source pairs and record_id_base.  Every comparison is with the oracle chain, byte for byte
(tests/test_s1s2_edges_cpu.py shows that this comparison notices a subtly wrong chain)."""

import numpy as np
import pytest

from tests import s1s2_edges_util as E
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DeviceSession
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import hip_default
from waveformanalysis_amd.s1s2_stream import HipS1S2Stream

pytestmark = pytest.mark.gpu


def _stage(sess, layout, records=None):
    """Pool + records up, filter and find_peaks with nothing downloaded; returns the peak count."""
    rec, pool, hit_kw = E.edge_run(layout)
    sess.upload_pool(pool)
    sess.upload_records(rec if records is None else records, 0.0)
    sess.set_sg_plan(11, 2)
    sess.savgol(download=False)
    return sess.find_peaks(_lib.SRC_F32, download=False, **hit_kw)


@pytest.fixture(scope="module")
def ragged():
    """A session that holds the whole ragged run and its peak rows for the module: its tests only call peak_chain."""
    with DeviceSession(0) as s:
        assert _stage(s, "ragged") == len(E.oracle_hits("ragged")) > 1025
        yield s


@pytest.fixture(scope="module")
def sess():
    """A second session for the tests that upload tables of their own."""
    with DeviceSession(0) as s:
        yield s


def _columns(rows, names):
    """The bytes of some columns (a multi-field view would carry the other columns along as padding)."""
    return b"".join(np.ascontiguousarray(rows[n]).tobytes() for n in names)


# ---- 1. range cuts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", E.UNITS)
@pytest.mark.parametrize("slot", E.SLOTS)
def test_range_cuts_on_the_ragged_run(ragged, slot, unit):
    golden = E.golden()
    for i in (1, 0):  # with and without interpolation: bounds on the values of each table
        sets = {n: kw for n, kw in golden[f"sets_{i}"].items() if n.startswith(f"{slot}/{unit}/")}
        assert len(sets) == 22
        for name, kw in sets.items():
            want = E.oracle_rows("ragged", kw, interpolation=bool(i))
            assert np.array_equal(want["label"], golden[f"labels_{i}"][name])  # the recorded reference
            got = ragged.peak_chain(interpolation=bool(i), **kw)
            E.assert_chain_equal(got, want, f"{name}, interpolation={bool(i)}")


def test_conflict_policies_and_strict_on_the_ragged_run(ragged):
    golden = E.golden()
    for i in (1, 0):
        for policy, label in zip(E.POLICIES, (0, 1, 2, 0)):
            kw = golden[f"sets_{i}"][f"conflict/{policy}"]
            want = E.oracle_rows("ragged", kw, interpolation=bool(i))
            at_m = want["width_ns"] == np.float32(kw["s1_width_range"][1])
            assert at_m.any() and np.all(want["label"][at_m] == label)
            E.assert_chain_equal(ragged.peak_chain(interpolation=bool(i), **kw), want, f"conflict/{policy}, {i}")
    none = {name: (None, None) for name in E.SLOTS}
    ragged.profile(True)
    got = ragged.peak_chain(**none)
    report = ragged.profile_report()
    ragged.profile(False)
    E.assert_chain_equal(got, E.oracle_rows("ragged", none), "every range (None, None)")
    assert "k_basic_features" in report and "k_basic_features_leaf" not in report, sorted(report)  # ragged records
    assert "k_peak_chain" in report and "k_peak_chain_compact" in report
    with pytest.raises(ValueError) as err:
        ragged.peak_chain(strict=True, **none)
    assert str(err.value) == golden["strict_text"]
    with pytest.raises(ValueError) as err:
        E.oracle_rows("ragged", dict(strict=True, **none))
    assert str(err.value) == golden["strict_text"]
    E.assert_chain_equal(ragged.peak_chain(**none), E.oracle_rows("ragged", none), "after the refusal")


def test_range_cuts_on_the_uniform_run(sess):
    hits, _w, _f = E.oracle_tables("uniform")
    sess.profile(True)
    assert _stage(sess, "uniform") == len(hits)
    rows = E.oracle_rows("uniform", {})
    sets = E.conflict_sets(rows)
    for slot in E.SLOTS:
        for unit in E.UNITS:
            mine = E.slot_sets(rows, slot, unit)
            sets.update({n: mine[n] for n in (f"{slot}/{unit}/eq_m/both", f"{slot}/{unit}/ge_next64/alone")})
    seen = set()
    for name, kw in sets.items():
        want = E.oracle_rows("uniform", kw)
        seen |= set(want["label"].tolist())
        E.assert_chain_equal(sess.peak_chain(**kw), want, f"uniform, {name}")
    report = sess.profile_report()
    sess.profile(False)
    assert seen == {0, 1, 2}
    assert "k_basic_features_leaf" in report and "k_basic_features" not in report, sorted(report)
    assert "k_peak_chain" in report and "k_peak_chain_compact" in report


# ---- 2. block and drop edges ----------------------------------------------------------------------------------------
def _block_set():
    """Labels 0, 1 and 2 from width, area and height at once."""
    rows = E.oracle_rows("ragged", {})
    return dict(s1_width_range=(None, E.middle_value(rows, "width_ns")), s1_area_range=(E.middle_value(rows, "area", 1), None),
                s2_height_range=(E.middle_value(rows, "height"), None), s2_width_range=(E.middle_value(rows, "width_ns", 2), None))


def test_peak_tables_at_the_block_sizes_and_all_dropped(sess):
    kw = _block_set()
    whole = E.oracle_rows("ragged", kw)
    assert set(whole["label"].tolist()) == {0, 1, 2}
    prefix = E.prefix_lengths("ragged")
    for n in E.PEAK_COUNTS:
        assert _stage(sess, "ragged", E.subset("ragged", 0, prefix[n])) == n
        want = E.oracle_rows("ragged", kw, lo=0, hi=prefix[n])
        E.assert_chain_equal(sess.peak_chain(**kw), want, f"{n} peaks in {prefix[n]} records")
    assert len(E.oracle_rows("ragged", kw, lo=0, hi=prefix[1])) == 0  # (the first peak is a dropped one)
    assert _stage(sess, "ragged") == len(E.oracle_hits("ragged"))
    E.assert_chain_equal(sess.peak_chain(**kw), whole, "the whole run")
    # a table whose peaks are all dropped: nothing to compact, nothing to fill
    lo, hi = E.dropped_stretch("ragged")
    assert _stage(sess, "ragged", E.subset("ragged", lo, hi)) == len(E.oracle_tables("ragged", lo, hi)[0]) >= 130
    sess.profile(True)
    got = sess.peak_chain(**kw)
    report = sess.profile_report()
    sess.profile(False)
    E.assert_chain_equal(got, E.oracle_rows("ragged", kw, lo=lo, hi=hi), "all dropped")
    assert len(got) == 0 and "k_peak_chain" in report and "k_peak_chain_compact" not in report, sorted(report)
    assert _stage(sess, "ragged") == len(E.oracle_hits("ragged"))
    E.assert_chain_equal(sess.peak_chain(**kw), whole, "the whole run after the empty table")


# ---- 3. feature options, sources, record_id_base --------------------------------------------------------------------
FEATURE_RANGES = ((0, None), (0, 1), (3, 3), (52, 60), (10, 500))  # 52: behind the records of 0 .. 51 samples; 500: behind all


def _feature_set(layout, ranges):
    """An S1 height bound equal to a height and an S2 area bound equal to an area produced under `ranges`."""
    rows = E.oracle_rows(layout, {}, **ranges)
    pick = lambda col: E.middle_value(rows, col) if len(np.unique(rows[col])) >= 3 else float(rows[col][0])  # noqa: E731
    return dict(s1_height_range=(pick("height"), None), s2_area_range=(None, pick("area")))


@pytest.mark.parametrize("layout", ["ragged", "uniform"])
def test_feature_ranges(ragged, sess, layout):
    if layout == "uniform":
        assert _stage(sess, "uniform") == len(E.oracle_hits("uniform"))
    s = ragged if layout == "ragged" else sess
    default_rows = E.oracle_rows(layout, {})
    differ = 0
    for r in FEATURE_RANGES:
        for ranges in (dict(height_range=r), dict(area_range=r), dict(height_range=r, area_range=(r[0], r[1]))):
            kw = _feature_set(layout, ranges)
            want = E.oracle_rows(layout, kw, **ranges)
            assert np.any(want["height"] == np.float32(kw["s1_height_range"][0]))
            differ += _columns(want, ("height", "area")) != _columns(default_rows, ("height", "area"))
            E.assert_chain_equal(s.peak_chain(**kw, **ranges), want, f"{layout}, {ranges}")
    assert differ >= 12


@pytest.mark.parametrize("feature_source", [_lib.SRC_RAW, _lib.SRC_F32])
@pytest.mark.parametrize("width_source", [_lib.SRC_RAW, _lib.SRC_F32])
def test_source_pairs(ragged, width_source, feature_source):
    tables = dict(width_filtered=width_source == _lib.SRC_F32, features_filtered=feature_source == _lib.SRC_F32)
    rows = E.oracle_rows("ragged", {}, **tables)
    _h, widths, feats = E.oracle_tables("ragged", **tables)
    _h, raw_widths, raw_feats = E.oracle_tables("ragged")
    assert (widths.tobytes() != raw_widths.tobytes()) == tables["width_filtered"]
    assert (feats.tobytes() != raw_feats.tobytes()) == tables["features_filtered"]
    # bounds on values of these tables: narrow -> S1, large and not higher than the highest -> S2, both -> unknown
    kw = dict(s1_width_range=(None, E.median_value(rows, "width_ns")), s2_area_range=(E.median_value(rows, "area"), None),
              s2_height_range=(None, float(rows["height"].max())))
    want = E.oracle_rows("ragged", kw, **tables)
    assert set(want["label"].tolist()) == {0, 1, 2}
    E.assert_chain_equal(ragged.peak_chain(width_source, feature_source, **kw), want, f"sources {width_source}, {feature_source}")


@pytest.mark.parametrize("base", [0, 1, 2**40 + 3])
def test_record_id_base(ragged, base):
    kw = _block_set()
    want = E.oracle_rows("ragged", kw).copy()
    want["record_id"] += base
    got = ragged.peak_chain(record_id_base=base, **kw)
    E.assert_chain_equal(got, want, f"record_id_base {base}")
    others = [n for n in got.dtype.names if n != "record_id"]
    assert _columns(got, others) == _columns(E.oracle_rows("ragged", kw), others)


# ---- 4. the stream --------------------------------------------------------------------------------------------------
def _stream_sets():
    sets = E.golden()["sets_1"]
    return {n: sets[n] for n in ("s1_width_range/ns/eq_m/both", "s2_area_range/ns/ge_next64/both", "conflict/prefer_s2")}


def _context(records, class_kw, **kw):
    _rec, pool, hit_kw = E.edge_run("ragged")
    return SimpleContext({"wave_source": "records", **hit_kw, **class_kw}, {"records": records, "wave_pool": pool}, **kw)


@pytest.fixture(scope="module")
def static_rows():
    """The static HIP plugin chain on the whole run and on its first 64 records, per stream set."""
    rec = E.edge_run("ragged")[0]
    out = {}
    for name, kw in _stream_sets().items():
        for n in (len(rec), 64):
            rows = _context(rec[:n], kw, plugins=hip_default()).get_data("run", "s1_s2")
            rows.setflags(write=False)
            out[name, n] = rows
    return out


def _run_stream(records, class_kw, chunk_size):
    ctx = _context(records, class_kw)
    return list(HipS1S2Stream().compute(ctx, "run", streaming_config={"chunk_size": chunk_size, "parallel": False}))


@pytest.mark.parametrize("chunk_size", [7, 128, "all"])
def test_stream_on_the_ragged_run(static_rows, chunk_size):
    rec = E.edge_run("ragged")[0]
    c = len(rec) + 1 if chunk_size == "all" else chunk_size
    for name, kw in _stream_sets().items():
        want = E.oracle_rows("ragged", kw)
        E.assert_chain_equal(static_rows[name, len(rec)], want, f"static chain, {name}")
        outs = _run_stream(rec, kw, c)
        assert len(outs) == -(-len(rec) // c)
        got = np.concatenate([o.data for o in outs])
        E.assert_chain_equal(got, want, f"stream, {name}, chunks of {c}")
        assert got.tobytes() == static_rows[name, len(rec)].tobytes()
        for k, o in enumerate(outs):
            assert np.all(o.data["record_id"] // c == k), (name, k)
        if c == 7:  # chunks that hold peaks and keep none of them
            hits = E.oracle_hits("ragged")
            with_peaks = set((hits["record_id"] // c).tolist())
            with_rows = set((want["record_id"] // c).tolist())
            assert len(with_peaks - with_rows) >= 10
            assert all(len(outs[k].data) == 0 for k in with_peaks - with_rows)


def test_stream_record_by_record(static_rows):
    rec = E.edge_run("ragged")[0][:64]
    hits = E.oracle_hits("ragged")
    for name, kw in _stream_sets().items():
        want = E.oracle_rows("ragged", kw, lo=0, hi=64)
        assert len(want) > 20 and static_rows[name, 64].tobytes() == want.tobytes()
        outs = _run_stream(rec, kw, 1)
        assert len(outs) == 64
        E.assert_chain_equal(np.concatenate([o.data for o in outs]), want, f"stream, {name}, record by record")
        # record 0: one peak, dropped by the width stage -> an empty table
        assert (hits["record_id"] == 0).sum() == 1 and len(outs[0].data) == 0 and outs[0].data.dtype == want.dtype
        for k, o in enumerate(outs):
            assert np.all(o.data["record_id"] == k)
