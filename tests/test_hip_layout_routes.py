"""Which kernels a records layout reaches, and what invalidates what the device context derived from an upload.

The library detects a uniform layout (equal lengths, back to back, one polarity class) once per records upload and
routes the fused hit pass and the materialised Savitzky-Golay filter by it: the streaming kernel in place or on the
padded shadow of the pool, the span16 mask kernel in place or on the shadow, or the per-record kernels.  Every layout
on either side of those conditions, through both upload routes (packed rows / columns) and under every option that
selects another path: rows against the oracle, byte-identical across routes and options, and the kernels the profile
names.  Then the state rules: a new pool voids the shadow and the records, a float32 twin of equal size keeps them,
release_scratch() gives back exactly what scratch_bytes() counts and the next pass rebuilds it."""

import functools
import re

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from waveformanalysis_amd import _lib, synth
from waveformanalysis_amd.device import DeviceSession

pytestmark = pytest.mark.gpu
FLOAT_RTOL = 1e-6          # tolerance of tests/test_hip_padded.py for the float fields of a hit row
N = 200                    # more than three spans of 64 records
WINDOW = (0, synth.BASELINE_SAMPLES)
STAGE = {"k_pad_rows", "k_sg_runs32", "k_sg_mask_span16", "k_sg_mask", "k_hits"}   # what tells the routes apart

RUNS, RUNS_PAD = {"k_sg_runs32"}, {"k_pad_rows", "k_sg_runs32"}
SPAN16, SPAN16_PAD = {"k_sg_mask_span16"}, {"k_pad_rows", "k_sg_mask_span16"}
MASK, LITERAL = {"k_sg_mask"}, {"k_hits"}
# layout -> route of the fused hit pass with SG(11,2) by option (no_fast: the float64 kernel for every layout), and the
# kernel of savgol()
ROUTES = {
    "L64":      ({"": RUNS, "no_runs32": SPAN16, "no_pad": RUNS, "no_span": RUNS}, "k_savgol_span"),
    "L88":      ({"": RUNS_PAD, "no_runs32": SPAN16_PAD, "no_pad": MASK, "no_span": RUNS_PAD}, "k_savgol_span<padded>"),
    "L90":      ({"": RUNS_PAD, "no_runs32": SPAN16_PAD, "no_pad": MASK, "no_span": RUNS_PAD}, "k_savgol_span<padded>"),
    "L72":      ({"": SPAN16_PAD, "no_runs32": SPAN16_PAD, "no_pad": MASK, "no_span": MASK}, "k_savgol_span<padded>"),
    "L40":      ({"": SPAN16_PAD, "no_runs32": SPAN16_PAD, "no_pad": MASK, "no_span": MASK}, "k_savgol_span<padded>"),
    "L80":      ({"": SPAN16, "no_runs32": SPAN16, "no_pad": SPAN16, "no_span": MASK}, "k_savgol_span"),
    "L68":      ({"": MASK, "no_runs32": MASK, "no_pad": MASK, "no_span": MASK}, "k_savgol_span<padded>"),
    "L24":      ({"": MASK, "no_runs32": MASK, "no_pad": MASK, "no_span": MASK}, "k_savgol_span"),
    "ragged":   ({"": MASK, "no_runs32": MASK, "no_pad": MASK, "no_span": MASK}, "k_savgol"),
    "L64off4":  ({"": MASK, "no_runs32": MASK, "no_pad": MASK, "no_span": MASK}, "k_savgol"),
    "L64mixed": ({"": MASK, "no_runs32": MASK, "no_pad": MASK, "no_span": MASK}, "k_savgol"),
}
OPTIONS = ("", "no_runs32", "no_pad", "no_span", "no_fast")


def _with_baselines(rec, pool):
    rec = rec.copy()
    for i in range(len(rec)):   # integer sum / count, as np.mean over float64 of integer samples
        o, n = int(rec["wave_offset"][i]), min(synth.BASELINE_SAMPLES, int(rec["event_length"][i]))
        rec["baseline"][i] = int(pool[o : o + n].sum(dtype=np.int64)) / float(n)
    return rec


@functools.lru_cache(maxsize=None)
def _case(name, cfg=0):
    """(records with their baselines, pool, oracle rows, oracle filtered pool) of one layout; computed once."""
    L = int(re.match(r"L(\d+)", name).group(1)) if name.startswith("L") else 64
    rec, pool = synth.make_run(N, "vx2730", cfg=300 + cfg + L, L=L)
    rng = np.random.default_rng(1000 + cfg + L)
    w = pool.reshape(N, L).astype(np.int32)
    for i in range(N):          # dips anywhere in the record, the edge samples included
        for _ in range(int(rng.integers(1, 3))):
            a = int(rng.integers(-4, L))
            w[i, max(a, 0) : a + int(rng.integers(3, 11))] -= int(rng.integers(15, 600))
    pool = w.clip(0, 16383).astype(np.uint16).reshape(-1)
    if name == "ragged":        # lengths 40..64 back to back inside the same pool
        length = rng.integers(40, 65, N).astype(np.int32)
        rec["event_length"] = length
        rec["wave_offset"] = np.concatenate([[0], np.cumsum(length[:-1], dtype=np.int64)])
    elif name == "L64off4":
        pool = np.concatenate([np.zeros(4, np.uint16), pool])
        rec["wave_offset"] += 4
    elif name == "L64mixed":    # one record of the other polarity class, in the last span
        rec["polarity"][N - 3] = "positive"
    rec = _with_baselines(rec, pool)
    filtered = O.filter_wave_pool(rec, pool)
    want = O.threshold_hits(rec, filtered)
    assert len(want) > 100
    for a in (rec, pool, want, filtered):
        a.setflags(write=False)
    return rec, pool, want, filtered


def _names(report):
    return {re.sub(r"[<( ].*", "", k) for k in report}


def _hit_pass(sess, rec, fused):
    """One fused hit pass on freshly uploaded records -> (rows, profile names).  The upload voids what the previous
    pass derived (the padded shadow, the baselines a fused pass wrote), so every pass shows its whole route."""
    rec_in = rec.copy()
    if fused:
        rec_in["baseline"] = np.nan
    sess.upload_records(rec_in, 10.0)
    sess.profile(True)
    if fused:
        rows = sess.fused_baseline_filter_hits(WINDOW, 2, 2)
    else:
        rows = sess.threshold_hits(_lib.SRC_SG_FUSED, 2, 2)
    return rows, set(sess.profile_report())


@functools.lru_cache(maxsize=None)
def _route_table(name, packed):
    """Every option x (baselines given, fused window) of one layout on one session -> {(option, fused): (rows, names)}."""
    rec, pool, want, filtered = _case(name)
    out = {}
    with DeviceSession(0) as sess:
        sess.packed_records = packed
        sess.upload_pool(pool)
        sess.set_sg_plan(11, 2)
        for option in OPTIONS:
            if option:
                sess.set_option(option, True)
            for fused in (False, True):
                out[option, fused] = _hit_pass(sess, rec, fused)
            if option:
                sess.set_option(option, False)
        sess.upload_records(rec, 10.0)
        sess.profile(True)
        out["savgol"] = (sess.savgol(), set(sess.profile_report()))
    return out


@pytest.mark.parametrize("name", list(ROUTES))
def test_route_table(name):
    rec, pool, want, filtered = _case(name)
    routes, savgol_kernel = ROUTES[name]
    got = _route_table(name, True)
    first = got["", False][0]
    for option in OPTIONS:
        for fused in (False, True):
            rows, report = got[option, fused]
            what = f"{name} option={option or 'none'} fused={fused}"
            G.assert_struct_equal(rows, want, float_rtol=FLOAT_RTOL, what=what)
            if option == "no_fast":  # the float64 kernel: its float fields agree to the tolerance, not to the last bit
                G.assert_struct_equal(rows, first, float_rtol=FLOAT_RTOL, what=what)
            else:
                assert rows.tobytes() == first.tobytes(), what
            assert _names(report) & STAGE == (LITERAL if option == "no_fast" else routes[option]), (what, report)
            stage = [k for k in report if _names([k]) & (STAGE - {"k_pad_rows"})]
            assert all(("baseline" in k) == fused for k in stage), (what, report)
    out, report = got["savgol"]
    np.testing.assert_array_equal(out, filtered, err_msg=name)
    assert {k for k in report if k.startswith("k_savgol")} == {savgol_kernel}, (name, report)


@pytest.mark.parametrize("name", list(ROUTES))
def test_both_upload_routes_one_layout(name):
    packed, columns = _route_table(name, True), _route_table(name, False)
    assert packed.keys() == columns.keys()
    for key in packed:
        assert packed[key][0].tobytes() == columns[key][0].tobytes(), (name, key)
        assert _names(packed[key][1]) == _names(columns[key][1]), (name, key)


def test_invalidation():
    rec, pool_a, want_a, _f = _case("L88")
    _r, pool_b, _w, _f = _case("L88", cfg=7)
    assert pool_a.size == pool_b.size and not np.array_equal(pool_a, pool_b)
    want_b = O.threshold_hits(_with_baselines(rec, pool_b), O.filter_wave_pool(rec, pool_b))
    assert want_a.tobytes() != want_b.tobytes()
    with DeviceSession(0) as sess:
        sess.set_sg_plan(11, 2)
        # (a) a new pool of the same size under the same records: a stale shadow would give run A's rows
        sess.upload_pool(pool_a)
        rows, report = _hit_pass(sess, rec, True)
        assert "k_pad_rows" in _names(report)
        G.assert_struct_equal(rows, want_a, float_rtol=FLOAT_RTOL, what="run A")
        sess.upload_pool(pool_b)
        rows_b, report = _hit_pass(sess, rec, True)
        G.assert_struct_equal(rows_b, want_b, float_rtol=FLOAT_RTOL, what="run B")
        # (b) the scratch given back: the next pass builds the shadow again and finds the same rows
        assert sess.release_scratch() > 0
        sess.profile(True)
        again = sess.threshold_hits(_lib.SRC_SG_FUSED, 2, 2)     # baselines: the ones the fused pass left
        assert again.tobytes() == rows_b.tobytes()
        assert "k_pad_rows" in _names(sess.profile_report())
        # (d) a float32 twin of equal size keeps the records usable
        sess.upload_filtered_pool(np.zeros(pool_b.size, np.float32))
        assert sess.threshold_hits(_lib.SRC_SG_FUSED, 2, 2).tobytes() == rows_b.tobytes()
        # (c) a new pool alone, uploaded or gathered on the device, voids the records
        sess.upload_pool(pool_a)
        with pytest.raises(_lib.WfaError, match="records not uploaded"):
            sess.threshold_hits(_lib.SRC_SG_FUSED, 2, 2)
        _hit_pass(sess, rec, True)
        sess.pool_gather(rec["wave_offset"], rec["event_length"], pool_b, download=False)
        with pytest.raises(_lib.WfaError, match="records not uploaded"):
            sess.threshold_hits(_lib.SRC_SG_FUSED, 2, 2)
        rows, _report = _hit_pass(sess, rec, True)
        G.assert_struct_equal(rows, want_b, float_rtol=FLOAT_RTOL, what="gathered pool")


def test_scratch_accounting():
    rec, pool, want, _f = _case("L88")
    with DeviceSession(0) as sess:
        sess.set_sg_plan(11, 2)
        sess.upload_pool(pool)
        rows, _report = _hit_pass(sess, rec, True)
        held = sess.scratch_bytes()
        assert held > 0
        assert sess.release_scratch() == held
        assert sess.scratch_bytes() == 0
        assert sess.release_scratch() == 0
