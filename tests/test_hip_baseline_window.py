"""The baseline window [start, min(end, L)) over its whole range on every route that computes it.

Cases and their CPU proof: tests/baseline_window_util.py, tests/test_baseline_window_cpu.py.  For every layout of
tests/test_hip_layout_routes.py, every route selector (its options, and SG(21,4) as a plan outside the fast set) and every
window: (1) baseline_mean equals the integer rule exactly, NaN positions included; (2) the fused pass on records
uploaded with NaN baselines gives the oracle's rows for the reference baselines; (3) the pass with those baselines
given gives the same bytes; (4) so does a pass straight after the fused one, on the baselines it left in the context;
(5) the profile names the kernels meant.  Then a window whose sum does not fit 32 bits on the span16 kernel, queued
passes that are redone with their window, the refusals, and the plugin's fuse_baseline on both of its routes."""

import functools

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import baseline_window_util as U
from tests import golden_util as G
from tests import test_hip_layout_routes as LR
from waveformanalysis_amd import _lib, synth
from waveformanalysis_amd.device import DeviceSession
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipThresholdHitPlugin, HipWavePoolFilteredPlugin

pytestmark = pytest.mark.gpu
FLOAT_RTOL = LR.FLOAT_RTOL


def _blank(rec):
    rec = rec.copy()
    rec["baseline"] = np.nan
    return rec


def _window_passes(sess, rec_ref, window, write_back=True):
    """The five device results of one window on a session whose pool, plan and options are set."""
    sess.upload_records(_blank(rec_ref), U.THRESHOLD)
    baselines = sess.baseline_mean(*window)
    sess.profile(True)
    fused = sess.fused_baseline_filter_hits(window, 2, 2)
    report = set(sess.profile_report())
    again = sess.threshold_hits(_lib.SRC_SG_FUSED, 2, 2) if write_back else None   # no upload in between
    sess.upload_records(rec_ref, U.THRESHOLD)
    given = sess.threshold_hits(_lib.SRC_SG_FUSED, 2, 2)
    return baselines, fused, report, again, given


@functools.lru_cache(maxsize=None)
def _passes(name, selector):
    """{window: (baselines, fused rows, profile names, rows after the fused pass, rows with baselines given)}."""
    _rec, pool, _want, _filt = LR._case(name)
    out = {}
    with DeviceSession(0) as sess:
        sess.upload_pool(pool)
        sess.set_sg_plan(*U.plan_of(selector))
        if selector in LR.OPTIONS and selector:
            sess.set_option(selector, True)
        for window in U.windows(name):
            out[window] = _window_passes(sess, U.case(name, window)[0], window)
    return out


def _check_profile(report, fused_stage, what):
    assert LR._names(report) & LR.STAGE == fused_stage, (what, report)
    stage = [k for k in report if LR._names([k]) & (LR.STAGE - {"k_pad_rows"})]
    assert stage and all("baseline" in k for k in stage), (what, report)


@pytest.mark.parametrize("selector", U.SELECTORS)
@pytest.mark.parametrize("name", U.LAYOUTS)
def test_window_on_route(name, selector):
    got = _passes(name, selector)
    assert list(got) == U.windows(name)
    for window, (baselines, fused, report, again, given) in got.items():
        rec_ref, _pool, want = U.case(name, window, U.plan_of(selector))
        what = f"{name} selector={selector or 'none'} window={window}"
        np.testing.assert_array_equal(baselines, rec_ref["baseline"], err_msg=what)                      # 1
        G.assert_struct_equal(fused, want, float_rtol=FLOAT_RTOL, what=what)                             # 2
        if np.isnan(rec_ref["baseline"]).all():
            assert len(fused) == 0, what
        assert given.tobytes() == fused.tobytes(), what                                                  # 3
        assert again.tobytes() == fused.tobytes(), what                                                  # 4
        _check_profile(report, U.expected_stage(name, selector, window), what)                           # 5
        runs32 = any(k.startswith("k_sg_runs32") for k in report)
        assert runs32 == (window == U.CONTROL and "k_sg_runs32" in U.expected_stage(name, selector, window)), what


@pytest.mark.parametrize("name", U.LAYOUTS)
def test_fast_selectors_give_one_table(name):
    """Whatever kernel the options leave for a window, the rows are the same bytes (test_route_table: (0, 40) only)."""
    first = _passes(name, "")
    for selector in U.FAST[1:]:
        for window, result in _passes(name, selector).items():
            assert result[1].tobytes() == first[window][1].tobytes(), (name, selector, window)
    if name == "L64":       # the layout of the streaming kernel: it ran for the control window and for no other
        for window, result in first.items():
            kernel = "k_sg_runs32<baseline>" if window == U.CONTROL else "k_sg_mask_span16<baseline>"
            assert kernel in result[2], (window, result[2])


@pytest.mark.parametrize("name", list(U.BIG_LAYOUTS))
def test_sum_beyond_32_bits(name):
    """Records of 0xFFFF whose window sums pass 2**31 - 1 from 32 769 samples on, on the span16 kernel in place
    (L = 32 784) and on the padded shadow (L = 32 790): its per-record sum must be a 64-bit one."""
    for window in U.big_windows(name):
        rec_ref, pool, want = U.big_case(name, window)
        what = f"{name} window={window}"
        with DeviceSession(0) as sess:
            sess.upload_pool(pool)
            sess.set_sg_plan(11, 2)
            baselines, fused, report, _again, given = _window_passes(sess, rec_ref, window, write_back=False)
        stage = LR.SPAN16 if name == "L32784" else LR.SPAN16_PAD
        _check_profile(report, stage, what)
        assert "k_sg_mask_span16<baseline>" in report, (what, report)
        np.testing.assert_array_equal(baselines, rec_ref["baseline"], err_msg=what)
        G.assert_struct_equal(fused, want, float_rtol=FLOAT_RTOL, what=what)
        assert given.tobytes() == fused.tobytes(), what


def test_queued_pass_is_redone_with_its_window():
    """wfa_hits_enqueue with the window (5, 29) on the L80 layout (span16 in place).  A queued pass is launched for a
    row bound taken from the pass before (hits + hits / 8 + 4096) and redone inside the wait when it finds more; the redo
    must carry the window.  The 200 records of the layout cases cannot pass the bound's floor of 4096 rows, so this run
    has 8000 records of the same shape."""
    window, n_rec = (5, 29), 8000
    rec, pool = synth.make_run(n_rec, "vx2730", cfg=380, L=80)
    rec_ref = rec.copy()
    rec_ref["baseline"] = U.reference(rec, pool, window)
    want = O.threshold_hits(rec_ref, O.filter_wave_pool(rec, pool), threshold=U.THRESHOLD)
    with DeviceSession(0) as sess:
        sess.upload_pool(pool)
        sess.set_sg_plan(11, 2)
        sess.upload_records(_blank(rec), 1500.0)                  # few rows: a small row bound for what follows
        few = sess.fused_baseline_filter_hits(window, 2, 2)
        sess.hits_enqueue(_lib.SRC_SG_FUSED, window, 2, 2)
        assert sess.hits_wait() == len(few) > 0
        sess.upload_records(_blank(rec), U.THRESHOLD)             # more rows than that bound
        sess.hits_enqueue(_lib.SRC_SG_FUSED, window, 2, 2)
        n = sess.hits_wait()
        got = sess._fill_hits(n)
        waited = sess.fused_baseline_filter_hits(window, 2, 2)
        assert n == len(waited) > len(few) + len(few) // 8 + 4096
        assert got.tobytes() == waited.tobytes()
        G.assert_struct_equal(waited, want, float_rtol=FLOAT_RTOL, what="waited pass")
        np.testing.assert_array_equal(sess.baseline_mean(*window), rec_ref["baseline"])
        for _ in range(2):                                        # now within the bound: nothing waits in between
            sess.hits_enqueue(_lib.SRC_SG_FUSED, window, 2, 2)
        assert sess._fill_hits(sess.hits_wait()).tobytes() == waited.tobytes()


def test_refusals():
    rec, pool, _want, _filt = LR._case("L80")
    out = np.empty(len(rec), np.float64)
    n = _lib.C.c_int64(0)
    with DeviceSession(0) as sess:
        sess.upload_pool(pool)
        sess.set_sg_plan(11, 2)
        sess.upload_records(rec, U.THRESHOLD)
        sess.profile(True)
        for call in (lambda: sess.baseline_mean(-1, 5), lambda: sess.fused_baseline_filter_hits((-1, 5), 2, 2),
                     lambda: sess.hits_enqueue(_lib.SRC_SG_FUSED, (-1, 5), 2, 2)):
            with pytest.raises(ValueError, match="baseline window start must be >= 0"):
                call()
        # the C ABI itself, behind the Python check
        lib = sess._lib
        assert lib.wfa_baseline_mean(sess._h, -1, 5, 0, out.ctypes.data) == _lib.WFA_E_INVALID
        assert "baseline window start must be >= 0" in _lib.last_error()
        assert lib.wfa_fused_baseline_filter_hits(sess._h, -1, 5, 2, 2, 0, _lib.C.byref(n)) == _lib.WFA_E_INVALID
        assert "baseline window start must be >= 0" in _lib.last_error()
        assert sess.profile_report() == {}
    with DeviceSession(0) as sess:     # a float32 pool alone: nothing to take raw samples from
        sess.upload_filtered_pool(pool.astype(np.float32))
        sess.set_sg_plan(11, 2)
        sess.upload_records(rec, U.THRESHOLD)
        sess.profile(True)
        with pytest.raises(_lib.WfaError, match=r"wave_pool \(uint16\) not uploaded"):
            sess.baseline_mean(5, 29)
        with pytest.raises(_lib.WfaError, match=r"wave_pool \(uint16\) not uploaded"):
            sess.fused_baseline_filter_hits((5, 29), 2, 2)
        assert sess.profile_report() == {}


@pytest.mark.parametrize("name", ["L80", "ragged"])
def test_plugin_fuse_baseline_on_both_routes(name):
    rec, pool, _want, _filt = LR._case(name)
    L = U.max_len(name)
    for window in ((5, 29), (L - 1, 2**31 - 1)):
        rec_ref = rec.copy()
        rec_ref["baseline"] = U.reference(rec, pool, window)
        for cfg, plugins, waves in (({}, [HipThresholdHitPlugin()], pool),
                                    ({"use_filtered": True, "fuse_filter": True},
                                     [HipWavePoolFilteredPlugin(), HipThresholdHitPlugin()],
                                     O.filter_wave_pool(rec, pool))):
            ctx = SimpleContext({"wave_source": "records",
                                 "hit_threshold": {"threshold": U.THRESHOLD, "fuse_baseline": window, **cfg}},
                                {"records": rec.copy(), "wave_pool": pool.copy()}, plugins=plugins)
            got = ctx.get_data("run", "hit_threshold")
            want = O.threshold_hits(rec_ref, waves, threshold=U.THRESHOLD)
            what = f"{name} fuse_baseline={window} {cfg or 'raw'}"
            assert len(want) > (100 if window == (5, 29) else 0), what
            G.assert_struct_equal(got, want, float_rtol=FLOAT_RTOL, what=what)
