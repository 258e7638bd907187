"""The Savitzky-Golay plan grid on the device: every plan of tests/sg_reference.plan_grid() materialised through the
span kernel (where the plan takes it) and through k_savgol, and fed to the fused hit routes, against scipy and the
exact reference.

* interior samples are bit-exact to scipy (the centre uses scipy's own coefficient bits, or the integer numerator
  above its guard);
* inside the parity set every non-zero edge sample is bit-exact to scipy;
* everywhere, a sample is RN_f32(exact) on the span kernel's integer edge route above its guard, and within the
  float route's bound (tests/sg_reference.float_route_bound, plus one float32 ulp) otherwise;
* outside the parity set a strict xfail keeps the difference from scipy on record."""

import functools

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests import sg_reference as R
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DeviceSession
from waveformanalysis_amd.sg_plan import build_plan

pytestmark = pytest.mark.gpu

GRID = R.plan_grid()
UNIFORM_L = 64


@functools.cache
def _case(W, P, layout):
    p = R.ragged_pool(W, P) if layout == "ragged" else R.uniform_pool(W, P, L=UNIFORM_L)
    ref = O.filter_wave_pool(p.records(), p.pool, "SG", sg_window_size=W, sg_poly_order=P)
    return p, R.expect(p, W, P), ref


def _span_plan(W, P):
    return build_plan(W, P).int_ok and 5 <= W <= 15


def _session(p, W, P, thresholds=10.0, records=None, **options):
    s = DeviceSession(0)
    for k, v in options.items():
        s.set_option(k, v)
    s.upload_pool(p.pool)
    s.upload_records(p.records() if records is None else records, thresholds)
    s.set_sg_plan(W, P)
    s.profile(True)
    return s


def _ran(sess, *prefixes, absent=()):
    names = sorted(sess.profile_report())
    for k in prefixes:
        assert any(n.startswith(k) for n in names), (k, names)
    for k in absent:
        assert not any(n.startswith(k) for n in names), (k, names)


@functools.cache
def _materialised(W, P, layout, no_fast):
    p, e, ref = _case(W, P, layout)
    with _session(p, W, P, no_fast=no_fast) as s:
        got = s.savgol()
        names = sorted(s.profile_report())
    return got, names


ROUTES = [("ragged", False), ("uniform", False), ("uniform", True)]


def _integer_edges(W, P, e, p):
    """Edge samples the span kernel takes on its integer route: full window, numerator >= guard_edge."""
    plan = build_plan(W, P)
    out = np.zeros(len(p.pool), dtype=bool)
    for i in np.flatnonzero(e.edge & (e.window == W)):
        num = e.exact[i] * plan.den_edge
        assert num.denominator == 1
        out[i] = num >= plan.guard_edge
    return out


@pytest.mark.parametrize("layout,no_fast", ROUTES)
@pytest.mark.parametrize("W,P", GRID)
def test_materialised_filter(W, P, layout, no_fast):
    p, e, ref = _case(W, P, layout)
    got, names = _materialised(W, P, layout, no_fast)
    span = layout == "uniform" and not no_fast and _span_plan(W, P)
    want_kernel = "k_savgol_span" if span else "k_savgol"
    assert any(n == want_kernel for n in names), (want_kernel, names)
    gaps = ~(e.copy | e.edge | e.interior)
    assert not np.any(got[gaps]), "samples between records must stay 0"
    np.testing.assert_array_equal(got[e.copy], p.pool[e.copy].astype(np.float32))
    bad = np.flatnonzero(e.interior & (got != ref))
    assert len(bad) == 0, ("interior", [(int(i), float(got[i]), float(ref[i])) for i in bad[:5]])
    edges = np.flatnonzero(e.edge)
    ok = R.within_bound(got, e, edges)
    assert ok.all(), ("bound", [(int(i), float(got[i]), float(e.rn[i]), float(e.bound[i])) for i in edges[~ok][:5]])
    if span:
        ie = _integer_edges(W, P, e, p)
        bad = np.flatnonzero(ie & (got != e.rn))
        assert len(bad) == 0, ("integer edges", [(int(i), float(got[i]), float(e.rn[i])) for i in bad[:5]])
    if R.in_parity_set(W, P):
        nz = np.array([q != 0 for q in e.exact])
        bad = np.flatnonzero(e.edge & nz & (got != ref))
        assert len(bad) == 0, ("parity", [(int(i), float(got[i]), float(ref[i])) for i in bad[:5]])


OUTSIDE = [(W, P) for W, P in GRID if not R.in_parity_set(W, P)]
# per band of orders; in each band scipy's edges differ from RN_f32(exact) on several plans of the grid
# (tests/test_sg_grid_cpu.py), so each xfail below fails for a reason of its own band
BANDS = {"P7-9": (7, 9), "P10-12": (10, 12), "P13-19": (13, 19), "P20-62": (20, 62)}


@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason="above the parity set the reference's edge values come from an ill-conditioned polyfit and "
                          "differ from the exact value the device returns")
@pytest.mark.parametrize("layout,no_fast", ROUTES)
@pytest.mark.parametrize("band", BANDS)
def test_edges_outside_parity_set_match_reference(band, layout, no_fast):
    lo, hi = BANDS[band]
    plans = [(W, P) for W, P in OUTSIDE if lo <= P <= hi]
    assert plans
    bad = {}
    for W, P in plans:
        p, e, ref = _case(W, P, layout)
        got, _ = _materialised(W, P, layout, no_fast)
        n = int(np.sum(e.edge & (got != ref)))
        if n:
            bad[(W, P)] = n
    assert not bad, bad


# ---- fused hit routes on the uniform pools -------------------------------------------------------------------------
def _hit_inputs(W, P):
    """Records with positive polarity and baseline 0 (signal = y) whose threshold is the device's own value at one of
    their edge samples: record k decides on sample k % (2h) of the left or right edge."""
    p, e, ref = _case(W, P, "uniform")
    dev, _ = _materialised(W, P, "uniform", False)  # the span kernel where the plan takes it
    rec = p.records()
    rec["baseline"] = 0.0
    rec["polarity"] = "positive"
    h = max(W // 2, 1)
    thr = np.empty(len(rec))
    for k, (o, L) in enumerate(p.slices()):
        j = k % (2 * h)
        i = j if j < h else L - 2 * h + j
        thr[k] = float(dev[o + min(i, L - 1)])
    return p, rec, thr, dev, ref


HIT_ROUTES = {
    "general": ({"no_fast": True}, ("k_hits<sg_fused>",)),
    "bitmap": ({"no_runs32": True}, ("k_sg_mask", "k_hit_runs")),
    "streaming": ({}, ("k_sg_runs32",)),
}
HIT_PLANS = [(W, P) for W, P in GRID if W >= 3 and (W <= 23 or (W, P) in R.LARGE_HIGH)]
HIT_CELLS = [(W, P, r) for W, P in HIT_PLANS for r in HIT_ROUTES
             if r == "general" or 5 <= W <= (11 if r == "streaming" else 15)]


@pytest.mark.parametrize("W,P,route", HIT_CELLS)
def test_fused_hit_routes(W, P, route):
    """Each route gives the oracle's rows on the device's own materialised pool (and the oracle's rows on scipy's pool
    where the two pools agree).  A plan without an integer plan falls back to the general route: that is asserted."""
    opts, kernels = HIT_ROUTES[route]
    if not build_plan(W, P).int_ok:
        kernels = ("k_hits<sg_fused>",)
    p, rec, thr, dev, ref = _hit_inputs(W, P)
    want = O.threshold_hits(rec, dev, thresholds=thr)
    assert len(want) >= len(rec)
    with _session(p, W, P, thresholds=thr, records=rec, **opts) as s:
        got = s.threshold_hits(_lib.SRC_SG_FUSED, 2, 2)
        _ran(s, *kernels)
    G.assert_struct_equal(got, want, float_rtol=1e-6, what=f"SG({W},{P}) {route}")
    if R.in_parity_set(W, P):
        # against the oracle's rows on scipy's pool, on every record whose filtered samples equal scipy's; the others
        # differ from scipy only at edge samples whose exact value is 0 (scipy returns rounding noise there)
        e = _case(W, P, "uniform")[1]
        nz = np.array([q != 0 for q in e.exact])
        assert not np.any((dev != ref) & (nz | ~e.edge))
        same = np.array([np.array_equal(dev[o : o + L], ref[o : o + L]) for o, L in p.slices()])
        assert same.sum() >= len(rec) // 2, (W, P, int((~same).sum()))
        keep = np.flatnonzero(same)
        want_ref = O.threshold_hits(rec, ref, thresholds=thr)
        G.assert_struct_equal(got[np.isin(got["record_id"], keep)], want_ref[np.isin(want_ref["record_id"], keep)],
                              float_rtol=1e-6, what=f"SG({W},{P}) {route} vs oracle")


# ---- reference fixtures at the new corners (tests/golden/sgbw_sg*.npz, made by the reference's plugins) -------------
SG_FIXTURES = ["sgbw_sg15_13", "sgbw_sg21_16", "sgbw_sg63_12"]


@functools.cache
def _fixture(name):
    c = G.load_case(name)
    fp = G.filter_params(c)
    W, P = fp["sg_window_size"], fp["sg_poly_order"]
    rec = c["records"]
    p = R.Pool(c["wave_pool"], rec["event_length"].astype(np.int64), rec["wave_offset"].astype(np.int64), [])
    with _session(p, W, P, thresholds=G.hit_params(c)["thresholds"], records=rec) as s:
        got = s.savgol()
        hits = s.threshold_hits(_lib.SRC_SG_FUSED, 2, 2)
    return c, (W, P), R.expect(p, W, P), got, hits


@pytest.mark.parametrize("name", SG_FIXTURES)
def test_reference_fixture_by_the_parity_rule(name):
    """Copies and interior samples are bit-exact to the reference; every edge sample is within the float route's bound of
    the exact value (bit-exact to the reference as well, where the plan is in the parity set); the fused hit pass gives
    the oracle's rows on the device's pool, and the reference's rows on every record whose samples equal the
    reference's."""
    c, (W, P), e, got, hits = _fixture(name)
    ref = c["wave_pool_filtered"]
    assert not np.any(got[~(e.copy | e.edge | e.interior)])
    np.testing.assert_array_equal(got[e.copy | e.interior], ref[e.copy | e.interior])
    edges = np.flatnonzero(e.edge)
    assert R.within_bound(got, e, edges).all()
    if R.in_parity_set(W, P):
        np.testing.assert_array_equal(got, ref)
    rec = c["records"]
    hp = G.hit_params(c)
    G.assert_struct_equal(hits, O.threshold_hits(rec, got, **hp), float_rtol=1e-6, what=f"{name} fused vs device pool")
    same = [int(r) for r, o, L in zip(rec["record_id"], rec["wave_offset"], rec["event_length"])
            if np.array_equal(got[o : o + L], ref[o : o + L])]
    # the other records differ from the reference only at edge samples (asserted above): outside the parity set that is
    # most records of SG(21,16), every record in the parity set
    assert same and (len(same) == len(rec) or not R.in_parity_set(W, P))
    want = c["hits_filt"]
    G.assert_struct_equal(hits[np.isin(hits["record_id"], same)], want[np.isin(want["record_id"], same)],
                          float_rtol=1e-6, what=f"{name} fused vs reference")


@pytest.mark.xfail(strict=True, raises=AssertionError,
                   reason="SG(15,13) and SG(21,16): the reference's polyfit edges differ from the exact value the device "
                          "returns")
def test_reference_fixture_high_order_edges_match_reference():
    bad = 0
    for name in SG_FIXTURES[:2]:
        c, _, e, got, _ = _fixture(name)
        bad += int(np.sum(e.edge & (got != c["wave_pool_filtered"])))
    assert bad == 0, bad
