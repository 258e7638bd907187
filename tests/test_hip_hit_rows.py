"""Every threshold-hit route against the oracle and the plain-Python reference on the hit-row sets of
tests/hit_rows_util.py (tests/test_hit_rows_cpu.py proves that the sets show the rules they are named for): window clamp
and asymmetric extensions, a higher neighbouring run inside the window, ties for the maximum, the sign and guard edges of
the integral, and the shapes of k_hit_rows_flat's work lists.

Asserted per cell: every field but `integral` exactly (height as float32 bits); `integral` exactly on the raw sets and
on the Savitzky-Golay sets with dyadic baselines, within one float32 ulp on the sets with arbitrary baselines (DESIGN.md
section 2); rows byte-identical between all cells of a set that end in the row kernels k_hit_rows_flat /
k_hit_rows_literal (streaming, queued, bitmap and its variants: ROWS keeps the first such result per set and extension
pair, whichever test function runs first).  The k_hits routes are held to the references alone: where the integral has
its one-ulp allowance their lane-wise float64 sum may round differently from the flat kernel's  npos * sb - tsum.  Each
cell runs in a fresh session and asserts the kernels of its route ran, so a silent fallback cannot pass.
k_hit_rows_literal is launched behind k_hit_rows_flat on every pass, so the profile cannot tell which of the two wrote a
row; the HitAcc::add mutant in the "Shown to bite" list of DESIGN.md ("Pinned hit-row rules") does.

Every cell is held to the oracle on all extension pairs and to the plain-Python reference on one pair per set, rotating
over the sets (tests/test_hit_rows_cpu.py holds the oracle to that reference on every pair).

Thinned against the full cross product: every set runs on every route its layout allows with all of its extension
pairs; the option sets rotate over the sets: span_records 0 everywhere and 51 on every second set, the queued pass with
and without no_speculate on alternating sets, the bitmap route's no_span / no_pad variants on the set's first extension
pair only.
"""

import functools
import time

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import hit_rows_util as U
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DeviceSession
from waveformanalysis_amd.dtypes import create_record_dtype
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipThresholdHitPlugin, HipWavePoolFilteredPlugin

pytestmark = pytest.mark.gpu

LITCAP = "E_sg5_litcap"
SG = [n for n in U.names(source="sg", window=None) if n != LITCAP]
UNIFORM = [n for n in SG if U.by_name(n).layout != "ragged"]
RAW = U.names(source="raw")
FUSED = [hs.name for hs in U.fused_sets()]
FUSED40 = [n for n in FUSED if U.by_name(n).window == (0, 40)]  # the one baseline window k_sg_runs32 fuses
STREAMED = UNIFORM + FUSED40
ROWS = {}     # (set, le, re) -> rows of the first cell that went through the row kernels
HOST = [0.0]  # seconds spent on the host references (printed by test_arbitrary_baseline_integrals)


def _exact_pair(hs):
    """The extension pair on which the set's cells are also held to the plain-Python reference."""
    return hs.ext[[h.name for h in U.all_sets()].index(hs.name) % len(hs.ext)]


def _session(hs, *, f32=False, **options):
    s = DeviceSession(0)
    for k, v in options.items():
        s.set_option(k, v)
    s.upload_pool(hs.pool)
    if f32:
        s.upload_filtered_pool(hs.filtered)
    rec = hs.records.copy()
    if hs.window is not None:
        rec["baseline"] = np.nan  # the pass computes it
    s.upload_records(rec, hs.thresholds)
    if hs.source == "sg":
        s.set_sg_plan(*hs.plan)
    s.profile(True)
    return s


def _ran(sess, *prefixes, absent=()):
    names = sorted(sess.profile_report())
    for p in prefixes:
        assert any(k.startswith(p) for k in names), (p, names)
    for p in absent:
        assert not any(k.startswith(p) for k in names), (p, names)


def _check(got, hs, le, re, what, row_kernels=False):
    """-> number of integrals that are not bit-identical to the oracle's."""
    exact_integral = hs.source == "raw" or hs.dyadic
    what = f"{hs.name} ({le}, {re}) {what}"
    t0 = time.perf_counter()
    want = hs.oracle(le, re)
    plain = hs.exact(le, re)[0] if (le, re) == _exact_pair(hs) else None
    HOST[0] += time.perf_counter() - t0
    n = U.assert_rows(got, want, exact_integral=exact_integral, what=what + " vs oracle")
    if plain is not None:
        U.assert_rows(got, plain, exact_integral=exact_integral, what=what + " vs plain reference")
    if row_kernels:
        first = ROWS.setdefault((hs.name, le, re), got)
        assert got.tobytes() == first.tobytes(), what + ": rows differ from another route through the row kernels"
    return n


def _hits(s, hs, src, le, re):
    s.profile(True)
    if hs.window is not None:
        return s.fused_baseline_filter_hits(hs.window, le, re, max_len=hs.max_len)
    return s.threshold_hits(src, le, re, max_len=hs.max_len)


def _queued(s, hs, le, re):
    s.profile(True)
    s.hits_enqueue(_lib.SRC_SG_FUSED, hs.window or (0, 0), le, re, max_len=hs.max_len)
    return s._fill_hits(s.hits_wait())


STREAM_KERNELS = ("k_sg_runs32", "k_runs_to_desc", "k_hit_rows_flat")
BITMAP_KERNELS = ("k_sg_mask", "k_hit_runs", "k_hit_rows_flat")


@pytest.mark.parametrize("name", STREAMED)
def test_streaming_and_queued(name):
    """k_sg_runs32 + k_hit_rows_flat; then the same passes queued (hits_enqueue / hits_wait: the speculative row bound,
    or the exact count with no_speculate)."""
    hs = U.by_name(name)
    i = STREAMED.index(name)
    base = "k_sg_runs32<baseline>" if hs.window else "k_sg_runs32"
    for span_records in (0, 51) if i % 2 == 0 else (0,):
        opts = {"span_records": span_records} if span_records else {}
        with _session(hs, **opts) as s:
            for le, re in hs.ext:
                _check(_hits(s, hs, _lib.SRC_SG_FUSED, le, re), hs, le, re, f"streaming span_records={span_records}",
                       row_kernels=True)
                _ran(s, base, *STREAM_KERNELS[1:], absent=("k_sg_mask", "k_hits<"))
    no_speculate = i % 2 == 1
    with _session(hs, no_speculate=no_speculate) as s:
        _hits(s, hs, _lib.SRC_SG_FUSED, *hs.ext[0])
        for le, re in hs.ext:
            _check(_queued(s, hs, le, re), hs, le, re, f"queued no_speculate={no_speculate}", row_kernels=True)
            _ran(s, base, "k_hit_rows_flat", absent=("k_sg_mask", "k_hits<"))


@pytest.mark.parametrize("name", SG + FUSED)
def test_bitmap_route(name):
    """k_sg_mask / k_sg_mask_span16 + k_hit_runs + the same row kernels: ragged sets take it by themselves, uniform ones
    with no_runs32; no_span and (padded layout) no_pad choose among its mask kernels."""
    hs = U.by_name(name)
    variants = [{}] if hs.layout == "ragged" else [{"no_runs32": True}, {"no_runs32": True, "no_span": True}]
    if hs.layout == "padded":
        variants.append({"no_runs32": True, "no_pad": True})
    for k, opts in enumerate(variants):
        with _session(hs, **opts) as s:
            for le, re in hs.ext if k == 0 else hs.ext[:1]:
                _check(_hits(s, hs, _lib.SRC_SG_FUSED, le, re), hs, le, re, f"bitmap {opts}", row_kernels=True)
                _ran(s, *BITMAP_KERNELS, absent=("k_sg_runs32", "k_hits<"))
                if opts.get("no_span") or hs.layout == "ragged":
                    _ran(s, absent=("k_sg_mask_span16",))


@pytest.mark.parametrize("name", SG + FUSED)
def test_general_fused_route(name):
    """no_fast: k_hits<sg_fused> (per-lane strict maximum, then wave_argmax across lanes and 64-sample steps)."""
    hs = U.by_name(name)
    with _session(hs, no_fast=True) as s:
        for le, re in hs.ext:
            _check(_hits(s, hs, _lib.SRC_SG_FUSED, le, re), hs, le, re, "general")
            _ran(s, "k_hits<sg_fused,baseline>" if hs.window else "k_hits<sg_fused>",
                 absent=("k_sg_runs32", "k_sg_mask", "k_hit_rows"))


@pytest.mark.parametrize("name", RAW)
def test_raw_source(name):
    hs = U.by_name(name)
    with _session(hs) as s:
        for le, re in hs.ext:
            _check(_hits(s, hs, _lib.SRC_RAW, le, re), hs, le, re, "raw")
            _ran(s, "k_hits<raw>", absent=("k_sg_runs32", "k_sg_mask", "k_hits<sg", "k_hit_rows"))


@pytest.mark.parametrize("name", SG)
def test_materialised_filter_source(name):
    """k_hits<f32> on the float32 pool the oracle's filter gives."""
    hs = U.by_name(name)
    with _session(hs, f32=True) as s:
        for le, re in hs.ext:
            _check(_hits(s, hs, _lib.SRC_F32, le, re), hs, le, re, "f32")
            _ran(s, "k_hits<f32>", absent=("k_sg_runs32", "k_sg_mask", "k_hits<sg", "k_hit_rows"))


def test_literal_list_overflow():
    """More than kLitCap hits under the integer guard in one streaming pass: the flat kernel's list of them overflows and
    k_hit_rows_literal falls back to scanning the descriptors' flags.  The bitmap route keeps no such list (its literal
    kernel always scans the flags): it runs here as the second opinion the streaming rows must equal byte for byte.
    Against the oracle on every row; against the plain-Python reference on the first and the last 512 records, which is
    what a few seconds allow."""
    hs = U.by_name(LITCAP)
    (le, re), = hs.ext
    want = hs.oracle(le, re)
    assert len(want) > U.LIT_CAP
    k = 512
    rec = hs.records
    head = U.hit_rows_exact(rec[:k], hs.filtered, hs.thresholds[:k], le, re, hs.width)
    tail = U.hit_rows_exact(rec[-k:], hs.filtered, hs.thresholds[-k:], le, re, hs.width)
    assert len(head) == 2 * k and len(tail) == 2 * k and len(want) == 2 * len(rec)  # two hits per record
    first = None
    for opts, kernels in (({}, STREAM_KERNELS), ({"no_runs32": True}, BITMAP_KERNELS)):
        with _session(hs, **opts) as s:
            got = _hits(s, hs, _lib.SRC_SG_FUSED, le, re)
            _ran(s, *kernels, absent=("k_hits<",))
            U.assert_rows(got, want, exact_integral=True, what=f"{LITCAP} {opts}")
            U.assert_rows(got[:2 * k], head, exact_integral=True, what=f"{LITCAP} {opts} head")
            U.assert_rows(got[-2 * k:], tail, exact_integral=True, what=f"{LITCAP} {opts} tail")
            if first is None:
                first = got
                queued = _queued(s, hs, le, re)
                assert queued.tobytes() == got.tobytes()
            assert got.tobytes() == first.tobytes()


# ---- HipThresholdHitPlugin: asymmetric and negative extensions ---------------------------------------------------
def _plugin_cfg(hs, le, re, **more):
    cc = {f"{int(b)}:{int(c)}": {"threshold": float(t)}
          for b, c, t in zip(hs.records["board"], hs.records["channel"], hs.thresholds)}
    return dict(threshold=10.0, channel_config=cc, left_extension=le, right_extension=re, **more)


@pytest.mark.parametrize("ext", [(1, 9), (-3, 2), (9, 1)])
def test_plugin_records_route(ext):
    le, re = ext
    raw = U.by_name("A_raw_stream_neg")
    got = SimpleContext({"wave_source": "records", "hit_threshold": _plugin_cfg(raw, le, re)},
                        {"records": raw.records, "wave_pool": raw.pool},
                        plugins=[HipThresholdHitPlugin()]).get_data("run", "hit_threshold")
    U.assert_rows(got, raw.oracle(le, re), exact_integral=True, what=f"plugin records raw {ext}")
    U.assert_rows(got, U.hit_rows_exact(raw.records, raw.pool, raw.thresholds, le, re, raw.width), exact_integral=True,
                  what=f"plugin records raw {ext} vs plain reference")
    sg = U.by_name("A_sg11_stream_pos")  # (11, 2): the filter plugin's default
    more = dict(use_filtered=True, fuse_filter=True)
    if ext == (1, 9):
        more["devices"] = [0]
    got = SimpleContext({"wave_source": "records", "hit_threshold": _plugin_cfg(sg, le, re, **more)},
                        {"records": sg.records, "wave_pool": sg.pool},
                        plugins=[HipWavePoolFilteredPlugin(), HipThresholdHitPlugin()]).get_data("run", "hit_threshold")
    U.assert_rows(got, sg.oracle(le, re), exact_integral=True, what=f"plugin records fused sg {ext}")
    U.assert_rows(got, U.hit_rows_exact(sg.records, sg.filtered, sg.thresholds, le, re, sg.width), exact_integral=True,
                  what=f"plugin records fused sg {ext} vs plain reference")


@functools.cache
def _dense_input():
    hs = U.by_name("A_raw_stream_neg")
    rec = hs.records
    L = U.L_STREAM
    st = np.zeros(len(rec), dtype=create_record_dtype(L))
    for f in ("baseline", "polarity", "timestamp", "record_id", "dt", "board", "channel"):
        st[f] = rec[f]
    st["wave"] = hs.pool.reshape(-1, L).astype(np.int16)
    lengths = np.where(np.arange(len(rec)) % 3 == 1, L - 5 - np.arange(len(rec)) % 40, L)  # shorter than the row
    st["event_length"] = lengths
    dense_rec = np.zeros(len(rec), dtype=[("record_id", "i8"), ("event_length", "i4"), ("wave_offset", "i8")])
    dense_rec["record_id"], dense_rec["event_length"] = st["record_id"], lengths
    return hs, st, dense_rec, lengths


@pytest.mark.parametrize("ext", [(1, 9), (-3, 2), (9, 1)])
def test_plugin_dense_route(ext):
    """st_waveforms rows whose event_length is shorter than the row: the whole row is searched, the edges clamp to the
    record's length."""
    le, re = ext
    hs, st, dense_rec, lengths = _dense_input()
    got = SimpleContext({"hit_threshold": _plugin_cfg(hs, le, re)}, {"st_waveforms": st, "records": dense_rec},
                        plugins=[HipThresholdHitPlugin()]).get_data("run", "hit_threshold")
    want = O.threshold_hits_dense(st, lengths, thresholds=hs.thresholds, left_extension=le, right_extension=re)
    assert np.sum(want["edge_end"] < np.minimum(want["position"] + 1, U.L_STREAM)) >= 10  # the clamp is in use
    U.assert_rows(got, want, exact_integral=True, what=f"plugin dense {ext}")
    plain = U.hit_rows_exact(hs.records, hs.pool, hs.thresholds, le, re, hs.width)  # the whole row, then the clamp
    limit = lengths[plain["record_id"]].astype(np.int32)
    plain["edge_start"] = np.minimum(plain["edge_start"], limit)
    plain["edge_end"] = np.maximum(np.minimum(plain["edge_end"], limit), plain["edge_start"])
    plain["width"] = (plain["edge_end"] - plain["edge_start"]).astype(np.float32)
    U.assert_rows(got, plain, exact_integral=True, what=f"plugin dense {ext} vs plain reference")


ARBITRARY = [n for n in SG if not U.by_name(n).dyadic]


def test_arbitrary_baseline_integrals():
    """The sets whose integral has the one-ulp allowance, once more through the row kernels (the bitmap route takes every
    layout): prints how many integrals are not bit-identical to the oracle's (the figure in DESIGN.md) and, when the rest
    of the file ran in this process, the seconds it spent on the host references."""
    assert len(ARBITRARY) == 6
    differ, rows = {}, 0
    for name in ARBITRARY:
        hs = U.by_name(name)
        with _session(hs, **({} if hs.layout == "ragged" else {"no_runs32": True})) as s:
            for le, re in hs.ext:
                got = _hits(s, hs, _lib.SRC_SG_FUSED, le, re)
                differ[name] = differ.get(name, 0) + _check(got, hs, le, re, "count", row_kernels=True)
                rows += len(got)
    print(f"\nintegrals not bit-identical: {sum(differ.values())} of {rows} rows {differ}; host references {HOST[0]:.1f} s")
