"""The hit-table stages on the GPU (wfa_hits.hip: lexsort, k_hit_prep / k_float_keys, k_event_flags, k_merge_chain,
k_merge_emit, wfa_records_sort) on the key, window and summation edges of tests/hit_table_edges_util.py, against the
oracle's literal loops.  `test_hit_table_edges_cpu.py` shows that those tables reach their edges and that the oracle agrees
with an independent restatement; here every comparison is exact: integer outputs with assert_array_equal, float32 heights,
integrals and widths bit for bit.  There is no tolerance anywhere in this file.

Not tested: NaN heights.  np.max would propagate a NaN where k_merge_emit's `v > max_h` loop does not, but both hit finders
produce finite heights by construction (a height is a difference of finite samples), and no reference path yields one.
Starts at or above 2^63 and a NaN in only one of the two fix arrays are outside the documented contract of the C ABI.
"""

import ctypes as C

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests import hit_table_edges_util as U
from waveformanalysis_amd import _lib, records_builder
from waveformanalysis_amd.device import DeviceSession, _ptr
from waveformanalysis_amd.event_grouping import group_hit_windows_flat
from waveformanalysis_amd.hit_merge import compute_cluster_rows, compute_merged_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sess():
    s = DeviceSession(0)
    yield s
    s.close()


# ---- helpers --------------------------------------------------------------------------------------------------------------
def run_grouping(sess, hits, window_ns, fix0=None, fix1=None):
    return sess.group_hit_windows(hits["timestamp"], hits["position"], hits["edge_start"], hits["edge_end"], hits["dt"],
                                  hits["board"], hits["channel"], hits["record_id"], window_ns, fix0, fix1)


def flat_events(events):
    """The oracle's event list in the flat form of wfa_group_hit_windows_fill."""
    order = np.concatenate([np.asarray(m, dtype=np.int64) for _, _, m in events]) if events else np.zeros(0, np.int64)
    start = np.concatenate(([0], np.cumsum([len(m) for _, _, m in events]))).astype(np.int64)
    return {"order": order, "event_start": start, "t_min": np.array([e[0] for e in events], dtype=np.int64),
            "t_max": np.array([e[1] for e in events], dtype=np.int64)}


def route_of(hits, fix0=None, fix1=None):
    a0 = np.array(U.abs_windows(hits, fix0, fix1)[0])
    return "float keys" if np.any(np.abs(a0) >= U.KEY_SWITCH) or np.any(a0 != np.floor(a0)) else "integer keys"


def explain(hits, got, want, fix0=None, fix1=None):
    """First differing position of two orders with the keys on both sides and the key route the table took."""
    n = min(len(got), len(want))
    bad = np.flatnonzero(np.asarray(got[:n]) != np.asarray(want[:n]))
    if len(bad) == 0:
        return f"orders agree on their first {n} entries ({len(got)} vs {len(want)}); {route_of(hits, fix0, fix1)}"
    j = int(bad[0])
    a0, a1 = U.abs_windows(hits, fix0, fix1)

    def keys(i):
        h = hits[i]
        return (f"hit {i}: abs_start {a0[i]!r} abs_end {a1[i]!r} dt {h['dt']} timestamp {h['timestamp']} record_id "
                f"{h['record_id']} board {h['board']} channel {h['channel']}")

    return f"first difference at position {j} ({route_of(hits, fix0, fix1)}): got {keys(int(got[j]))}; want {keys(int(want[j]))}"


def assert_flat_equal(hits, got, want, what, fix0=None, fix1=None):
    if not np.array_equal(got["order"], want["order"]):
        pytest.fail(f"{what}: order differs; " + explain(hits, got["order"], want["order"], fix0, fix1))
    for k in ("event_start", "t_min", "t_max"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k} ({route_of(hits, fix0, fix1)})")


def run_merge(sess, hits, gap, cap):
    return sess.hit_merge_clusters(hits["timestamp"], hits["position"], hits["edge_start"], hits["edge_end"], hits["dt"],
                                   hits["board"], hits["channel"], gap, cap)


def assert_clusters_equal(hits, got, clusters, what):
    order, offset = got
    want_order = np.array([i for c in clusters for i in c], dtype=np.int64)
    if not np.array_equal(order, want_order):
        pytest.fail(f"{what}: order differs; " + explain(hits, order, want_order))
    np.testing.assert_array_equal(offset, np.concatenate(([0], np.cumsum([len(c) for c in clusters]))), err_msg=what)


def run_emit(sess, hits, clusters):
    member = np.array([i for c in clusters for i in c], dtype=np.int64)
    offset = np.concatenate(([0], np.cumsum([len(c) for c in clusters]))).astype(np.int64)
    return sess.hit_merge_emit(hits["timestamp"], hits["edge_start"], hits["edge_end"], hits["record_id"], hits["height"],
                               hits["integral"], member, offset)


def assert_emit_equal(hits, clusters, got, what):
    """wfa_hit_merge_emit against the restatement, which test_hit_table_edges_cpu.py pins to the oracle's rows; clusters of
    one hit are the hit itself on the host (compute_merged_rows) and only their anchor is compared."""
    want = U.merged_model(hits, clusters)
    multi = np.array([len(c) > 1 for c in clusters])
    np.testing.assert_array_equal(got["anchor"], [w[0] for w in want], err_msg=f"{what}: anchor")
    for k, col in (("height", 1), ("integral", 2), ("width", 5)):
        w = np.array([x[col] for x in want], dtype=np.float32)
        np.testing.assert_array_equal(got[k].view(np.uint32)[multi], w.view(np.uint32)[multi], err_msg=f"{what}: {k} bits")
    for k, col in (("sample_start", 3), ("sample_end", 4)):
        np.testing.assert_array_equal(got[k][multi], np.array([x[col] for x in want])[multi], err_msg=f"{what}: {k}")


# ---- event grouping -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.group_case_names())
def test_grouping_on_edge_tables(sess, name):
    case = U.group_case(name)
    hits, f0, f1 = case["hits"], case["fix0"], case["fix1"]
    for w in case["windows"]:
        want = flat_events(O.group_hit_windows_literal(hits, w, f0, f1))
        assert_flat_equal(hits, run_grouping(sess, hits, w, f0, f1), want, f"{name} window {w}", f0, f1)
    if name.endswith("+".join(U.KEY_NAMES)):  # every key constant: every radix pass is skipped, the identity remains
        np.testing.assert_array_equal(run_grouping(sess, hits, 0.0)["order"], np.arange(len(hits)))


@pytest.mark.parametrize("base", U.INTEGER_ROUTE_BASES)
def test_float_keys_agree_with_integer_keys(sess, base):
    """One extra row at or above 4.0e18, in a channel and at a time of its own, switches ALL rows to k_float_keys: without
    that row the result must be what the integer keys gave (and what the oracle gives)."""
    hits = U.key_route(base)
    far = U.with_far_row(hits)
    n = len(hits)
    assert route_of(hits) == "integer keys" and route_of(far) == "float keys"
    for w in (0.0, 100.0):
        by_int = run_grouping(sess, hits, w)
        by_float = run_grouping(sess, far, w)
        ev = int(np.searchsorted(by_float["event_start"], int(np.flatnonzero(by_float["order"] == n)[0]), side="right")) - 1
        assert by_float["event_start"][ev + 1] - by_float["event_start"][ev] == 1  # the far row is an event of its own
        keep = by_float["order"] != n
        start = np.delete(by_float["event_start"], ev + 1)
        start[ev + 1:] -= 1
        dropped = {"order": by_float["order"][keep], "event_start": start,
                   "t_min": np.delete(by_float["t_min"], ev), "t_max": np.delete(by_float["t_max"], ev)}
        assert_flat_equal(hits, dropped, by_int, f"{base} window {w}: float keys vs integer keys")
        assert_flat_equal(hits, by_int, flat_events(O.group_hit_windows_literal(hits, w)), f"{base} window {w}")
    gap, cap = 30.0, 900.0
    by_int, by_float = run_merge(sess, hits, gap, cap), run_merge(sess, far, gap, cap)
    assert by_float[0][-1] == n  # the far row's (board, channel) sorts last
    np.testing.assert_array_equal(by_float[0][:-1], by_int[0])
    np.testing.assert_array_equal(by_float[1][:-1], by_int[1])
    assert_clusters_equal(hits, by_int, O.hit_merge_clusters(hits, gap, cap), f"{base} merge")


def test_grouping_through_the_python_layer(sess):
    for name in ("A-straddle", "B-0.0005-2p62", "D-257-vary", "C-boundaries"):
        case = U.group_case(name)
        if case["fix0"] is not None:
            continue
        for w in case["windows"][:2]:
            flat = group_hit_windows_flat(case["hits"], w, session=sess)
            assert_flat_equal(case["hits"], flat, flat_events(O.group_hit_windows_literal(case["hits"], w)), f"{name} {w}")


# ---- hit merge ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.merge_case_names())
def test_merge_on_edge_tables(sess, name):
    case = U.merge_case(name)
    hits = case["hits"]
    for gap, cap in case["configs"]:
        clusters = O.hit_merge_clusters(hits, gap, cap)
        assert_clusters_equal(hits, run_merge(sess, hits, gap, cap), clusters, f"{name} gap {gap} cap {cap}")
        assert_emit_equal(hits, clusters, run_emit(sess, hits, clusters), f"{name} gap {gap} cap {cap}")


@pytest.mark.parametrize("name", ["C-boundaries", "C-long_segment", "A-below_2p63"])
def test_merge_through_the_python_layer(sess, name):
    case = U.merge_case(name)
    hits = case["hits"]
    gap, cap = case["configs"][0]
    clusters = O.hit_merge_clusters(hits, gap, cap)
    rows = compute_cluster_rows(sess, hits, gap, cap, None, "t")
    G.assert_struct_equal(rows, O.hit_merge_cluster_rows(clusters), what=name)
    G.assert_struct_equal(compute_merged_rows(sess, hits, rows, None, "t"), O.hit_merged_rows(hits, clusters), what=name)


def test_integral_sums_follow_numpys_tree(sess):
    """The float32 integral of every (size, pattern) pair says which way its float64 additions were nested
    (np_pairwise_sum in k_merge_emit): all pairs in one launch (more than 256 clusters: several blocks, one LDS column per
    thread), then a few clusters per launch."""
    sets = U.integral_ties()
    hits, clusters = U.clusters_table([x for _, _, x in sets])
    assert len(clusters) > 256
    want = O.hit_merged_rows(hits, clusters)
    got = run_emit(sess, hits, clusters)
    bad = np.flatnonzero(got["integral"].view(np.uint32) != want["integral"].view(np.uint32))
    assert len(bad) == 0, [(sets[k][0], sets[k][1], float(got["integral"][k]), float(want["integral"][k])) for k in bad[:10]]
    assert_emit_equal(hits, clusters, got, "integral ties, one launch")
    G.assert_struct_equal(compute_merged_rows(sess, hits, O.hit_merge_cluster_rows(clusters), None, "t"), want)
    for a in range(0, len(clusters), 61):
        some = clusters[a:a + 7]
        part = run_emit(sess, hits, some)
        np.testing.assert_array_equal(part["integral"].view(np.uint32), want["integral"][a:a + 7].view(np.uint32))


def test_anchor_ties_and_windows(sess):
    hits, clusters = U.anchor_ties()
    assert_emit_equal(hits, clusters, run_emit(sess, hits, clusters), "anchor ties")
    G.assert_struct_equal(compute_merged_rows(sess, hits, O.hit_merge_cluster_rows(clusters), None, "t"),
                          O.hit_merged_rows(hits, clusters))


# ---- records sort ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.sort_case_names())
def test_records_sort_on_key_extremes(sess, name):
    rec = U.sort_case(name)
    want = O.records_sort_order(rec)
    np.testing.assert_array_equal(sess.records_sort_order(rec["timestamp"], rec["pid"], rec["board"], rec["channel"]), want,
                                  err_msg=name)
    if name.startswith("257-"):
        np.testing.assert_array_equal(records_builder.records_sort_order(rec, session=sess), want, err_msg=name)


# ---- resident rows, state reuse, argument checks --------------------------------------------------------------------------
def test_resident_rows_at_a_fractional_window_and_an_exact_gap():
    """The rows of a real hit pass, read on the device (hit_rows_source("hits")), against the oracle: with a window of half
    a picosecond, and with a merge gap that equals a gap between two hits of the data."""
    from waveformanalysis_amd import synth

    rec, pool = synth.make_run(4000, "v1725", cfg=91)
    with DeviceSession(0) as s:
        s.upload_pool(pool)
        s.upload_records(rec, 10.0)
        s.set_sg_plan(11, 2)
        rows = s.threshold_hits(_lib.SRC_SG_FUSED, 2, 2)
        n = len(rows)
        assert n > 3000
        # a gap that occurs: the commonest positive distance from a hit's end to the next start of its channel
        a0, a1 = (np.array(v) for v in U.abs_windows(rows))
        o = np.lexsort((a0, rows["channel"], rows["board"]))
        same = (rows["board"][o][1:] == rows["board"][o][:-1]) & (rows["channel"][o][1:] == rows["channel"][o][:-1])
        d = (a0[o][1:] - a1[o][:-1])[same]
        d = d[(d > 0) & (d < 1e6)]
        d = d[(d / 1e3) * 1e3 == d]  # gaps that the ns -> ps conversion of the C ABI reproduces exactly
        values, counts = np.unique(d, return_counts=True)
        gap_ps = float(values[np.argmax(counts)])
        gap_ns = gap_ps / 1e3
        clusters, met = U.merge_model(rows, gap_ns, 10000.0)
        assert met["gap_eq"] >= 1
        assert clusters == O.hit_merge_clusters(rows, gap_ns, 10000.0)
        s.hit_rows_source("hits")
        got = s.group_hit_windows_resident(n, 0.0005)
        assert_flat_equal(rows, got, flat_events(O.group_hit_windows_literal(rows, 0.0005)), "resident rows, window 0.0005")
        assert_clusters_equal(rows, s.hit_merge_clusters_resident(n, gap_ns, 10000.0), clusters, f"resident rows, gap {gap_ns}")


def test_scratch_is_reused_across_sizes_and_stages(sess):
    """Scratch slots grow and never shrink, and lexsort may start from an earlier result (init_perm): a large table, a tiny
    one and the large one again, with other stages and one release_scratch() in between, all give the oracle's answer."""
    big, tiny = U.group_case("D-65537-vary"), U.group_case("D-2-vary")
    want_big = flat_events(O.group_hit_windows_literal(big["hits"], 0.0))
    want_tiny = flat_events(O.group_hit_windows_literal(tiny["hits"], 0.0))
    rec = U.sort_case("257-vary")
    merge = U.merge_case("C-boundaries")
    clusters = O.hit_merge_clusters(merge["hits"], U.MERGE_GAP_NS, U.MERGE_CAP_NS)
    assert_flat_equal(big["hits"], run_grouping(sess, big["hits"], 0.0), want_big, "large")
    assert_flat_equal(tiny["hits"], run_grouping(sess, tiny["hits"], 0.0), want_tiny, "tiny after large")
    assert_clusters_equal(merge["hits"], run_merge(sess, merge["hits"], U.MERGE_GAP_NS, U.MERGE_CAP_NS), clusters, "merge")
    assert_flat_equal(big["hits"], run_grouping(sess, big["hits"], 0.0), want_big, "large again")
    np.testing.assert_array_equal(sess.records_sort_order(rec["timestamp"], rec["pid"], rec["board"], rec["channel"]),
                                  O.records_sort_order(rec))
    assert sess.release_scratch() > 0
    assert_flat_equal(tiny["hits"], run_grouping(sess, tiny["hits"], 0.0), want_tiny, "tiny after release_scratch")
    assert_flat_equal(big["hits"], run_grouping(sess, big["hits"], 0.0), want_big, "large after release_scratch")
    assert_clusters_equal(merge["hits"], run_merge(sess, merge["hits"], U.MERGE_GAP_NS, U.MERGE_CAP_NS), clusters, "merge again")


def test_c_abi_argument_checks(sess):
    """Malformed calls the session wrapper cannot make: the documented code and message, and the session stays usable."""
    lib = sess._lib
    hits = U.key_extremes(257)
    n = len(hits)
    cols = [np.ascontiguousarray(hits[k]) for k in ("timestamp", "position", "edge_start", "edge_end", "dt", "board", "channel",
                                                   "record_id")]
    fix = np.full(n, np.nan)
    m = C.c_int64(0)

    def group_count(h, columns, f0, f1, window):
        return lib.wfa_group_hit_windows_count(h, n, *[_ptr(c) for c in columns], _ptr(f0), _ptr(f1), window, C.byref(m))

    for k in range(8):  # one NULL column among non-NULL ones
        some = list(cols)
        some[k] = None
        assert group_count(sess._h, some, None, None, 10.0) == _lib.WFA_E_INVALID
        assert "null column" in _lib.last_error()
    for k in range(7):
        some = list(cols[:7])
        some[k] = None
        assert lib.wfa_hit_merge_count(sess._h, n, *[_ptr(c) for c in some], 10.0, 100.0, C.byref(m)) == _lib.WFA_E_INVALID
        assert "null column" in _lib.last_error()
    for f0, f1 in ((fix, None), (None, fix)):  # only one of the two fix arrays
        assert group_count(sess._h, cols, f0, f1, 10.0) == _lib.WFA_E_INVALID
        assert "pass both abs_*_fix arrays or neither" in _lib.last_error()
    assert group_count(sess._h, cols, None, None, -1e-9) == _lib.WFA_E_INVALID
    assert "time_window_ns must be >= 0" in _lib.last_error()
    # _fill with the wrong sizes after a good _count
    assert group_count(sess._h, cols, None, None, 10.0) == _lib.WFA_OK
    k = int(m.value)
    order, start, t0, t1 = np.empty(n + 1, np.int64), np.empty(k + 2, np.int64), np.empty(k + 1, np.int64), np.empty(k + 1, np.int64)
    for bad_n, bad_k in ((n + 1, k), (n - 1, k), (n, k + 1), (n, k - 1)):
        assert lib.wfa_group_hit_windows_fill(sess._h, bad_n, bad_k, _ptr(order), _ptr(start), _ptr(t0), _ptr(t1)) == \
            _lib.WFA_E_INVALID
        assert "caller expects" in _lib.last_error()
    assert lib.wfa_hit_merge_fill(sess._h, n, k, _ptr(order), _ptr(start)) == _lib.WFA_E_STATE  # the last pass was a grouping
    assert "no hit merge pass has been run" in _lib.last_error()
    assert lib.wfa_group_hit_windows_fill(sess._h, n, k, _ptr(order), _ptr(start), _ptr(t0), _ptr(t1)) == _lib.WFA_OK
    want = flat_events(O.group_hit_windows_literal(hits, 10.0))
    np.testing.assert_array_equal(order[:n], want["order"])
    np.testing.assert_array_equal(start[:k + 1], want["event_start"])
    assert lib.wfa_hit_merge_count(sess._h, n, *[_ptr(c) for c in cols[:7]], 10.0, 100.0, C.byref(m)) == _lib.WFA_OK
    for bad_n, bad_k in ((n + 1, int(m.value)), (n, int(m.value) + 1)):
        assert lib.wfa_hit_merge_fill(sess._h, bad_n, bad_k, _ptr(order), _ptr(start)) == _lib.WFA_E_INVALID
        assert "caller expects" in _lib.last_error()
    # _fill before any _count on a fresh session
    with DeviceSession(0) as fresh:
        assert lib.wfa_group_hit_windows_fill(fresh._h, n, k, _ptr(order), _ptr(start), _ptr(t0), _ptr(t1)) == _lib.WFA_E_STATE
        assert "no event grouping pass has been run" in _lib.last_error()
        assert lib.wfa_hit_merge_fill(fresh._h, n, k, _ptr(order), _ptr(start)) == _lib.WFA_E_STATE
        assert "no hit merge pass has been run" in _lib.last_error()
