"""The hit-table edge tables (tests/hit_table_edges_util.py) checked without a GPU: the oracle and the independent plain
Python restatement agree on every table; every table does reach the edge it is built for (asserted with counts, so a
builder that silently stops producing its edge fails here); and every way of being subtly wrong that the restatement can
be switched to (`MUTANTS`, the five wrong summation trees) is told apart from the oracle by at least one table."""

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import hit_table_edges_util as U


def oracle_events(case, window_ns):
    return [(t0, t1, [int(i) for i in m]) for t0, t1, m in
            O.group_hit_windows_literal(case["hits"], window_ns, case["fix0"], case["fix1"])]


def model_events(case, window_ns, **switch):
    return U.group_model(case["hits"], window_ns, case["fix0"], case["fix1"], quantum=case["quantum"], **switch)


def merged_fields(hits, rows):
    """The columns of the oracle's HIT_MERGED rows the model restates, anchor taken through its identifying fields."""
    return [(int(r["position"]), int(r["timestamp"]), int(r["record_id"]), np.float32(r["height"]).view(np.uint32),
             np.float32(r["integral"]).view(np.uint32), int(r["sample_start"]), int(r["sample_end"]),
             np.float32(r["width"]).view(np.uint32)) for r in rows]


def model_fields(hits, clusters, tree=None):
    out = []
    for anchor, h, q, s0, s1, w in U.merged_model(hits, clusters, tree):
        a = hits[anchor]
        out.append((int(a["position"]), int(a["timestamp"]), int(a["record_id"]), h.view(np.uint32), q.view(np.uint32), s0, s1,
                    w.view(np.uint32)))
    return out


# ---- (1) oracle == restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.group_case_names())
def test_grouping_oracle_equals_restatement(name):
    case = U.group_case(name)
    for w in case["windows"]:
        assert oracle_events(case, w) == model_events(case, w)[0], f"{name} window {w}"


@pytest.mark.parametrize("name", U.merge_case_names())
def test_merge_oracle_equals_restatement(name):
    case = U.merge_case(name)
    hits = case["hits"]
    for gap, cap in case["configs"]:
        want = O.hit_merge_clusters(hits, gap, cap)
        got, _ = U.merge_model(hits, gap, cap)
        assert got == want, f"{name} gap {gap} cap {cap}"
        assert model_fields(hits, got) == merged_fields(hits, O.hit_merged_rows(hits, want)), f"{name} rows {gap} {cap}"


@pytest.mark.parametrize("name", U.sort_case_names())
def test_record_sort_oracle_equals_restatement(name):
    rec = U.sort_case(name)
    want = O.records_sort_order(rec).tolist()
    assert U.sort_model(rec["timestamp"], rec["pid"], rec["board"], rec["channel"]) == want
    if name.endswith("+".join(U.SORT_KEYS)):
        assert want == list(range(len(rec)))  # every key constant: the identity


def test_anchor_ties_oracle_equals_restatement():
    hits, clusters = U.anchor_ties()
    rows = O.hit_merged_rows(hits, clusters)
    assert model_fields(hits, clusters) == merged_fields(hits, rows)
    # the edges the table is built for
    assert rows["timestamp"][0] == 3200 and rows["position"][1] == 20 and rows["timestamp"][2] == 10**6 - 1
    assert (rows["sample_start"][3], rows["sample_end"][3], rows["width"][3]) == (-1, -1, -1.0)
    assert rows["width"][4] == 0.0 and rows["width"][5] == 0.0 and rows["sample_end"][5] < rows["sample_start"][5] + 1
    assert rows["record_id"][6] == -2**63 and rows["timestamp"][6] == -2**62 - 1 and rows["sample_start"][7] == -1
    assert rows["component_count"][8] == 1


# ---- (2) the tables reach their edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", list(U.KEY_ROUTE_BASES))
def test_key_route_tables_sit_where_they_should(base):
    hits = U.key_route(base)
    a0, a1 = (np.array(v) for v in U.abs_windows(hits))
    share = float(np.mean(np.abs(a0) >= U.KEY_SWITCH))
    if base == "straddle":
        assert 0.1 <= share <= 0.9
    else:
        assert share == (1.0 if base in ("2p62", "below_2p63") else 0.0)
    assert a1.max() < U.COMPARABLE_END and np.all(a0 == np.floor(a0))
    if base == "negative":
        assert a0.max() < 0
    if base in ("2p58", "below_switch", "straddle", "2p62", "below_2p63"):
        ts = hits["timestamp"]
        o = np.lexsort((hits["record_id"], ts, hits["dt"], a0))
        ties = (a0[o][1:] == a0[o][:-1]) & (ts[o][1:] != ts[o][:-1])
        assert ties.mean() >= 0.30, ties.mean()
    far = U.with_far_row(hits)
    assert abs(U.abs_windows(far[-1:])[0][0]) >= U.KEY_SWITCH
    assert not np.any((far["board"][:-1] == far["board"][-1]) & (far["channel"][:-1] == far["channel"][-1]))


@pytest.mark.parametrize("name", [n for n in U.group_case_names() if n.startswith("B-")])
def test_window_boundaries_are_met_exactly(name):
    case = U.group_case(name)
    events, counts = model_events(case, case["design_window"])
    assert counts["eq"] >= 100 and counts["above"] >= 100 and counts["below"] >= 100, counts
    assert counts["held_earlier"] >= 300, counts  # the running max is held by an earlier hit than the previous one
    assert len(model_events(case, U.ONE_EVENT_WINDOW_NS)[0]) == 1
    if case["fix0"] is not None:  # fractional thresholds: the float keys
        f = case["fix0"][~np.isnan(case["fix0"])]
        assert np.any(f != np.floor(f))


def test_merge_boundaries_are_met_exactly():
    for name in ("C-boundaries", "C-boundaries-above_2p53"):
        case = U.merge_case(name)
        clusters, counts = U.merge_model(case["hits"], U.MERGE_GAP_NS, U.MERGE_CAP_NS, quantum=case["quantum"])
        for k in ("gap_eq", "gap_above", "gap_below", "cap_eq", "cap_above", "cap_below"):
            assert counts[k] >= 100, (name, counts)
        assert counts["shadowed"] >= 200, (name, counts)
        dt = case["hits"]["dt"]
        assert sum(1 for c in clusters if len(c) > 1 and dt[c[0]] == 2) >= 100  # clusters opened by a dt change
    assert U.quantum_at(2**53 + 2**40) == 2.0
    # merge_gap_ns = 0: every hit its own cluster, whatever the table
    hits = U.merge_case("C-boundaries")["hits"]
    assert all(len(c) == 1 for c in U.merge_model(hits, 0.0, U.MERGE_CAP_NS)[0])


def test_long_segment_and_many_segments():
    hits = U.long_segment()
    clusters, counts = U.merge_model(hits, U.MERGE_GAP_NS, U.MERGE_CAP_NS)
    a0, a1 = U.abs_windows(hits)
    main = sorted((i for i in range(len(hits)) if hits["channel"][i] == 3), key=a0.__getitem__)
    assert len(main) >= 20000
    run = a1[main[0]]
    for i in main[1:]:  # no gap ever cuts the channel: one segment, one walking lane
        assert a0[i] - run <= U.MERGE_GAP_NS * 1e3
        run = max(run, a1[i])
    assert sum(1 for c in clusters if hits["channel"][c[0]] == 3) >= 200  # ... cut by the cap alone
    hits = U.many_segments()
    assert len(hits) >= 50000
    for gap in (U.MERGE_GAP_NS, 0.001):
        assert all(len(c) == 1 for c in U.merge_model(hits, gap, U.MERGE_CAP_NS)[0])


def test_key_extremes_occur():
    for n in (255, 256, 257, 65537):
        hits = U.key_extremes(n)
        for field, values in (("board", U.I16), ("channel", U.I16), ("record_id", U.I64), ("dt", U.DT_EXTREMES)):
            assert set(values) <= set(hits[field].tolist()), (n, field)
        rec = U.record_sort_columns(n)
        for field, values in (("timestamp", U.I64), ("pid", U.I32), ("board", U.I16), ("channel", U.I16)):
            assert set(values) <= set(rec[field].tolist()), (n, field)
        assert len(np.unique(rec)) <= 7 * 4 * 4 * 4  # heavy ties: the stable order decides
    for n in U.KEY_SIZES:
        case = U.group_case(f"D-{n}-{'+'.join(U.KEY_NAMES)}")
        a0 = U.abs_windows(case["hits"])[0]
        assert len(set(a0)) == 1
        for w in case["windows"]:
            events = oracle_events(case, w)
            assert len(events) == 1 and events[0][2] == list(range(n))  # every key constant: the identity
    for c in U.KEY_NAMES:  # one constant key at a time: that one is constant, every other one varies
        hits = U.key_extremes(257, (c,))
        cols = dict(abs_start=np.array(U.abs_windows(hits)[0]), dt=hits["dt"], timestamp=hits["timestamp"],
                    record_id=hits["record_id"], board=hits["board"], channel=hits["channel"])
        for k, v in cols.items():
            assert (len(np.unique(v)) == 1) == (k == c), (c, k)


def test_fixed_windows_hold_their_edges():
    hits, f0, f1 = U.fixed_windows(True)
    assert np.signbit(f0[:8]).tolist() == [False, True] * 4 and np.all(f0[:8] == 0.0)
    case = U.group_case("E-fractional")
    events = oracle_events(case, 0.0)
    zeros = next(m for _, _, m in events if 0 in m)
    # the reference ties -0.0 with +0.0: the zeros stand in (board, channel, dt, timestamp, record_id) order
    inner = sorted(range(8), key=lambda i: (hits["board"][i], hits["channel"][i], hits["dt"][i], hits["timestamp"][i]))
    assert [i for i in zeros if i < 8] == inner
    key_order = sorted(range(8), key=lambda i: (hits["dt"][i], hits["timestamp"][i], hits["record_id"][i]))
    assert key_order == list(range(7, -1, -1))  # the reverse of the input order
    assert any(t0 == -2 and t1 == -1 for t0, t1, _ in events)  # int(-2.5), int(-1.5): truncation toward zero
    frac = f0[~np.isnan(f0)]
    assert np.sum(frac != np.floor(frac)) >= 30 and np.sum(frac < 0) >= 7
    own = np.array(U.abs_windows(hits)[0])
    assert np.nanmax(np.abs(f0 - own)) >= 10**9  # fixes far from the row's own timestamp
    hits_i, g0, g1 = U.fixed_windows(False)
    assert np.all(g0[~np.isnan(g0)] == np.floor(g0[~np.isnan(g0)])) and np.all(g1[~np.isnan(g1)] == np.floor(g1[~np.isnan(g1)]))


def test_integral_ties_probe_the_addition_tree():
    sets = U.integral_ties()
    assert {n for n, _, _ in sets} == set(U.TIE_SIZES) and len(sets) >= 250
    want = {}
    for n, label, x in sets:
        xs = [float(v) for v in x]
        want[(n, label)] = np.float32(np.sum(xs))
        assert np.float32(U.pairwise_sum(xs, **U.NUMPY_TREE)).view(np.uint32) == want[(n, label)].view(np.uint32), (n, label)
        assert want[(n, label)] in (np.float32(2.0**30), np.float32(2.0**30 + 128))
    for n in U.TIE_SIZES:
        if n >= 8:
            assert {float(v) for (m, _), v in want.items() if m == n} == {2.0**30, 2.0**30 + 128}, n
    for tree_name, tree in U.WRONG_TREES.items():
        differ = [(n, label) for n, label, x in sets
                  if np.float32(U.pairwise_sum([float(v) for v in x], **tree)) != want[(n, label)]]
        assert differ, f"no integral set tells {tree_name} from numpy's tree"
    # and through the merged rows of the oracle
    hits, clusters = U.clusters_table([x for _, _, x in sets])
    assert len(clusters) > 256
    rows = O.hit_merged_rows(hits, clusters)
    assert model_fields(hits, clusters) == merged_fields(hits, rows)
    np.testing.assert_array_equal(rows["integral"], [want[(n, label)] for n, label, _ in sets])
    loop = model_fields(hits, clusters, U.WRONG_TREES["left_to_right"])
    assert loop != merged_fields(hits, rows)


# ---- (3) every mutant of the restatement is caught by some table -------------------------------------------------------
def _group_mutant_differs(switch):
    for name in U.group_case_names():
        if name.startswith("A-") or name.startswith("D-65537"):
            continue  # (the small tables are enough, and quick)
        case = U.group_case(name)
        for w in case["windows"]:
            if model_events(case, w, **{switch: True})[0] != oracle_events(case, w):
                return name, w
    return None


def _merge_mutant_differs(switch):
    for name in ("C-boundaries", "C-boundaries-above_2p53"):
        case = U.merge_case(name)
        for gap, cap in case["configs"]:
            if U.merge_model(case["hits"], gap, cap, **{switch: True})[0] != O.hit_merge_clusters(case["hits"], gap, cap):
                return name, gap, cap
    return None


@pytest.mark.parametrize("mutant", list(U.MUTANTS))
def test_mutants_of_the_restatement_are_caught(mutant):
    model, switch, _ = U.MUTANTS[mutant]
    found = _group_mutant_differs(switch) if model == "group" else _merge_mutant_differs(switch)
    assert found is not None, f"no table tells {mutant} from the reference"
    if mutant == "neg_zero_first":
        assert found[0] == "E-fractional" or found[0] == "E-integer"
    if mutant == "int_keys_always":
        case = U.group_case(found[0])  # caught on a table that is not integer-exact
        a0 = np.array(U.abs_windows(case["hits"], case["fix0"], case["fix1"])[0])
        assert np.any(a0 != np.floor(a0))
