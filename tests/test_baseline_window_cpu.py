"""Proof, without a GPU, of the cases tests/test_hip_baseline_window.py runs (tests/baseline_window_util.py): the
reference is the oracle's baseline_mean and np.mean over float64, every window group lands on every layout it fits, the
ragged-only windows split the run into NaN and finite baselines, every case has rows to compare (or, all NaN, none), and
the sums of the 32-bit case lie on the sides of 2**31 - 1 they are meant to."""

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import baseline_window_util as U
from tests import test_hip_layout_routes as LR


@pytest.mark.parametrize("name", U.LAYOUTS)
def test_reference_is_the_oracle_and_np_mean(name):
    rec, pool, _want, _filt = LR._case(name)
    uniform = name != "ragged"
    L = U.max_len(name)
    raw = pool[int(rec["wave_offset"][0]):].reshape(LR.N, L) if uniform else None
    for window in U.windows(name):
        s, e = window
        ref = U.reference(rec, pool, window)
        if uniform:
            np.testing.assert_array_equal(ref, O.baseline_mean(raw, s, e), err_msg=f"{name} {window}")
        for i in range(len(rec)):
            o, n = int(rec["wave_offset"][i]), int(rec["event_length"][i])
            w = pool[o : o + n]
            e1 = min(e, n)
            if e1 <= s:
                assert np.isnan(ref[i]), (name, window, i)
            else:
                assert ref[i] == np.mean(w[s:e1].astype(float)), (name, window, i)


@pytest.mark.parametrize("name", U.LAYOUTS)
def test_every_group_on_every_layout_it_fits(name):
    L = U.max_len(name)
    groups = U.window_groups(name)
    want = {"chunk edges", "control", "record end", "empty by clamp"}
    if L >= 32:
        want.add("round edges")
    if name == "ragged":
        want.add("ragged only")
    assert set(groups) == want, (name, sorted(groups))
    # nothing that fits is dropped: the whole chunk-edge group from 29 samples on, the whole round-edge group from 72
    assert len(groups["chunk edges"]) == (7 if L >= 29 else 6), name
    if L >= 32:
        assert L >= 40 and len(groups["round edges"]) == (6 if L >= 72 else 5), name
    assert (24, 72) not in U.windows("L64") and (24, 72) in U.windows("L72")
    for ws in groups.values():
        for s, e in ws:
            assert 0 <= s <= L + 70 and e <= U.I32_MAX, (name, s, e)   # what a GPU test may pass as a window


def test_layouts_and_selectors_of_the_route_table():
    assert set(U.LAYOUTS) <= set(LR.ROUTES)
    assert U.SELECTORS == ("", "no_runs32", "no_pad", "no_span", "no_fast", "sg21_4")
    # L64 takes the streaming kernel for the control window and must fall to span16 for every other one
    assert U.expected_stage("L64", "", U.CONTROL) == LR.RUNS
    assert U.expected_stage("L88", "", U.CONTROL) == LR.RUNS_PAD
    for w in U.windows("L64"):
        if w != U.CONTROL:
            assert U.expected_stage("L64", "", w) == LR.SPAN16, w
            assert U.expected_stage("L88", "", w) == LR.SPAN16_PAD, w
    assert U.expected_stage("L80", "", (5, 29)) == LR.SPAN16
    assert U.expected_stage("L72", "", (5, 29)) == LR.SPAN16_PAD
    assert U.expected_stage("L68", "", (5, 29)) == U.expected_stage("ragged", "", (5, 29)) == LR.MASK


def test_ragged_only_windows_give_nan_and_finite():
    rec, pool, _want, _filt = LR._case("ragged")
    length = rec["event_length"]
    assert length.min() == 40 and length.max() == 64          # the lengths drawn with the layout's fixed seed
    assert U.window_groups("ragged")["ragged only"] == [(44, 52), (39, 41), (40, 42), (63, 64)]
    for window in U.window_groups("ragged")["ragged only"]:
        ref = U.reference(rec, pool, window)
        nan = np.isnan(ref)
        np.testing.assert_array_equal(nan, length <= window[0], err_msg=str(window))
        short = (~nan) & (length < window[1])                   # a mean of fewer samples than the window asks for
        if window == (39, 41):  # starts inside the shortest record: no NaN, a one-sample mean next to two-sample ones
            assert not nan.any() and short.any() and not short.all(), window
            continue
        assert nan.any() and (~nan).any(), window
        if window != (63, 64):
            assert short.any(), window


@pytest.mark.parametrize("name", U.LAYOUTS)
def test_cases_have_rows_to_compare(name):
    for selector_plan in ((11, 2), U.SG_SLOW):
        for window in U.windows(name):
            rec_ref, _pool, want = U.case(name, window, selector_plan)
            nan = np.isnan(rec_ref["baseline"])
            what = f"{name} {window} SG{selector_plan}: {len(want)} oracle hits"
            if not nan.any():
                assert len(want) > 100, what
            if nan.all():
                assert len(want) == 0, what
            assert not np.isin(want["record_id"], rec_ref["record_id"][nan]).any(), what
    for window in U.window_groups(name)["empty by clamp"]:
        assert np.isnan(U.case(name, window)[0]["baseline"]).all(), (name, window)


@pytest.mark.parametrize("name", list(U.BIG_LAYOUTS))
def test_the_32_bit_case(name):
    L = U.BIG_LAYOUTS[name]
    fits, edge, whole = U.big_windows(name)
    assert (fits, edge, whole) == ((0, 32_768), (0, 32_769), (0, L))
    assert L % 16 == (0 if name == "L32784" else 6) and L % 32 != 0 and U.BIG_R == 66
    for window in (fits, edge, whole):
        rec_ref, pool, want = U.big_case(name, window)
        assert pool.nbytes == U.BIG_R * L * 2 < 4.4e6
        w = pool.reshape(U.BIG_R, L)
        sums = w[:, : window[1]].sum(axis=1, dtype=np.int64)
        np.testing.assert_array_equal(rec_ref["baseline"], sums / float(window[1]))
        np.testing.assert_array_equal(rec_ref["baseline"], O.baseline_mean(w, *window))
        assert len(want) >= U.BIG_R, (name, window, len(want))    # every record's dips are hits
        if window == fits:
            assert sums.max() <= U.I32_MAX, (name, window)
            continue
        assert sums.min() > U.I32_MAX, (name, window)
        if window == edge:
            assert (sums == 2_147_516_415).all(), (name, window)
        # what a sum wrapped to 32 bits would give: further from the reference than the threshold, so a regression
        # cannot hide in an unchanged hit table
        wrapped = (sums + 2**31) % 2**32 - 2**31
        assert (np.abs(wrapped / float(window[1]) - rec_ref["baseline"]) > U.THRESHOLD).all(), (name, window)
