"""HipRecordsView without a GPU: the numpy restatement the GPU tests compare against reproduces the reference's recorded
arrays byte for byte (tests/golden/vx2730csv_records_view.npz), and the host code of HipRecordsView itself -- id lookup, window
clamping, pad_to / baseline / unknown-id / dtype errors, query_time_window, residency -- runs against a stand-in session
that records its calls and gathers with numpy."""

import numpy as np
import pytest

from tests import records_view_util as U
from waveformanalysis_amd import device as D
from waveformanalysis_amd.dtypes import RECORDS_DTYPE
from waveformanalysis_amd.records_view import HipRecordsView, hip_records_view

RECORDS, POOLS, CALLS, ARRAYS = U.load()


class StubSession(D.DeviceSession):
    """DeviceSession with the C calls replaced.  Residency tags are the real ones; view_gather is a per-row numpy loop
    over what was 'uploaded' (copies, so serving another pool would show)."""

    def __init__(self):  # no wfa_ctx
        self._h = None
        self._res_pool = self._res_filtered = self._res_records = None
        self.uploads = self.record_uploads = self.n_samples = self.n_records = 0
        self.dev = {"u16": None, "f32": None}
        self.dev_records = None
        self.gathers = []

    def upload_pool(self, wave_pool):
        self.forget_resident()
        self.uploads += 1
        self.dev = {"u16": None, "f32": None}
        self.dev["f32" if wave_pool.dtype == np.float32 else "u16"] = np.array(wave_pool, copy=True)
        self.dev_records = None
        self.n_samples = wave_pool.size

    def upload_filtered_pool(self, pool_f32):
        assert pool_f32.size == self.n_samples
        self._drop_f32_tags()
        self._res_records = None
        self.uploads += 1
        self.dev["f32"] = np.array(pool_f32, copy=True)

    def upload_records(self, records, thresholds=10.0, polarity=None):
        self._res_records = None
        self._check_unique_ids(np.ascontiguousarray(records["record_id"], dtype=np.int64))
        self.record_uploads += 1
        self.dev_records = records.copy()
        self.n_records = len(records)

    def view_gather(self, rec_index, *, mode, source, out_dtype, pad_len, sample_start=0, sample_end=None, mask=False,
                    baseline_override=None, out=None, batch_bytes=0):
        self.gathers.append(dict(n=len(rec_index), mode=mode, source=source, dtype=np.dtype(out_dtype), pad_len=pad_len,
                                 sample_start=sample_start, sample_end=sample_end, mask=mask))
        rec, pool = self.dev_records, self.dev[source]
        assert rec is not None and pool is not None and pool.dtype == (np.uint16 if source == "u16" else np.float32)
        values = np.zeros((len(rec_index), pad_len), dtype=out_dtype)
        valid = np.zeros((len(rec_index), pad_len), dtype=np.uint8)
        positive = D.polarity_codes(rec) == D._lib.POL_POSITIVE
        for k, r in enumerate(rec_index):
            assert 0 <= r < len(rec)
            n = int(rec["event_length"][r])
            end = n if sample_end is None else min(max(sample_end, 0), n)
            start = min(max(sample_start, 0), end)
            x = pool[rec["wave_offset"][r] + start:rec["wave_offset"][r] + end].astype(out_dtype)
            if mode != "waves":
                b = rec["baseline"][r] if baseline_override is None else baseline_override[k]
                x = x - np.asarray(b, dtype=out_dtype)
                if mode == "signals" and positive[r]:
                    x = -x
            assert len(x) <= pad_len
            values[k, :len(x)] = x
            valid[k, :len(x)] = 1
        return (values, valid) if mask else values


def _view(pool="u16", sess=None):
    sess = sess or StubSession()
    return HipRecordsView(RECORDS, POOLS[pool], session=sess), sess


# ---- the fixture pins the numpy helper ---------------------------------------------------------------------------------
def test_fixture_holds_the_cases_it_is_meant_to():
    lengths = set(RECORDS["event_length"].tolist())
    assert {0, 1, 7, 8, 9} <= lengths and max(lengths) > 1024 and len(RECORDS) == 40
    assert {int(o) & 1 for o in RECORDS["wave_offset"]} == {0, 1}
    assert int(np.sum(RECORDS["event_length"])) < len(POOLS["u16"])  # gaps
    rid = RECORDS["record_id"]
    assert np.any(np.diff(rid) < 0) and not np.array_equal(np.sort(rid), np.arange(rid.min(), rid.min() + len(rid)))
    assert set(RECORDS["polarity"].tolist()) == {"positive", "negative", "unknown"}
    b = RECORDS["baseline"]
    assert np.sum(b.astype(np.float32).astype(np.float64) != b) >= len(b) - 1
    assert POOLS["u16"].min() == 0 and POOLS["u16"].max() == 65535
    assert len(np.unique(RECORDS["timestamp"])) < len(RECORDS) and np.all(np.diff(RECORDS["timestamp"]) >= 0)
    minus_zero = [k for k, c in enumerate(CALLS) if c["method"] == "signals" and c["pool"] == "u16"
                  and np.any((ARRAYS[f"c{k}_values"] == 0) & np.signbit(ARRAYS[f"c{k}_values"]))]
    assert minus_zero
    assert {c["method"] for c in CALLS} == {"waves", "signals", "query_time_window"}
    assert {c["pool"] for c in CALLS} == {"u16", "f32"}


@pytest.mark.parametrize("k", range(len(CALLS)))
def test_numpy_restatement_matches_the_reference(k):
    call = CALLS[k]
    view = U.NumpyRecordsView(RECORDS, POOLS[call["pool"]])
    U.assert_same_bytes(U.run_call(view, call), U.expected(call, k, ARRAYS), f"call {k} {call}")


# ---- HipRecordsView: host code over the stand-in session ------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CALLS)))
def test_view_host_code_matches_the_reference(k):
    call = CALLS[k]
    view, _sess = _view(call["pool"])
    U.assert_same_bytes(U.run_call(view, call), U.expected(call, k, ARRAYS), f"call {k} {call}")


def test_len_and_constructor_checks():
    view, _ = _view()
    assert len(view) == len(RECORDS)
    with pytest.raises(ValueError, match="structured array"):
        HipRecordsView(np.zeros(3), POOLS["u16"])
    with pytest.raises(ValueError, match=r"missing required fields: \['baseline'\]"):
        HipRecordsView(RECORDS[["record_id", "wave_offset", "event_length", "timestamp"]], POOLS["u16"])
    for field, value, text in (("wave_offset", -1, "negative wave_offset"), ("event_length", -1, "negative event_length"),
                               ("wave_offset", len(POOLS["u16"]), "outside wave_pool bounds")):
        bad = RECORDS.copy()
        bad[field][5] = value
        with pytest.raises(ValueError, match=text):
            HipRecordsView(bad, POOLS["u16"])
    with pytest.raises(ValueError, match="uint16 or float32"):
        HipRecordsView(RECORDS, POOLS["u16"].astype(np.int32))
    empty = HipRecordsView(RECORDS[:0], POOLS["u16"][:0], session=StubSession())
    assert len(empty) == 0 and empty.waves([]).shape == (0, 0)


def test_id_lookup_is_by_value_and_names_the_first_missing_id():
    view, sess = _view()
    ids = RECORDS["record_id"]
    got = view.waves([int(ids[7]), int(ids[3]), int(ids[7])], pad_to=40)
    assert sess.gathers[-1]["n"] == 3 and got.shape == (3, 40)
    off, n = int(RECORDS["wave_offset"][3]), int(RECORDS["event_length"][3])
    assert np.array_equal(got[1, :n], POOLS["u16"][off:off + n]) and np.array_equal(got[0], got[2])
    np.testing.assert_array_equal(view._resolve_record_indices(ids[::-1]), np.arange(len(ids))[::-1])
    np.testing.assert_array_equal(view._resolve_record_indices(iter([int(ids[4])])), [4])
    calls = len(sess.gathers)
    for bad, first in (([int(ids[0]), 5, int(ids[1]), 6], 5), ([10**12, -3], 10**12), (np.array([-3, 5]), -3)):
        with pytest.raises(KeyError, match=f"Unknown record_id: {first}'$"):
            view.signals(bad)
    with pytest.raises(KeyError, match="Unknown record_id: 17'$"):
        view.waves(17)
    assert len(sess.gathers) == calls


def test_window_clamping_and_pad_len_reach_the_session():
    view, sess = _view()
    ids = [int(i) for i in RECORDS["record_id"][[6, 9, 13]]]   # lengths 16, 64, 3
    for start, end, pad in ((0, None, 64), (-4, None, 64), (5, None, 59), (70, None, 0), (2, 6, 4), (0, 0, 0), (9, 3, 0),
                            (60, 1000, 4), (0, -2, 0)):
        got, m = view.signals(ids, mask=True, sample_start=start, sample_end=end)
        assert got.shape == m.shape == (3, pad) and m.dtype == np.bool_, (start, end)
        assert sess.gathers[-1]["pad_len"] == pad
    assert view.waves(ids[2], sample_start=1).shape == (2,) and sess.gathers[-1]["pad_len"] == 2
    assert view.waves(ids[2], sample_start=5).shape == (0,)


def test_pad_to_baseline_and_dtype_errors():
    view, sess = _view()
    ids = [int(i) for i in RECORDS["record_id"][[6, 9]]]
    with pytest.raises(ValueError, match=r"^pad_to must be >= 0$"):
        view.waves(ids, pad_to=-1)
    with pytest.raises(ValueError, match=r"^pad_to \(63\) < max length \(64\)$"):
        view.signals(ids, pad_to=63)
    assert view.signals(ids, pad_to=63, sample_start=1).shape == (2, 63)
    with pytest.raises(ValueError, match="^baseline override is only supported for scalar signal access$"):
        view.signals(ids, baseline=3.0)
    n = len(sess.gathers)
    for call in (lambda: view.waves(ids, dtype=np.int32), lambda: view.signals(ids, dtype=np.float16),
                 lambda: view.waves(ids, baseline_correct=True, dtype=np.uint16), lambda: view.signals(ids[0], dtype=np.uint16),
                 lambda: view.waves(ids[0], dtype=np.int16)):
        with pytest.raises(ValueError, match="unsupported dtype"):
            call()
    f32_view, _ = _view("f32")
    with pytest.raises(ValueError, match="unsupported dtype uint16"):
        f32_view.waves(ids, dtype=np.uint16)
    assert len(sess.gathers) == n
    # defaults: the pool's dtype for plain waves, float32 otherwise
    assert view.waves(ids).dtype == np.uint16 and f32_view.waves(ids).dtype == np.float32
    assert view.waves(ids, baseline_correct=True).dtype == np.float32 and view.signals(ids).dtype == np.float32
    assert view.signals(ids, dtype="float64").dtype == np.float64


def test_empty_id_list_touches_no_device():
    view, sess = _view()
    for got in (view.waves([]), view.signals(np.zeros(0, dtype=np.int64))):
        assert got.shape == (0, 0) and got.dtype == np.float32
    values, m = view.waves([], mask=True, dtype=np.float64)
    assert values.shape == m.shape == (0, 0) and values.dtype == np.float64 and m.dtype == np.bool_
    assert sess.uploads == sess.record_uploads == len(sess.gathers) == 0


def test_query_time_window_is_host_code():
    view, sess = _view()
    ts = RECORDS["timestamp"]
    assert len(view.query_time_window()) == len(RECORDS)
    got = view.query_time_window(int(ts[10]), int(ts[12]))
    assert np.array_equal(got["timestamp"], ts[(ts >= ts[10]) & (ts <= ts[12])]) and np.shares_memory(got, RECORDS)
    assert len(view.query_time_window(int(ts[-1]) + 1)) == 0 and len(view.query_time_window(None, int(ts[0]) - 1)) == 0
    assert sess.uploads == sess.record_uploads == 0


def test_second_call_uploads_nothing_and_a_resident_pool_is_not_uploaded():
    sess = StubSession()
    sess.ensure_pool(POOLS["u16"])   # what a records-route plugin leaves behind
    assert sess.uploads == 1
    view, _ = _view(sess=sess)
    ids = [int(i) for i in RECORDS["record_id"][:5]]
    view.waves(ids)
    assert (sess.uploads, sess.record_uploads) == (1, 1)
    view.signals(ids[::-1], mask=True)
    view.waves(ids[0])
    assert (sess.uploads, sess.record_uploads, len(sess.gathers)) == (1, 1, 3)
    # a fresh session: one pool upload, one records upload, then nothing
    view2, sess2 = _view()
    for _ in range(3):
        view2.signals(ids)
    assert (sess2.uploads, sess2.record_uploads) == (1, 1)


def test_replaced_pool_or_records_are_uploaded_again():
    view, sess = _view()
    ids = [int(i) for i in RECORDS["record_id"][:5]]
    want = view.signals(ids)
    other = (POOLS["u16"] // 2).astype(np.uint16)
    sess.ensure_pool(other)                       # another caller replaced the pool
    assert np.array_equal(view.signals(ids), want) and (sess.uploads, sess.record_uploads) == (3, 2)
    sess.upload_records(RECORDS[::-1].copy())     # another caller replaced the records table
    assert np.array_equal(view.signals(ids), want) and (sess.uploads, sess.record_uploads) == (3, 4)
    twin, _ = _view(sess=sess)                    # two views on one session take turns
    assert np.array_equal(twin.signals(ids), want) and np.array_equal(view.signals(ids), want)
    assert (sess.uploads, sess.record_uploads) == (3, 6)


def test_float32_pool_goes_to_the_float32_pool():
    sess = StubSession()
    sess.ensure_pool(POOLS["u16"])
    sess.dev["f32"] = POOLS["f32"].copy()         # what wave_pool_filtered leaves behind: the filter's output on the
    sess.note_filtered(POOLS["f32"])              # device, tagged with the array it was downloaded into
    view, _ = _view("f32", sess)
    ids = [int(i) for i in RECORDS["record_id"][:5]]
    got = view.waves(ids)
    assert sess.uploads == 1 and sess.gathers[-1]["source"] == "f32" and got.dtype == np.float32
    assert sess.holds_pool(POOLS["u16"])          # the raw pool stays
    # the twin of a resident raw pool is uploaded as the float32 pool; a float32 pool of another size replaces the pool
    sess2 = StubSession()
    sess2.ensure_pool(POOLS["u16"])
    view2, _ = _view("f32", sess2)
    view2.signals(ids)
    view2.signals(ids)
    assert sess2.uploads == 2 and sess2.holds_filtered(POOLS["f32"]) and sess2.holds_pool(POOLS["u16"])
    sess3 = StubSession()
    sess3.ensure_pool(np.zeros(7, dtype=np.uint16))
    view3, _ = _view("f32", sess3)
    view3.signals(ids)
    view3.signals(ids)
    assert sess3.uploads == 2 and sess3.holds_pool(POOLS["f32"]) and sess3.record_uploads == 1


def test_factory_and_package_export():
    import waveformanalysis_amd as pkg

    assert pkg.HipRecordsView is HipRecordsView and pkg.hip_records_view is hip_records_view

    class Pool:
        def __init__(self):
            self.s = StubSession()

        def session(self):
            return self.s

    class Source:
        def __init__(self, data):
            self.data, self.asked, self.wfa_device_pool = data, [], Pool()

        def get_data(self, run_id, name):
            self.asked.append((run_id, name))
            return self.data.get(name)

    src = Source({"records": RECORDS, "wave_pool": POOLS["u16"], "wave_pool_filtered": POOLS["f32"]})
    view = hip_records_view(src, "run_001")
    assert isinstance(view, HipRecordsView) and src.asked == [("run_001", "records"), ("run_001", "wave_pool")]
    rid = int(RECORDS["record_id"][4])
    assert np.array_equal(view.waves(rid), U.NumpyRecordsView(RECORDS, POOLS["u16"]).waves(rid))
    assert src.wfa_device_pool.s.uploads == 1     # the context's pool, not the default one
    filtered = hip_records_view(src, "run_001", wave_pool_name="wave_pool_filtered")
    assert filtered.wave_pool is POOLS["f32"]
    with pytest.raises(ValueError, match="^records_view requires formal 'wave_pool_x' plugin output$"):
        hip_records_view(src, "run_001", wave_pool_name="wave_pool_x")
    with pytest.raises(ValueError, match="^records_view requires formal 'recs' plugin output$"):
        hip_records_view(src, "run_001", records_name="recs")


def test_duplicate_ids_follow_upload_records():
    rec = np.zeros(2, dtype=RECORDS_DTYPE)
    rec["record_id"] = [10, 10]
    rec["wave_offset"] = [0, 1]
    rec["event_length"] = 1
    view = HipRecordsView(rec, np.array([1, 2], dtype=np.uint16), session=StubSession())
    with pytest.raises(ValueError, match="record_id must be unique, got duplicate 10"):
        view.waves(10)
