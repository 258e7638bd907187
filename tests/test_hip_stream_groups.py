"""HipThresholdHitStream under per-channel settings on the GPU (channel_config, filter_source="wave_pool_filtered"), and
the calls below it: wfa_sg_plan_store, wfa_sosfiltfilt_group, wfa_hits_enqueue_groups, wfa_hits_pending.

The stream must give the rows of hit_threshold under the same Context whatever the chunk size: the reference's rows on
the fixture runs of tests/golden/c5_fused_groups.npz, the run-wide oracle on the runs of tests/stream_groups_util.py.
The queued grouped call must give, byte for byte, the host merge of the groups' single passes run one after another
(tests/fused_groups_util.run_groups, host_merge)."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import fused_groups_util as F
from tests import golden_util as G
from tests import stream_groups_util as U
from tests import stream_hits_util as S
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DevicePool, DeviceSession, device_count
from waveformanalysis_amd.dtypes import THRESHOLD_HIT_DTYPE
from waveformanalysis_amd.filter_engine import design_bw
from waveformanalysis_amd.streaming import HipThresholdHitStream, records_to_chunks

pytestmark = pytest.mark.gpu
FLOAT_RTOL = 1e-6          # the bar of tests/test_hip_parity.py, test_hip_stream_hits.py and test_hip_fused_groups.py
FIXTURE_CHUNKS = (24, 40, 64, 160)


@pytest.fixture(scope="module")
def dp():
    pool = DevicePool([0])
    yield pool
    pool.close()


@pytest.fixture(scope="module")
def sess():
    with DeviceSession(0) as s:
        yield s


def _drivers(plugin, chunks, ctx, c):
    yield "compute serial", list(plugin.compute(ctx, "run", streaming_config={"chunk_size": c, "parallel": False}))
    yield "compute parallel", list(plugin.compute(ctx, "run", streaming_config={"chunk_size": c, "max_workers": 3}))
    for w in (1, 2, 8):
        yield f"run_chunks workers={w}", plugin.run_chunks(chunks, ctx, "run", max_workers=w)


def _rows(outs):
    return np.concatenate([o.data for o in outs]) if outs else np.zeros(0, dtype=THRESHOLD_HIT_DTYPE)


# ---- 1. the stream against the reference's rows -------------------------------------------------------------------------
@pytest.mark.parametrize("tag", F.RUNS)
def test_stream_gives_the_reference_rows_on_the_fixture(tag, dp):
    run = F.load_run(tag)
    ctx = U.context(run["records"], run["wave_pool"])
    static = ctx.get_data("run", "hit_threshold")
    G.assert_struct_equal(static, run["hits"], float_rtol=FLOAT_RTOL, what=f"run {tag}: hit_threshold vs reference")
    plugin = HipThresholdHitStream(device_pool=dp)
    for c in FIXTURE_CHUNKS:
        chunks = records_to_chunks(run["records"], c, "run")
        first = None
        for what, outs in _drivers(plugin, chunks, ctx, c):
            got = _rows(outs)
            print(f"run {tag} c={c} {what}: {len(got)} rows (reference {len(run['hits'])}, uniform {len(run['hits_uniform'])})")
            G.assert_struct_equal(got, run["hits"], float_rtol=FLOAT_RTOL, what=f"run {tag} c={c} {what} vs reference")
            G.assert_struct_equal(got, static, float_rtol=FLOAT_RTOL, what=f"run {tag} c={c} {what} vs hit_threshold")
            first = got if first is None else first
            assert got.tobytes() == first.tobytes(), f"run {tag} c={c} {what}: bytes differ from another driver's"
            assert len(outs) == len(chunks)


# ---- 2. the stream against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.RUN_NAMES)
def test_stream_gives_the_run_wide_oracle(name, dp):
    run = U.run(name)
    want = U.want(name)
    ctx = U.context(run.records, run.pool)
    plugin = HipThresholdHitStream(device_pool=dp)
    for c in run.chunk_sizes:
        chunks = run.chunks(c)
        first = None
        for what, outs in _drivers(plugin, chunks, ctx, c):
            got = S.check_bookkeeping(run, chunks, outs, want, f"{name} c={c} {what}")
            print(f"{name} c={c} {what}: {len(got)} rows, oracle {len(want)}")
            G.assert_struct_equal(got, want, float_rtol=FLOAT_RTOL, what=f"{name} c={c} {what} vs oracle")
            for k, (ch, o) in enumerate(zip(chunks, outs)):     # every chunk complete by itself
                assert len(o.data) == int(np.isin(want["record_id"], ch.data["record_id"]).sum()), (name, what, k)
            first = got if first is None else first
            assert got.tobytes() == first.tobytes(), f"{name} c={c} {what}: bytes differ from another driver's"


def test_sg_only_configuration_and_the_exact_redo(dp):
    """Every group on a speculative route; on `sparse` the per-group counts jump between chunks, so a bound sized by the
    previous chunk is exceeded and wfa_hits_wait redoes the grouped pass the exact way."""
    for name in ("sparse", "mixed"):
        run = U.run(name)
        want = U.want(name, "sg_only")
        ctx = U.context(run.records, run.pool, "sg_only")
        plugin = HipThresholdHitStream(device_pool=dp)
        chunks = run.chunks(run.chunk_sizes[0])
        for w in (1, 2):
            outs = plugin.run_chunks(chunks, ctx, "run", max_workers=w)
            got = S.check_bookkeeping(run, chunks, outs, want, f"{name} sg_only workers={w}")
            G.assert_struct_equal(got, want, float_rtol=FLOAT_RTOL, what=f"{name} sg_only workers={w}")


# ---- 3. the C call alone ------------------------------------------------------------------------------------------------
def _queued(s, rec, thr, keys, gor, option=None):
    """upload + the queued grouped pass on a session that holds the pool -> (rows, pending right after the call)."""
    s.upload_records(rec, thr)
    F.stage_groups(s, keys, gor)
    pending = s.hits_pending()
    n = s.hits_wait()
    assert not s.hits_pending()
    return s._fill_hits(n), pending


def _synchronous(s, rec, thr, keys, gor):
    """The groups' single passes, each waited for and downloaded, merged on the host -> (table, the passes' rows).
    run_groups ends with a queued grouped call of its own -- on a context that has not seen these groups, the cold one --
    whose table must already be that merge."""
    parts, n = F.run_groups(s, rec, thr, [(key, gor == g) for g, key in enumerate(keys)])
    want = F.host_merge(rec, parts)
    assert s._fill_hits(n).tobytes() == want.tobytes()
    return want, parts


def _channel_groups(rec):
    return rec["channel"].astype(np.int32)


CASES = ["plain", "empty_group", "unowned", "one_group", "unordered_ids", "no_speculate"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tag", F.RUNS)
def test_queued_call_equals_the_synchronous_sequence(sess, tag, case):
    run = F.load_run(tag)
    rec, pool = run["records"], run["wave_pool"]
    keys, gor, thr = list(F.KEYS), _channel_groups(rec), F.thresholds_of(rec)
    if case == "empty_group":      # a fifth group nobody belongs to, in the middle
        keys = keys[:2] + [("SG", 5, 2)] + keys[2:]
        gor = np.where(gor >= 2, gor + 1, gor).astype(np.int32)
    elif case == "unowned":        # channel 2 belongs to no pass
        keys = keys[:2] + keys[3:]
        gor = np.where(gor == 2, -1, np.where(gor == 3, 2, gor)).astype(np.int32)
    elif case == "one_group":
        keys, gor = [("SG", 7, 3)], np.zeros(len(rec), dtype=np.int32)
    elif case == "unordered_ids":
        rec = rec.copy()
        rec["record_id"] = np.random.default_rng(5).permutation(len(rec)) * 7 + 3
    sess.upload_pool(pool)
    want, parts = _synchronous(sess, rec, thr, keys, gor)
    assert len(want) > 100 and sum(len(p) > 0 for p in parts) == len(keys) - (case == "empty_group")
    if case == "plain":
        G.assert_struct_equal(want, run["hits"], float_rtol=FLOAT_RTOL, what=f"run {tag}: synchronous sequence vs reference")
    if case == "no_speculate":
        sess.set_option("no_speculate", True)
    try:
        sess.upload_pool(pool)
        for call in range(3):      # warm calls (the cold one ran inside _synchronous): every group's previous count is known
            got, pending = _queued(sess, rec, thr, keys, gor)
            print(f"run {tag} {case} call {call}: {len(got)} rows, pending after the call: {pending}")
            assert got.tobytes() == want.tobytes(), (tag, case, call)
            if case == "no_speculate":
                assert not pending
    finally:
        sess.set_option("no_speculate", False)
    # the uploaded threshold column is intact: a plain pass gives the rows of the records' own thresholds
    sess.set_sg_plan(11, 2)
    plain = sess.threshold_hits(_lib.SRC_SG_FUSED)
    sess.upload_records(rec, thr)
    assert plain.tobytes() == sess.threshold_hits(_lib.SRC_SG_FUSED).tobytes() and len(plain) > 100


@pytest.mark.parametrize("tag", ["a", "c"])
def test_resident_stages_read_the_queued_merged_table(sess, tag):
    run = F.load_run(tag)
    rec = run["records"]
    sess.upload_pool(run["wave_pool"])
    for _call in range(2):
        rows, _pending = _queued(sess, rec, F.thresholds_of(rec), list(F.KEYS), _channel_groups(rec))
    n = len(rows)
    assert n == len(run["hits"])
    sess.hit_rows_source("hits")
    order, offset = sess.hit_merge_clusters_resident(n, 200.0, 4000.0)
    want_order, want_offset = sess.hit_merge_clusters(rows["timestamp"], rows["position"], rows["edge_start"],
                                                      rows["edge_end"], rows["dt"], rows["board"], rows["channel"], 200.0, 4000.0)
    np.testing.assert_array_equal(order, want_order)
    np.testing.assert_array_equal(offset, want_offset)
    assert 1 < len(offset) - 1 < n
    got = sess.group_hit_windows_resident(n, 1000.0)
    want = sess.group_hit_windows(rows["timestamp"], rows["position"], rows["edge_start"], rows["edge_end"], rows["dt"],
                                  rows["board"], rows["channel"], rows["record_id"], 1000.0)
    for name in want:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    # the stash is scratch: 64 bytes per stashed row
    before = sess.scratch_bytes()
    assert before >= 64 * n
    assert sess.release_scratch() == before and sess.scratch_bytes() == 0
    again, _pending = _queued(sess, rec, F.thresholds_of(rec), list(F.KEYS), _channel_groups(rec))
    assert again.tobytes() == rows.tobytes()


# ---- 4. queued means queued ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", F.RUNS)
def test_warm_sg_only_call_returns_with_the_pass_pending(tag):
    run = F.load_run(tag)
    rec, pool = run["records"], run["wave_pool"]
    keys, gor, thr = U.KEYS["sg_only"], _channel_groups(rec), F.thresholds_of(rec)
    with DeviceSession(0) as s:
        s.upload_pool(pool)
        want, _parts = _synchronous(s, rec, thr, keys, gor)
        s.upload_pool(pool)
        first, _pending = _queued(s, rec, thr, keys, gor)
        second, pending = _queued(s, rec, thr, keys, gor)
        print(f"run {tag}: pending after the warm call: {pending}")
        if tag in ("a", "b"):      # uniform records: every group on the streaming or the bitmap route
            assert pending
        assert first.tobytes() == want.tobytes() == second.tobytes() and len(want) > 300


def test_ring_keeps_its_order_under_the_sg_only_configuration():
    run = U.run("mixed")
    ctx = U.context(run.records, run.pool, "sg_only")
    chunks = run.chunks(100)
    want = U.want("mixed", "sg_only")
    pool = DevicePool([0])
    try:
        plugin = HipThresholdHitStream(device_pool=pool)
        for _call in range(3):
            timeline = []
            outs = plugin.run_chunks(chunks, ctx, "run", max_workers=3, timeline=timeline)
            assert [t[0] for t in timeline] == list(range(len(chunks)))
            # chunk k + 1 is staged and queued before anybody waits for chunk k
            for (k, _b, queued, collected), (_k1, begin1, queued1, _c1) in zip(timeline, timeline[1:]):
                assert queued <= begin1 <= queued1 <= collected, (k, timeline)
            G.assert_struct_equal(_rows(outs), want, float_rtol=FLOAT_RTOL, what="mixed ring, sg_only")
            assert pool.live_sessions == 2
    finally:
        pool.close()


# ---- 5. every visible device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "missing"])
def test_ring_over_every_visible_device(name, dp):
    n = device_count()
    if n < 2:
        pytest.skip("1 device visible: the every-device ring needs two or more")
    run = U.run(name)
    ctx = U.context(run.records, run.pool)
    chunks = run.chunks(run.chunk_sizes[0])
    one = _rows(HipThresholdHitStream(device_pool=dp).run_chunks(chunks, ctx, "run", max_workers=2))
    pool = DevicePool(list(range(n)))
    try:
        for w in (2, 8):
            got = _rows(HipThresholdHitStream(device_pool=pool).run_chunks(chunks, ctx, "run", max_workers=w))
            assert got.tobytes() == one.tobytes() and len(got) == len(U.want(name))
    finally:
        pool.close()


# ---- 6. error contract ----------------------------------------------------------------------------------------------------
def test_error_codes_of_the_new_calls():
    run = F.load_run("a")
    rec, pool = run["records"], run["wave_pool"]
    sos, zi, padlen = design_bw(*F.KEYS[3][1:])
    sos, zi = np.ascontiguousarray(sos), np.ascontiguousarray(zi)
    with DeviceSession(0) as s:
        lib, h = s._lib, s._h
        gor = np.zeros(len(rec), dtype=np.int32)
        one = (C.c_int32 * 2)(_lib.SRC_SG_FUSED, 0)

        def enqueue(n_groups, groups, column, max_len=0):
            return lib.wfa_hits_enqueue_groups(h, n_groups, groups, column.ctypes.data, 0, 0, 2, 2, max_len)

        def bw(column, group=0):
            return lib.wfa_sosfiltfilt_group(h, len(sos), sos.ctypes.data, zi.ctypes.data, padlen, column.ctypes.data, group)

        pending = C.c_int(-1)
        assert lib.wfa_hits_pending(h, C.byref(pending)) == 0 and pending.value == 0
        assert lib.wfa_hits_pending(h, None) == _lib.WFA_E_INVALID
        assert enqueue(1, one, gor) == _lib.WFA_E_STATE           # no records
        assert bw(gor) == _lib.WFA_E_STATE
        s.upload_pool(pool)
        assert enqueue(1, one, gor) == _lib.WFA_E_STATE           # a pool, still no records
        s.upload_records(rec, 10.0)
        assert enqueue(0, one, gor) == _lib.WFA_E_INVALID and enqueue(_lib.MAX_HIT_GROUPS + 1, one, gor) == _lib.WFA_E_INVALID
        assert enqueue(1, one, gor) == _lib.WFA_E_STATE           # slot 0 holds no plan
        assert "wfa_sg_plan_store" in _lib.last_error()
        with pytest.raises(ValueError, match="plan slot"):
            s.store_sg_plan(_lib.MAX_HIT_GROUPS, 11, 2)
        with pytest.raises(ValueError, match="plan slot"):
            s.store_sg_plan(-1, 11, 2)
        s.store_sg_plan(0, 11, 2)
        assert enqueue(1, (C.c_int32 * 2)(_lib.SRC_SG_FUSED, _lib.MAX_HIT_GROUPS), gor) == _lib.WFA_E_INVALID
        assert enqueue(1, (C.c_int32 * 2)(_lib.SRC_RAW, 0), gor) == _lib.WFA_E_INVALID
        assert enqueue(1, (C.c_int32 * 2)(_lib.SRC_F32, 0), gor) == _lib.WFA_E_STATE    # no float32 pool, no filter call
        bad = gor.copy()
        bad[7] = 1
        assert enqueue(1, one, bad) == _lib.WFA_E_INVALID and "group_of_record[7]" in _lib.last_error()
        bad[7] = -2
        assert enqueue(1, one, bad) == _lib.WFA_E_INVALID
        assert enqueue(1, one, gor, max_len=int(rec["event_length"].max()) - 1) == _lib.WFA_E_INVALID
        assert lib.wfa_sosfiltfilt_group(h, 0, sos.ctypes.data, zi.ctypes.data, padlen, gor.ctypes.data, 0) == _lib.WFA_E_INVALID
        assert lib.wfa_sosfiltfilt_group(h, len(sos), None, zi.ctypes.data, padlen, gor.ctypes.data, 0) == _lib.WFA_E_INVALID
        with pytest.raises(ValueError, match="one group index per uploaded record"):
            s.hits_enqueue_groups([(_lib.SRC_SG_FUSED, 0)], gor[:-1])
        # nothing above left a pass behind; the calls work once their conditions hold
        assert lib.wfa_hits_pending(h, C.byref(pending)) == 0 and pending.value == 0
        assert bw(gor) == 0
        assert enqueue(1, (C.c_int32 * 2)(_lib.SRC_F32, 0), gor) == 0
        assert s.hits_wait() > 100
        assert enqueue(1, one, gor) == 0
        n = s.hits_wait()
        s.set_sg_plan(11, 2)
        assert n == s.threshold_hits(_lib.SRC_SG_FUSED, download=False) and n > 100


# ---- 7. a bound that does not hold ------------------------------------------------------------------------------------------
def test_exceeded_bound_is_redone_exactly():
    """A warm context whose groups found nothing sizes every group's launch for 4096 rows; the next call finds about
    6000 rows per group.  The call still returns with the pass pending, wfa_hits_wait sees the bounds exceeded and redoes
    the grouped pass the exact way: the host merge of the groups' single passes, byte for byte."""
    rec, pool = U.exceeding_run()
    n = len(rec)
    keys, gor, thr = U.KEYS["sg_only"], _channel_groups(rec), F.thresholds_of(rec)
    with DeviceSession(0) as s:
        s.upload_pool(pool)
        want, parts = _synchronous(s, rec, thr, keys, gor)
        assert all(len(p) > 4096 + 4096 // 8 for p in parts), [len(p) for p in parts]
        s.upload_pool(pool)
        for _call in range(2):
            nothing, _pending = _queued(s, rec, np.full(n, 1e9), keys, gor)
            assert len(nothing) == 0
        got, pending = _queued(s, rec, thr, keys, gor)
        assert pending and got.tobytes() == want.tobytes()
        got, pending = _queued(s, rec, thr, keys, gor)      # and the redo left every group's count behind: this one stands
        assert pending and got.tobytes() == want.tobytes()
