"""Records stream on the GPU: the chunks of HipRecordsStream against the static builder, the fixture made by the
reference, and the CPU model of tests/records_stream_util.py.  Every case is a few hundred waves at most."""

import ctypes as C

import numpy as np
import pytest

from tests import golden_util as G
from tests import ingest_edges_util as IE
from tests import records_stream_util as U

pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1
WIDE_WINDOW_NS = ((1 << 48) - 1) * 4       # 2^48 - 1 ticks of 4 ns: still fits int64 in ps


def _stream(paths, dt_ns, **kw):
    from waveformanalysis_amd.records_stream import HipRecordsStream

    s = HipRecordsStream()
    chunks = list(s.stream_files(paths, dt_ns, **kw))
    return s, chunks


def _static(paths, dt_ns):
    from waveformanalysis_amd.records_builder import build_records_from_v1725_files

    return build_records_from_v1725_files(paths, dt_ns=dt_ns)


def _assert_bundle(chunks, records, wave_pool, what=""):
    rec, pool = U.collect(chunks)
    G.assert_struct_equal(rec, records, what=what)
    assert rec.tobytes() == np.ascontiguousarray(records).tobytes(), what
    assert pool.dtype == np.uint16 and pool.tobytes() == np.ascontiguousarray(wave_pool).tobytes(), what


def _assert_chunk_shape(chunks):
    """Every chunk's rows lie below its horizon; wave_offset runs from pool_base without a gap, through the run."""
    cursor = rid = 0
    for c in chunks:
        d, meta = c.data, c.metadata
        assert len(d) > 0 and int(d["timestamp"].max()) < meta["horizon"]
        assert meta["pool_base"] == cursor == int(d["wave_offset"][0]) and meta["first_record"] == rid
        lengths = d["event_length"].astype(np.int64)
        assert np.array_equal(d["wave_offset"], cursor + np.concatenate(([0], np.cumsum(lengths)[:-1])))
        assert np.array_equal(d["record_id"], rid + np.arange(len(d)))
        assert len(meta["wave_pool"]) == int(lengths.sum())
        cursor += int(lengths.sum())
        rid += len(d)


@pytest.fixture(scope="module")
def fixture_case():
    return U.load_fixture()


@pytest.mark.parametrize("block_bytes", [1, 64, 4096, 1 << 20])
def test_fixture_equality(tmp_path, fixture_case, block_bytes):
    case = fixture_case
    blobs, boards = U.fixture_blobs(case)
    paths = U.write_files(tmp_path, zip(case["file_names"], blobs))
    s, chunks = _stream(paths, 4, block_bytes=block_bytes, reorder_window_ns=8)
    _assert_bundle(chunks, case["records"], case["wave_pool"], "fixture")
    static = _static(paths, 4)
    _assert_bundle(chunks, static.records, static.wave_pool, "static builder")
    _assert_chunk_shape(chunks)
    m = U.model_run(blobs, boards, 4, 8, block_bytes)
    releasing = [(p[0], p[1]) for p in m["pushes"] if p[0] > 0]
    assert [(len(c.data), c.metadata["n_carry"]) for c in chunks] == releasing
    assert [c.metadata["horizon"] for c in chunks] == [p[2] for p in m["pushes"] if p[0] > 0]
    assert s.stats["pushes"] == len(m["pushes"]) and s.stats["max_carry"] == m["max_carry"]
    assert s.stats["rows_in"] == s.stats["rows_out"] == 320
    assert s.stats["bytes_read"] == sum(len(b) for b in blobs)
    # one file alone, at another dt
    s1, single = _stream(paths[2:], 2, block_bytes=block_bytes, reorder_window_ns=4)
    _assert_bundle(single, case["records_single"], case["wave_pool_single"], "single file")
    _assert_chunk_shape(single)


def test_edge_files(tmp_path):
    groups = IE.v1725_file_groups()
    paths = U.write_files(tmp_path, groups)
    for listed in (paths, paths[:3] + [str(tmp_path / "missing_b1_seg9.bin")] + paths[3:], paths + [paths[1]]):
        static = _static(listed, 4)
        for block_bytes in (1, 100, 1 << 20):
            s, chunks = _stream(listed, 4, block_bytes=block_bytes, reorder_window_ns=WIDE_WINDOW_NS)
            _assert_bundle(chunks, static.records, static.wave_pool, f"block_bytes={block_bytes}")
            _assert_chunk_shape(chunks)
    assert len(static.records) > 0 and int((static.records["event_length"] == 0).sum()) > 0


def _tie_files(tmp_path, rng):
    s30a, s30b = rng.integers(-32768, 32768, 6).astype(np.int16), rng.integers(-32768, 32768, 6).astype(np.int16)
    assert not np.array_equal(s30a, s30b)
    mk = lambda n: rng.integers(-32768, 32768, n).astype(np.int16)
    f0 = U.wave_file([(3, 10, mk(4)), (3, 20, mk(8)), (3, 30, s30a)])
    f1 = U.wave_file([(3, 5, mk(2)), (3, 30, s30b), (3, 40, mk(4))])
    return U.write_files(tmp_path, [("tie_b0_seg0.bin", f0), ("tie_b0_seg1.bin", f1)]), s30a, s30b


def test_tie_across_files_of_one_board(tmp_path):
    rng = np.random.default_rng(30)
    paths, s30a, s30b = _tie_files(tmp_path, rng)
    static = _static(paths, 4)
    s, chunks = _stream(paths, 4, block_bytes=1, reorder_window_ns=0)     # one event per block
    _assert_bundle(chunks, static.records, static.wave_pool)
    rec, pool = U.collect(chunks)
    at = np.flatnonzero(rec["timestamp"] == 30 * 4000)
    assert len(at) == 2 and at[1] == at[0] + 1
    first = pool[rec["wave_offset"][at[0]]:][:6].view(np.int16)
    second = pool[rec["wave_offset"][at[1]]:][:6].view(np.int16)
    assert np.array_equal(first, s30a) and np.array_equal(second, s30b)     # file 0's wave first, as in the static table
    # file 1's 30 was read (and carried) before file 0's: the model says so, and the stream agrees push by push
    blobs = [open(p, "rb").read() for p in paths]
    m = U.model_run(blobs, [0, 0], 4, 0, 1)
    order = [p[4] for p in m["pushes"]]
    assert order[:3] == [0, 1, 1] and [w[3] for w in m["released"] if w[0] == 30 * 4000] == [0, 1]
    k1 = [i for i, p in enumerate(m["pushes"]) if p[4] == 1][1]            # the push that read file 1's 30
    k0 = [i for i, p in enumerate(m["pushes"]) if p[4] == 0][2]            # the push that read file 0's 30
    assert k1 < k0
    assert [(len(c.data), c.metadata["n_carry"]) for c in chunks] == [(p[0], p[1]) for p in m["pushes"] if p[0] > 0]


def test_equal_timestamps_at_the_horizon_are_released_together(tmp_path):
    rng = np.random.default_rng(31)
    mk = lambda n: rng.integers(-32768, 32768, n).astype(np.int16)
    # file 0: channel 9 at 50, then 90; file 1: channel 2 at 50 (read later), then 90.  While file 1 stands at 50 the
    # horizon is 50: file 0's wave at 50 is held back, and goes out behind file 1's (smaller channel) once 50 has passed
    f0 = U.wave_file([(9, 50, mk(6)), (9, 90, mk(2))])
    f1 = U.wave_file([(2, 50, mk(4)), (2, 90, mk(8))])
    paths = U.write_files(tmp_path, [("eq_b0_seg0.bin", f0), ("eq_b0_seg1.bin", f1)])
    static = _static(paths, 4)
    s, chunks = _stream(paths, 4, block_bytes=1, reorder_window_ns=0)
    _assert_bundle(chunks, static.records, static.wave_pool)
    first = chunks[0].data
    assert first["timestamp"].tolist()[:2] == [200000, 200000] and first["channel"].tolist()[:2] == [2, 9]
    m = U.model_run([f0, f1], [0, 0], 4, 0, 1)
    assert m["pushes"][0][:2] == (0, 1) and m["pushes"][1][:2] == (0, 2)   # both held at horizon 50
    assert [(len(c.data), c.metadata["n_carry"]) for c in chunks] == [(p[0], p[1]) for p in m["pushes"] if p[0] > 0]


@pytest.mark.parametrize("carried", [False, True])
def test_sample_pass_shapes(tmp_path, carried):
    rng = np.random.default_rng(16)
    events, seen = U.shape_events(rng)
    assert seen["src"] == {0, 4, 8, 12} and seen["dst"] == {0, 2, 4, 6}
    assert len(seen["combos"]) == len(U.SHAPE_LENGTHS) * 16
    blob = IE.v1725_stream(events)
    named = [("shapes_b2_seg0.bin", blob)]
    window = 0
    if carried:
        # a second file whose single late wave keeps the horizon below every wave of the first: the first file's waves
        # are carried through the pushes of its blocks (and moved from sample carry to sample carry) before they go out
        late = U.wave_file([(0, 0, rng.integers(-32768, 32768, 10).astype(np.int16))])
        named = [("shapes_b2_seg1.bin", late), ("shapes_b2_seg0.bin", blob)]
        window = WIDE_WINDOW_NS
    paths = U.write_files(tmp_path, named)
    static = _static(paths, 4)
    s, chunks = _stream(paths, 4, block_bytes=len(blob) // 3, reorder_window_ns=window)
    _assert_bundle(chunks, static.records, static.wave_pool)
    _assert_chunk_shape(chunks)
    if carried:
        # everything went through the carry, the first block's waves through at least two more pushes, and out at the end
        assert len(chunks) == 1 and s.stats["pushes"] >= 4 and s.stats["max_carry"] >= len(static.records) - 200
    else:
        assert len(chunks) >= 3          # released straight from the blocks


def test_bounded_carry(tmp_path):
    rng = np.random.default_rng(300)
    blob = U.wave_file([(k % 16, 1000 + 3 * k, rng.integers(-32768, 32768, 2 * (k % 5)).astype(np.int16)) for k in range(300)])
    paths = U.write_files(tmp_path, [("mono_b0_seg0.bin", blob)])
    static = _static(paths, 4)
    from waveformanalysis_amd.records_stream import HipRecordsStream

    s = HipRecordsStream(block_bytes=256, reorder_window_ns=0)
    chunks = list(s.stream_files(paths, 4))
    _assert_bundle(chunks, static.records, static.wave_pool)
    assert all(c.metadata["n_carry"] == 1 for c in chunks[:-1]) and chunks[-1].metadata["n_carry"] == 0
    assert s.stats["max_carry"] == 1 and s.stats["pushes"] == len(chunks) > 10
    assert s.stats["max_carry_samples"] <= 8


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _push(sess, block, waves, horizon, final=False):
    return sess.records_stream_push(block, waves, horizon, final)


def _waves(ts, off, ns, seq0=0, board=1, channel=None):
    n = len(ts)
    return {"timestamp_ps": np.asarray(ts, np.int64), "seq": seq0 + np.arange(n, dtype=np.int64),
            "payload_offset": np.asarray(off, np.int64), "n_samples": np.asarray(ns, np.int32),
            "board": np.full(n, board, np.int16), "channel": np.arange(n, dtype=np.int16) if channel is None else np.asarray(channel, np.int16),
            "baseline": np.full(n, 77, np.uint16), "trunc": np.zeros(n, np.uint8)}


def test_c_abi_refusals_leave_the_stream_as_it_was():
    from waveformanalysis_amd import _lib
    from waveformanalysis_amd.device import DeviceSession

    rng = np.random.default_rng(7)
    block = rng.integers(0, 256, 64, dtype=np.uint8)
    samples = block.view(np.uint16)
    good1 = _waves([1000, 3000, 2000], [0, 8, 16], [4, 2, 6])
    good2 = _waves([2500, 5000], [4, 12], [2, 4], seq0=10)

    def run(refused: bool):
        """Two accepted pushes and a final flush, with every refusal tried in between when `refused`."""
        with DeviceSession(0) as sess:
            lib, h = sess._lib, sess._h
            out = []
            if refused:
                with pytest.raises(_lib.WfaError) as e:       # _push without _begin
                    _push(sess, block, good1, 0)
                assert e.value.code == _lib.WFA_E_STATE
                with pytest.raises(ValueError):                # dt_ns <= 0
                    sess.records_stream_begin(0)
            sess.records_stream_begin(4)
            if refused:
                rows, pool = np.zeros(1, dtype="V102"), np.zeros(8, np.uint16)
                assert lib.wfa_records_stream_fill(h, rows.ctypes.data_as(C.c_void_p), pool.ctypes.data_as(C.c_void_p), 0, 0) \
                    == _lib.WFA_E_STATE                        # _fill before a push
            out.append(_push(sess, block, good1, 2500))
            if refused:
                bad = [
                    (_waves([2499], [0], [2]), 2500),                    # a row below the previous horizon
                    (_waves([2600], [0], [2]), 2499),                    # a horizon below the previous one
                    (_waves([2600], [60], [4]), 2600),                   # a payload slice outside the block
                    (_waves([2600], [-4], [2]), 2600),
                    (_waves([2600], [2], [2]), 2600),                    # not 4-byte aligned
                    (_waves([2600], [0], [-2]), 2600),                   # negative n_samples
                    (_waves([2600], [0], [3]), 2600),                    # odd n_samples
                ]
                for waves, horizon in bad:
                    with pytest.raises(ValueError):
                        _push(sess, block, waves, horizon)
                    assert lib.wfa_records_stream_fill(h, None, None, 0, 0) == _lib.WFA_E_STATE    # after a refused push
                # carry + new rows >= 2^31: refused on the count alone (the columns are not read)
                cols = [good1[name].ctypes.data_as(C.c_void_p) for name, _ in sess.RECORDS_STREAM_COLUMNS]
                n4 = [C.c_int64(0) for _ in range(4)]
                rc = lib.wfa_records_stream_push(h, block.ctypes.data_as(C.c_void_p), 64, (1 << 31) - 1, *cols, 2600, 0,
                                                 *[C.byref(v) for v in n4])
                assert rc == _lib.WFA_E_INVALID
            out.append(_push(sess, block, good2, 2500))
            if refused:
                rows = np.zeros(len(out[-1][0]) + 1, dtype="V102")
                rc = lib.wfa_records_stream_fill(h, rows.ctypes.data_as(C.c_void_p), None, len(rows), len(out[-1][1]))
                assert rc == _lib.WFA_E_INVALID                # _fill with other counts
            out.append(_push(sess, None, None, I64_MAX, final=True))
            sess.records_stream_end()
            return out

    plain, tried = run(False), run(True)
    for (r0, p0, c0, s0), (r1, p1, c1, s1) in zip(plain, tried):
        assert r0.tobytes() == r1.tobytes() and p0.tobytes() == p1.tobytes() and (c0, s0) == (c1, s1)
    # and the accepted pushes are right: release below 2500 in (timestamp, board, channel, seq) order
    rows, pool, n_carry, n_carry_samples = plain[0]
    assert rows["timestamp"].tolist() == [1000, 2000] and (n_carry, n_carry_samples) == (1, 2)
    assert rows["wave_offset"].tolist() == [0, 4] and rows["event_length"].tolist() == [4, 6]
    assert np.array_equal(pool, np.concatenate([samples[0:4], samples[8:14]]))
    assert rows["time"].tolist() == [1, 2] and rows["dt"].tolist() == [4, 4] and rows["baseline"].tolist() == [77.0, 77.0]
    assert rows["polarity"].tolist() == ["unknown"] * 2 and np.isnan(rows["baseline_upstream"]).all()
    rows, pool, n_carry, n_carry_samples = plain[1]
    assert len(rows) == 0 and (n_carry, n_carry_samples) == (3, 8)
    rows, pool, n_carry, n_carry_samples = plain[2]
    assert rows["timestamp"].tolist() == [2500, 3000, 5000] and rows["record_id"].tolist() == [2, 3, 4]
    assert rows["wave_offset"].tolist() == [10, 12, 14] and (n_carry, n_carry_samples) == (0, 0)
    assert np.array_equal(pool, np.concatenate([samples[2:4], samples[4:6], samples[6:10]]))


def test_stream_stays_open_beside_the_others_and_survives_release_scratch():
    from waveformanalysis_amd.device import DeviceSession

    block = np.arange(32, dtype=np.uint8)
    with DeviceSession(0) as sess:
        sess.records_stream_begin(2)
        sess.df_event_stream_begin(100.0)
        rows, pool, n_carry, _ = _push(sess, block, _waves([10, 30], [0, 8], [4, 8]), 20)
        assert len(rows) == 1 and n_carry == 1
        sess.release_scratch()
        rows, pool, n_carry, _ = _push(sess, None, None, I64_MAX, final=True)
        assert rows["timestamp"].tolist() == [30] and np.array_equal(pool, block.view(np.uint16)[4:12]) and n_carry == 0
        sess.df_event_stream_end()
        sess.records_stream_end()


def test_plugin_refusals_and_empty_runs(tmp_path):
    from waveformanalysis_amd.plugin_api import SimpleContext
    from waveformanalysis_amd.records_stream import HipRecordsStream

    rng = np.random.default_rng(9)
    mk = lambda n: rng.integers(-32768, 32768, n).astype(np.int16)
    good = U.wave_file([(0, 100, mk(4)), (1, 200, mk(4))])
    late = U.wave_file([(0, 100, mk(4)), (1, 300, mk(4)), (2, 200, mk(4)), (3, 400, mk(4))])
    paths = U.write_files(tmp_path, [("good_b0_seg0.bin", good), ("late_b0_seg1.bin", late), ("empty_b0_seg2.bin", b"")])
    ctx = SimpleContext(config={"daq_adapter": "vx2730"}, data={"raw_files": [paths[:1]]})
    with pytest.raises(ValueError, match="v1725"):
        list(HipRecordsStream().compute(ctx, "run"))
    with pytest.raises(ValueError, match="block_bytes"):
        list(HipRecordsStream().stream_files(paths[:1], 4, block_bytes=0))
    # a window violation: raised before that block is uploaded -- the chunks before it are those of the blocks before it
    s = HipRecordsStream(block_bytes=1, reorder_window_ns=0)
    got = []
    with pytest.raises(ValueError, match=r"late_b0_seg1.bin: wave 2 .*400 would have been needed"):
        for c in s.stream_files(paths[1:2], 4):
            got.append(c)
    assert s.stats["pushes"] == 2 and s.stats["rows_in"] == 2      # the third block never went up
    assert sum(len(c.data) for c in got) == 1
    # an event larger than block_bytes is read whole
    big = IE.v1725_stream([(0x0007, [(5, 0, 1, mk(40)), (6, 0, 2, mk(60)), (7, 0, 3, mk(20))])])
    bpath = U.write_files(tmp_path, [("big_b1_seg0.bin", big)])
    s = HipRecordsStream(block_bytes=16, reorder_window_ns=0)
    chunks = list(s.stream_files(bpath, 4))
    static = _static(bpath, 4)
    _assert_bundle(chunks, static.records, static.wave_pool)
    assert s.stats["pushes"] == 1 and s.stats["rows_in"] == 3
    # all files empty or missing: no chunk
    assert list(HipRecordsStream().stream_files([paths[2], str(tmp_path / "nothing_b0.bin")], 4)) == []
    assert list(HipRecordsStream().stream_files([], 4)) == []
    # compute(): paths from raw_files, dt from the adapter
    ctx = SimpleContext(config={"daq_adapter": "v1725", "records_stream": {"reorder_window_ns": 0, "block_bytes": 64}},
                        data={"raw_files": [paths[:1], paths[:1]]})
    chunks = list(HipRecordsStream().compute(ctx, "run"))
    static = _static(paths[:1], 4)
    _assert_bundle(chunks, static.records, static.wave_pool)


@pytest.mark.parametrize("use_filtered", [False, True])
def test_files_to_hits(tmp_path, fixture_case, use_filtered):
    from waveformanalysis_amd.plugin_api import SimpleContext
    from waveformanalysis_amd.plugins import HipThresholdHitPlugin
    from waveformanalysis_amd.streaming import HipThresholdHitStream

    case = fixture_case
    blobs, _boards = U.fixture_blobs(case)
    paths = U.write_files(tmp_path, zip(case["file_names"], blobs))
    _s, chunks = _stream(paths, 4, block_bytes=4096, reorder_window_ns=8)
    static = _static(paths, 4)
    longest = int(static.records["event_length"].max())
    cfg = {"threshold": 25.0, "use_filtered": use_filtered}
    if use_filtered:
        cfg.update({"sg_window_size": 7, "sg_poly_order": 2})
    stream = HipThresholdHitStream(max_len=longest, **cfg)
    out = stream.run_chunks(chunks, SimpleContext(), "run")
    assert len(out) == len(chunks)
    for c in out:
        assert "wave_pool" not in c.metadata and "pool_base" not in c.metadata and "horizon" in c.metadata
    got = np.concatenate([c.data for c in out])
    # hit_threshold of the static bundle under the same configuration (the fused route reads the filter settings of the
    # registered wave_pool_filtered plugin)
    from waveformanalysis_amd.plugins import HipWavePoolFilteredPlugin

    ctx = SimpleContext({"wave_source": "records", "hit_threshold": {"threshold": 25.0, "use_filtered": use_filtered,
                                                                     "fuse_filter": use_filtered},
                         "wave_pool_filtered": {"filter_type": "SG", "sg_window_size": 7, "sg_poly_order": 2}},
                        {"records": static.records, "wave_pool": static.wave_pool},
                        plugins=[HipWavePoolFilteredPlugin(), HipThresholdHitPlugin()])
    want = ctx.get_data("run", "hit_threshold")
    assert len(want) > 0
    G.assert_struct_equal(got, want)
