"""Records stream, the parts that need no GPU: the block walker (host code of the library), the read schedule and
horizon rule (pure Python), and the declarations."""

import os
import re

import numpy as np
import pytest

from tests import ingest_edges_util as IE
from tests import records_stream_util as U
from waveformanalysis_amd import _lib
from waveformanalysis_amd import records_builder as RB
from waveformanalysis_amd.records_stream import HORIZON_END, BlockFile, HipRecordsStream, ReadSchedule, window_ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN = -(1 << 63)
COLS = ("channel", "timestamp", "trunc", "baseline", "payload_offset", "n_samples")


def _rows(idx, base=0):
    return [(int(idx["channel"][k]), int(idx["timestamp"][k]), int(idx["trunc"][k]), int(idx["baseline"][k]),
             int(idx["payload_offset"][k]) + base, int(idx["n_samples"][k])) for k in range(len(idx["channel"]))]


def _chain(blob: bytes, block_bytes: int):
    """Windows of block_bytes (grown by block_bytes while they hold no whole event) chained by consumed_bytes ->
    (waves with offsets rebased to the file, end of the stream)."""
    buf = np.frombuffer(blob, dtype=np.uint8)
    pos, out = 0, []
    while True:
        size = block_bytes
        while True:
            at_end = pos + size >= len(buf)
            idx, used = RB.v1725_index_block(buf[pos:pos + size], at_end)
            if used > 0 or at_end:
                break
            assert len(idx["channel"]) == 0      # a window that ends inside its first event yields no wave of it
            size += block_bytes
        out += _rows(idx, pos)
        assert used == (min(size, len(buf) - pos) if at_end else used) and used <= len(buf) - pos
        pos += used
        if at_end:
            return out, pos


def test_block_walker_chains_to_the_plain_walk():
    blobs = {"prefix": IE.v1725_prefix_stream()}
    blobs.update({name: blob for name, (blob, _board) in IE.v1725_cases().items()})
    for name, blob in blobs.items():
        want = IE.v1725_walk(blob)
        for block_bytes in range(1, len(blob) + 2):
            got, end = _chain(blob, block_bytes)
            assert got == want, (name, block_bytes)
            assert end == len(blob), (name, block_bytes)


def test_block_walker_cut_event_and_file_end():
    blob = IE.v1725_prefix_stream()
    events = U.v1725_events(blob)
    buf = np.frombuffer(blob, dtype=np.uint8)
    start = 0
    for end, waves in events:
        for cut in range(start + 1, end):       # every buffer that ends inside this event
            idx, used = RB.v1725_index_block(buf[:cut], False)
            assert used == start, cut
            assert _rows(idx) == [w for e, ws in events if e <= start for w in ws], cut
            idx_end, used_end = RB.v1725_index_block(buf[:cut], True)
            assert used_end == cut and _rows(idx_end) == IE.v1725_walk(blob[:cut]), cut
        start = end
    idx, used = RB.v1725_index_block(buf, False)
    assert used == len(blob) and _rows(idx) == IE.v1725_walk(blob)
    bad = bytearray(blob)
    bad[16:19] = (2, 0, 0)
    for at_end in (False, True):
        with pytest.raises(ValueError, match="channel size"):
            RB.v1725_index_block(np.frombuffer(bytes(bad), dtype=np.uint8), at_end)
    plain = RB.v1725_index(buf)
    assert _rows(plain) == IE.v1725_walk(blob)      # the plain walker still is the same loop


def test_block_file_follows_the_block_rule(tmp_path):
    cases = {"prefix": IE.v1725_prefix_stream(), "empty": b""}
    cases.update({name: blob for name, (blob, _b) in IE.v1725_cases().items()})
    for name, blob in cases.items():
        path = tmp_path / f"{name}.bin"
        path.write_bytes(blob)
        for block_bytes in (1, 17, 64, 100, 4096):
            bf = BlockFile(str(path), block_bytes)
            got, pos = [], 0
            for start, end, waves, at_end in U.model_blocks(blob, block_bytes):
                block, idx, file_end = bf.next_block()
                assert (pos, pos + len(block), file_end) == (start, end, at_end), (name, block_bytes)
                assert _rows(idx, pos) == waves, (name, block_bytes)
                pos += len(block)
            bf.close()
            assert pos == len(blob) and bf.bytes_read == len(blob)


def _fixture_model(block_bytes, window_ns=8):
    case = U.load_fixture()
    blobs, boards = U.fixture_blobs(case)
    return case, U.model_run(blobs, boards, 4, window_ns, block_bytes)


@pytest.mark.parametrize("block_bytes", [1, 64, 4096, 1 << 20])
def test_model_reproduces_the_fixture_order(block_bytes):
    case, m = _fixture_model(block_bytes)
    want = case["records"]
    got = m["released"]
    assert len(got) == len(want) == 320
    assert [w[0] for w in got] == want["timestamp"].tolist()
    assert [w[1] for w in got] == want["board"].tolist()
    assert [w[2] for w in got] == want["channel"].tolist()
    assert [w[5] for w in got] == want["event_length"].tolist()
    horizons = [p[2] for p in m["pushes"]]
    assert horizons == sorted(horizons) and m["pushes"][-1][3] and not any(p[3] for p in m["pushes"][:-1])


def test_model_does_not_hold_everything():
    """So that the tests against the model cannot pass by releasing everything at the end."""
    _case, m = _fixture_model(4096)
    early = sum(1 for n_out, _c, _h, final, _f in m["pushes"] if n_out > 0 and not final)
    print("pushes", len(m["pushes"]), "releasing before the final one", early, "max carry", m["max_carry"])
    assert early > len(m["pushes"]) / 2
    assert m["max_carry"] < 320 / 4


def _drive_schedule(blobs, boards, dt_ns, window_ns, block_bytes, names=None):
    """The schedule object fed the model's blocks: what it asks to read and the (H, final) it answers."""
    blocks = [U.model_blocks(b, block_bytes) for b in blobs]
    sched = ReadSchedule(names or [f"file{k}" for k in range(len(blobs))], window_ns)
    at = [0] * len(blobs)
    order, answers = [], []
    while True:
        f = sched.next_file()
        if f is None:
            break
        _s, _e, waves, at_end = blocks[f][at[f]]
        at[f] += 1
        ts = np.array([w[1] * dt_ns * 1000 for w in waves], dtype=np.int64)
        answers.append(sched.feed(f, ts, at_end))
        order.append(f)
    assert all(a == len(b) for a, b in zip(at, blocks))
    return order, answers


@pytest.mark.parametrize("block_bytes", [1, 64, 4096, 1 << 20])
def test_schedule_matches_the_model_on_the_fixture(block_bytes):
    case, m = _fixture_model(block_bytes)
    blobs, boards = U.fixture_blobs(case)
    order, answers = _drive_schedule(blobs, boards, 4, 8, block_bytes, case["file_names"])
    assert order == [p[4] for p in m["pushes"]]
    assert [(h, fin) for h, fin in answers] == [(p[2], p[3]) for p in m["pushes"]]
    horizons = [h for h, _ in answers]
    assert horizons == sorted(horizons)
    assert answers[-1] == (HORIZON_END, True)


def test_schedule_window_violation_names_the_file():
    case = U.load_fixture()
    blobs, boards = U.fixture_blobs(case)
    with pytest.raises(ValueError) as err:
        _drive_schedule(blobs, boards, 4, 4, 4096, case["file_names"])
    assert any(name in str(err.value) for name in case["file_names"])
    assert "wave" in str(err.value) and "8 would have been needed" in str(err.value)
    with pytest.raises(ValueError):
        U.model_run(blobs, boards, 4, 4, 4096)
    # the refusal takes nothing: the file's state is as before the block
    s = ReadSchedule(["a_b0.bin"], 1)
    s.feed(0, [5000, 9000], False)
    with pytest.raises(ValueError, match="a_b0.bin: wave 3 "):
        s.feed(0, [8500, 7000], False)
    assert s.hi[0] == 9000 and s.waves[0] == 2
    assert s.feed(0, [8000, 12000], False) == (11000, False)


def test_schedule_ties_unread_files_and_saturation():
    s = ReadSchedule(["f0", "f1", "f2"], 0)
    assert s.next_file() == 0 and s.low(1) == I64_MIN
    assert s.feed(0, [100], False) == (I64_MIN, False)       # files never read keep H at the smallest int64
    assert s.next_file() == 1
    assert s.feed(1, [100], False) == (I64_MIN, False)
    assert s.next_file() == 2
    assert s.feed(2, [300], False) == (100, False)
    assert s.next_file() == 0                                  # tie of low_0 = low_1 = 100: the lowest index
    assert s.feed(0, [200], False) == (100, False)
    assert s.next_file() == 1
    assert s.feed(1, [], True) == (200, False)                 # a finished file no longer holds the horizon back
    assert s.feed(0, [250], True) == (300, False)
    assert s.feed(2, [], True) == (HORIZON_END, True)
    assert s.next_file() is None
    wide = ReadSchedule(["f"], (1 << 63) // 1000)              # low saturates instead of wrapping
    assert wide.feed(0, [-(1 << 62), -(1 << 62) - 5], False) == (I64_MIN, False)
    assert wide.low(0) == I64_MIN and wide.hi[0] == -(1 << 62)


def test_window_overflow_and_option_refusals():
    assert window_ps(8) == 8000 and window_ps(0) == 0
    assert window_ps(((1 << 63) - 1) // 1000) == ((1 << 63) - 1) // 1000 * 1000
    for bad in (((1 << 63) - 1) // 1000 + 1, -1, 1.5, None, True):
        with pytest.raises(ValueError):
            window_ps(bad)
    with pytest.raises(ValueError):
        ReadSchedule(["f"], 1 << 62)
    with pytest.raises(ValueError, match="v1725"):
        HipRecordsStream(daq_adapter="vx2730")
    with pytest.raises(ValueError, match="block_bytes"):
        HipRecordsStream(block_bytes=0)
    with pytest.raises(ValueError):
        HipRecordsStream(reorder_window_ns=1 << 62)
    with pytest.raises(TypeError):
        HipRecordsStream(no_such_option=1)
    s = HipRecordsStream()
    assert s.provides == "records_stream" and s.depends_on == ["raw_files"]
    assert s.cfg["block_bytes"] == 64 << 20 and s.cfg["reorder_window_ns"] == 0


def test_profile_and_exports():
    from waveformanalysis_amd import plugins

    names = [p.provides for p in plugins.hip_streaming_records()]
    assert names == [p.provides for p in plugins.hip_streaming()] + ["records_stream"]


def test_declared_symbols_and_abi_version():
    header = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    for name in ("wfa_v1725_index_block", "wfa_records_stream_begin", "wfa_records_stream_push", "wfa_records_stream_fill",
                 "wfa_records_stream_end"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES
    assert int(re.search(r"#define WFA_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 12
    assert _lib.load().wfa_abi_version() == _lib.ABI_VERSION
