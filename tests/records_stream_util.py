"""Shared helpers of the records stream tests: an independent numpy / pure-Python model of the stream's rule (blocks of
whole events, read schedule, horizon, release), crafted V1725 files, and the fixture.

The model shares no code with waveformanalysis_amd.records_stream: events are walked here, byte by byte, and a push
releases (everything carried + the new waves), sorted by (timestamp, board, channel, file, wave index), cut at the horizon.
"""

from __future__ import annotations

import os
import re

import numpy as np

from tests import golden_util as G
from tests import ingest_edges_util as IE

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1


def load_fixture() -> dict:
    z = np.load(os.path.join(G.GOLDEN, "v1725bin_files.npz"), allow_pickle=False)
    case = {k: z[k] for k in z.files}
    case["file_names"] = bytes(case["names"]).decode().split("\n")
    return case


def board_of(name: str) -> int:
    m = re.search(r"_b(\d+)", os.path.basename(name), flags=re.IGNORECASE)
    return int(m.group(1)) if m else 0


def v1725_events(blob: bytes):
    """[(end of event, [(channel, timestamp, trunc, baseline, payload_offset, n_samples), ...])] of a whole file.  Bytes
    behind the last whole event -- a short header, or an event cut in a channel header or payload -- are one last entry that
    ends with the file and holds the complete waves of the cut event."""
    blob = bytes(blob)
    n, pos, out = len(blob), 0, []
    while pos + 16 <= n:
        mask = blob[pos + 4] + 256 * blob[pos + 11]
        pos += 16
        waves, cut = [], False
        for ch in range(16):
            if not mask & (1 << ch):
                continue
            if pos + 12 > n:
                cut = True
                break
            words = int.from_bytes(blob[pos:pos + 3], "little") % (1 << 22)
            if words < 3:
                raise ValueError(f"V1725 channel size {words} < 3 words at byte {pos}")
            size = 4 * (words - 3)
            if pos + 12 + size > n:
                cut = True
                break
            waves.append((ch, int.from_bytes(blob[pos + 4:pos + 10], "little"), (blob[pos + 3] & 0x40) >> 6,
                          int.from_bytes(blob[pos + 10:pos + 12], "little"), pos + 12, size // 2))
            pos += 12 + size
        if cut:
            out.append((n, waves))
            return out
        out.append((pos, waves))
    if pos < n:
        out.append((n, []))
    return out


def model_blocks(blob: bytes, block_bytes: int):
    """[(start, end, waves, at_end)]: whole events from the current position while (end of event - start) <= block_bytes,
    at least one; an empty file is one empty block."""
    events = v1725_events(blob)
    if not events:
        return [(0, 0, [], True)]
    out, k, start = [], 0, 0
    while k < len(events):
        end, waves = events[k]
        waves = list(waves)
        k += 1
        while k < len(events) and events[k][0] - start <= block_bytes:
            end = events[k][0]
            waves += events[k][1]
            k += 1
        out.append((start, end, waves, k == len(events)))
        start = end
    return out


def model_run(blobs, boards, dt_ns: int, window_ns: int, block_bytes: int) -> dict:
    """The stream's rule on whole files held in memory.  -> released: the rows (timestamp ps, board, channel, n_samples,
    file, wave index, payload offset in the file) in release order; pushes: per push (records out, records carried, H,
    final, file); max_carry."""
    window = window_ns * 1000
    nf = len(blobs)
    blocks = [model_blocks(b, block_bytes) for b in blobs]
    at = [0] * nf                 # next block of every file
    hi = [None] * nf
    waves_read = [0] * nf
    held: list = []
    released: list = []
    pushes: list = []
    max_carry = 0

    def low(f):
        return I64_MIN if hi[f] is None else max(hi[f] - window, I64_MIN)

    while True:
        left = [f for f in range(nf) if at[f] < len(blocks[f])]
        if not left:
            break
        f = min(left, key=lambda g: (low(g), g))
        _start, _end, waves, _at_end = blocks[f][at[f]]
        at[f] += 1
        for ch, ticks, _trunc, _bl, off, ns in waves:
            ts = ticks * dt_ns * 1000
            if hi[f] is not None and ts < hi[f] - window:
                raise ValueError(f"model: file {f} wave {waves_read[f]} breaks the promise")
            hi[f] = ts if hi[f] is None else max(hi[f], ts)
            held.append((ts, boards[f], ch, f, waves_read[f], ns, off))
            waves_read[f] += 1
        left = [g for g in range(nf) if at[g] < len(blocks[g])]
        final = not left
        horizon = I64_MAX if final else min(low(g) for g in left)
        held.sort(key=lambda w: w[:5])
        n_out = len(held) if final else sum(1 for w in held if w[0] < horizon)
        released += held[:n_out]
        held = held[n_out:]
        pushes.append((n_out, len(held), horizon, final, f))
        max_carry = max(max_carry, len(held))
    return {"released": released, "pushes": pushes, "max_carry": max_carry}


def fixture_blobs(case: dict):
    names = case["file_names"]
    return [bytes(case[f"blob{k}"]) for k in range(len(names))], [board_of(n) for n in names]


def write_files(tmp_path, named_blobs) -> list[str]:
    paths = []
    for name, blob in named_blobs:
        p = tmp_path / name
        p.write_bytes(bytes(blob))
        paths.append(str(p))
    return paths


def collect(chunks):
    """(records, wave_pool) of a list of records stream chunks, concatenated."""
    from waveformanalysis_amd.dtypes import RECORDS_DTYPE

    if not chunks:
        return np.zeros(0, dtype=RECORDS_DTYPE), np.zeros(0, dtype=np.uint16)
    return np.concatenate([c.data for c in chunks]), np.concatenate([c.metadata["wave_pool"] for c in chunks])


def wave_file(waves) -> bytes:
    """DAW_DEMO bytes of [(channel, timestamp ticks, samples)]: one event per wave."""
    return IE.v1725_stream([(1 << ch, [(ts, 0, 100 + ch, np.asarray(s, dtype=np.int16))]) for ch, ts, s in waves])


SHAPE_LENGTHS = (0, 2, 6, 8, 14, 16, 18, 1022, 1024, 1026)


def shape_events(rng):
    """One event per wave, timestamps increasing, so that the pool order is the file order: lengths x (source residue mod
    16 bytes in 0, 4, 8, 12) x (destination residue mod 8 samples in 0, 2, 4, 6).  In front of every wave under test a
    short wave sets the destination residue (as gather_cases does), then 0..3 zero-sample waves -- 28 bytes of headers
    each, 12 mod 16, and nothing in the pool -- set the source residue.  -> (events for IE.v1725_stream, counters)."""
    events, ts = [], 1
    pos = cursor = 0       # byte position in the file, sample position in the pool
    seen = {"src": set(), "dst": set(), "combos": set()}
    for length in SHAPE_LENGTHS:
        for smod in (0, 4, 8, 12):
            for dmod in (0, 2, 4, 6):
                pad = (dmod - cursor) % 8
                events.append((0x0001, [(ts, 0, 7, rng.integers(-32768, 32768, pad).astype(np.int16))]))
                ts += 1
                pos += 28 + 2 * pad
                cursor += pad
                while (pos + 28) % 16 != smod:
                    events.append((0x0004, [(ts, 0, 8, np.zeros(0, dtype=np.int16))]))
                    ts += 1
                    pos += 28
                events.append((0x0002, [(ts, 1, 9, rng.integers(-32768, 32768, length).astype(np.int16))]))
                ts += 1
                seen["src"].add((pos + 28) % 16)
                seen["dst"].add(cursor % 8)
                seen["combos"].add((length, (pos + 28) % 16, cursor % 8))
                pos += 28 + 2 * length
                cursor += length
    return events, seen
