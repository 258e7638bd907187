"""st_waveforms built from raw files on the GPU (reference: waveform_analysis/core/plugins/builtin/cpu/waveforms.py
`WaveformsPlugin.compute` :1111-1254, `_load_waveforms_flat` :1256-1414, `WaveformStruct` :625-860, the streaming
structurizer :351-478 and `_convert_v1725_to_st_waveforms` :233-290).

The reference parses every CSV file with pandas / pyarrow, stacks each channel list and fills the packed rows of
create_record_dtype(L) with a strided host pass.  Here the file texts are decoded on the GPU into the session's sample
arena (the records path's decoder, records_builder._decode_parts' part mechanism), the rows are packed once into the
resident pool for the baseline means (k_baseline_mean over the untruncated rows), and one kernel (wfa_st_pack) writes
the final packed rows, which come down through the pinned staging ring in bounded batches.  There is no sort: st rows
are in raw-file order.
"""

from __future__ import annotations

import io
import os
from typing import Sequence

import numpy as np

from . import records_builder as RB
from .dtypes import RECORDS_DTYPE, create_record_dtype

DEFAULT_WAVE_LENGTH = 1500        # processing/dtypes.py:16
DEFAULT_PACK_BATCH_BYTES = 512 << 20
VX2730_SAMPLES_START = RB.VX2730_SAMPLES_START
ST_HEADER_BYTES = 76
# byte offsets of numpy's packed create_record_dtype(L) rows, as k_st_pack writes them
ST_FIELD_OFFSETS = {"baseline": 0, "baseline_upstream": 8, "polarity": 16, "timestamp": 48, "record_id": 56, "dt": 64,
                    "event_length": 68, "board": 72, "channel": 74, "wave": 76}
SNIFF_DELIMITERS = (";", ",", "\t", "|")


def check_st_layout(wave_length: int) -> np.dtype:
    """create_record_dtype(wave_length), after checking numpy lays it out as k_st_pack writes it."""
    dtype = create_record_dtype(int(wave_length))
    got = {name: dtype.fields[name][1] for name in dtype.names}
    if got != ST_FIELD_OFFSETS or dtype.itemsize != ST_HEADER_BYTES + 2 * int(wave_length) or \
            dtype["polarity"].itemsize != 32:
        raise RuntimeError(f"create_record_dtype({wave_length}) is not the packed layout wfa_st_pack writes: {got}")
    return dtype


def empty_st(wave_length: int | None = None) -> np.ndarray:
    return np.zeros(0, dtype=create_record_dtype(int(wave_length) if wave_length is not None else DEFAULT_WAVE_LENGTH))


def _lines(data: bytes):
    """The file's lines as `open(path, encoding="utf-8", errors="replace")` yields them (universal newlines)."""
    return io.TextIOWrapper(io.BytesIO(data), encoding="utf-8", errors="replace")


def _is_number(token: str) -> bool:
    try:
        float(token)
    except ValueError:
        return False
    return True


def sniff_csv_layout(data: bytes | None, default_delimiter: str = ";", max_lines: int = 50) -> tuple[str, int]:
    """(delimiter, header rows) of one file (waveforms.py:83-138 `_sniff_csv_layout`); data=None for a file that
    cannot be read.  The header-row count indexes the non-blank lines among the first `max_lines`."""
    if data is None:
        return default_delimiter, 0
    fh = _lines(data[: 1 << 20] if len(data) > 1 << 20 else data)
    lines = []
    for _ in range(max_lines):
        line = fh.readline()
        if not line:
            break
        line = line.strip()
        if line:
            lines.append(line)
    if not lines:
        return default_delimiter, 0
    delimiter, best = default_delimiter, -1
    for cand in SNIFF_DELIMITERS:
        counts = sorted(line.count(cand) + 1 for line in lines if cand in line)
        if counts and counts[len(counts) // 2] > best:
            best, delimiter = counts[len(counts) // 2], cand
    for idx, line in enumerate(lines):
        parts = [p for p in line.split(delimiter) if p != ""]
        if len(parts) < 3:
            continue
        sample = parts[: min(8, len(parts))]
        if sum(1 for p in sample if _is_number(p)) / max(len(sample), 1) >= 0.6:
            return delimiter, idx
    return delimiter, 0


def _first_data_width(data: bytes, delimiter: str, skiprows: int) -> int | None:
    """Field count of the first non-blank line after `skiprows` lines (waveforms.py:141-165)."""
    fh = _lines(data)
    for _ in range(skiprows):
        fh.readline()
    line = fh.readline()
    while line and not line.strip():
        line = fh.readline()
    return line.count(delimiter) + 1 if line else None


def _read(path) -> bytes | None:
    try:
        with open(path, "rb") as fh:
            return fh.read()
    except OSError:
        return None


def detect_wave_length(texts: Sequence[Sequence[bytes | None]], samples_start: int = VX2730_SAMPLES_START,
                       default_delimiter: str = ";") -> int | None:
    """`_detect_wave_length_from_files`: the first file (list order, then file order) with a data line gives
    count(delimiter) + 1 - samples_start; None when no file has one."""
    for group in texts:
        for data in group:
            if data is None:
                continue
            delimiter, skiprows = sniff_csv_layout(data, default_delimiter)
            width = _first_data_width(data, delimiter, skiprows)
            if width is not None and width > samples_start:
                return int(width - samples_start)
    return None


def decode_plan(delimiters: Sequence[str], bodies: Sequence[bytes], part_bytes: int) -> list[tuple[str, list]]:
    """Decode parts of a run: files in order, cut at every change of delimiter and then by vx2730_parts (at file ends
    or after a '\\n', at most part_bytes each).  -> [(delimiter, [(file index, start, end), ...]), ...]."""
    plan: list[tuple[str, list]] = []
    k = 0
    while k < len(bodies):
        j = k
        while j < len(bodies) and delimiters[j] == delimiters[k]:
            j += 1
        for part in RB.vx2730_parts(bodies[k:j], min(int(part_bytes), RB.MAX_PART_BYTES)):
            plan.append((delimiters[k], [(f + k, a, b) for f, a, b in part]))
        k = j
    return plan


def _decode_run(sess, delimiters, bodies, part_bytes: int, timings: dict | None) -> dict:
    """Every part decoded into the session's sample arena (csv_decode_part); tables concatenated, row_offset relative
    to the concatenated bodies."""
    import time

    total_bytes = sum(len(b) for b in bodies)
    sess.csv_arena_reserve(total_bytes // 4 + 1, keep_filled=False)
    tables, sample_base, byte_base = [], 0, 0
    t0 = time.perf_counter()
    for delimiter, part in decode_plan(delimiters, bodies, part_bytes):
        text = RB._part_text(bodies, part)
        d = sess.csv_decode_part(text, sample_base, delimiter, VX2730_SAMPLES_START, (0, 1, 2))
        d["row_offset"] += byte_base
        tables.append(d)
        byte_base += len(text)
        sample_base += d["n_samples"]
    if timings is not None:
        timings["decode"] = timings.get("decode", 0.0) + time.perf_counter() - t0
    out = {k: np.concatenate([d[k] for d in tables]) for k in ("meta", "row_offset", "n_fields", "sample_offset")}
    out["n_samples"] = sample_base
    return out


def _polarity_codes(polarity: np.ndarray | str, n: int) -> tuple[np.ndarray, list[str]]:
    if isinstance(polarity, str):
        return np.zeros(n, dtype=np.uint8), [polarity]
    table, codes = np.unique(np.asarray(polarity, dtype="U8"), return_inverse=True)
    if len(table) > 8:
        raise ValueError(f"{len(table)} distinct polarity strings; wfa_st_pack takes at most 8")
    return codes.astype(np.uint8), [str(t) for t in table]


def build_st_waveforms_from_vx2730_files(raw_files, wave_length: int | None = None, dt_ns: int = 2,
                                         baseline_samples=None, polarity_of=None, streaming: bool = False,
                                         upstream_baselines=None, session=None,
                                         part_bytes: int = 1 << 30, pack_batch_bytes: int = DEFAULT_PACK_BATCH_BYTES,
                                         timings: dict | None = None) -> np.ndarray:
    """st_waveforms of a VX2730 CSV run: raw_files is a list of per-channel file lists.

    Rows in channel-list order, then file order, then row order; empty lists, empty and missing files are skipped.
    wave_length=None: detected from the first data line (detect_wave_length), else DEFAULT_WAVE_LENGTH.  Per channel
    list of width W fields: event_length = min(W - 7, L); baseline = mean of samples [b0, min(b1, W - 7)) of the
    untruncated row (NaN when empty); rows narrower than W count as NaN-padded, as the reference's stacking does.
    polarity_of(boards, channels) -> per-row polarity strings (batch mode); streaming=True leaves polarity empty and
    baseline_upstream NaN.  upstream_baselines[k]: baseline_upstream of channel list k when its length matches."""
    import time

    RB._baseline_window(baseline_samples, 0, 0, 1)     # the reference's validation messages
    b0, b1 = RB._baseline_window(baseline_samples, VX2730_SAMPLES_START, *RB.VX2730_BASELINE_COLUMNS)
    s0, s1 = b0 - VX2730_SAMPLES_START, b1 - VX2730_SAMPLES_START
    t0 = time.perf_counter()
    texts = [[_read(p) for p in (group or [])] for group in (raw_files or [])]
    if wave_length is None:
        wave_length = detect_wave_length(texts)
    L = int(wave_length) if wave_length is not None else DEFAULT_WAVE_LENGTH
    dtype = check_st_layout(L)
    bodies, delimiters, file_list, file_base = [], [], [], []
    total = 0
    for k, group in enumerate(texts):
        for data in group:
            if not data:                       # missing or empty
                continue
            delimiter, skiprows = sniff_csv_layout(data)
            body = RB._strip_rows(data, skiprows)
            if body and not body.endswith(b"\n"):
                body += b"\n"
            if not body:
                continue
            bodies.append(body)
            delimiters.append(delimiter)
            file_list.append(k)
            file_base.append(total)
            total += len(body)
    if timings is not None:
        timings["read"] = timings.get("read", 0.0) + time.perf_counter() - t0
    if not bodies:
        return np.zeros(0, dtype=dtype)
    sess = RB._session(session)
    dec = _decode_run(sess, delimiters, bodies, part_bytes, timings)
    t0 = time.perf_counter()
    keep = dec["n_fields"] > 0                  # blank lines
    rows = np.flatnonzero(keep)
    n = len(rows)
    if n == 0:
        return np.zeros(0, dtype=dtype)
    file_of = np.searchsorted(np.asarray(file_base, dtype=np.int64), dec["row_offset"][rows], side="right") - 1
    list_of = np.asarray(file_list, dtype=np.int64)[file_of]
    width = dec["n_fields"][rows].astype(np.int64)
    row_len = np.maximum(width - VX2730_SAMPLES_START, 0)
    n_lists = len(texts)
    list_width = np.zeros(n_lists, dtype=np.int64)
    np.maximum.at(list_width, list_of, width)
    W = list_width[list_of]
    ev_len = np.minimum(np.maximum(W - VX2730_SAMPLES_START, 0), L)
    short = row_len < ev_len                    # a NaN of the padding would be cast to int16: the reference raises
    if np.any(short):
        i = int(np.flatnonzero(short)[0])
        raise ValueError(f"CSV channel list {int(list_of[i])}: rows with {int(width[i])} and {int(W[i])} fields "
                         f"(a row of {int(width[i])} fields has no sample {int(row_len[i])} to fill wave_length {L})")

    meta = dec["meta"][rows]
    pool_off, _ = sess.csv_arena_gather(dec["sample_offset"][rows], row_len.astype(np.int32), download=False)
    rec = np.zeros(n, dtype=RECORDS_DTYPE)
    rec["wave_offset"] = pool_off
    rec["event_length"] = row_len
    rec["record_id"] = np.arange(n, dtype=np.int64)
    rec["polarity"] = "unknown"
    sess.upload_records(rec)
    baseline = sess.baseline_mean(s0, s1)
    end = np.minimum(s1, W - VX2730_SAMPLES_START)
    baseline[(end <= s0) | (end > row_len)] = np.nan   # empty window, or one reaching into a row's padding
    if timings is not None:
        timings["baseline"] = timings.get("baseline", 0.0) + time.perf_counter() - t0

    t0 = time.perf_counter()
    baseline_up = np.full(n, np.nan)
    if upstream_baselines is not None and not streaming:
        counts = np.bincount(list_of, minlength=n_lists)
        for k in range(min(len(upstream_baselines), n_lists)):
            up = upstream_baselines[k]
            if up is not None and counts[k] and len(up) == counts[k]:
                baseline_up[list_of == k] = np.asarray(up, dtype=np.float64)
    board = meta[:, 0].astype(np.int16)
    channel = meta[:, 1].astype(np.int16)
    if streaming:
        polarity = ""
    else:
        polarity = polarity_of(board, channel) if polarity_of is not None else "unknown"
    codes, table = _polarity_codes(polarity, n)
    out = sess.st_pack(L, pool_off, row_len, {
        "baseline": baseline, "baseline_upstream": baseline_up, "timestamp": meta[:, 2],
        "record_id": np.arange(n, dtype=np.int64), "dt": np.int32(dt_ns), "event_length": ev_len,
        "board": board, "channel": channel}, codes, table, source="pool", src_samples=int(row_len.sum()),
        batch_bytes=pack_batch_bytes)
    if timings is not None:
        timings["pack"] = timings.get("pack", 0.0) + time.perf_counter() - t0
    return out


def build_st_waveforms_from_v1725_files(file_paths, wave_length: int | None = None, dt_ns: int = 4, polarity_of=None,
                                        session=None, pack_batch_bytes: int = DEFAULT_PACK_BATCH_BYTES) -> np.ndarray:
    """st_waveforms of V1725 binary files in the reader's order, no sort (waveforms.py:233-290): the header walk on
    the host (records_builder.v1725_index), the rows packed on the device straight from the file bytes.
    L = wave_length, else the longest wave; baseline from the channel header, baseline_upstream NaN."""
    idx_all, bases, blobs = [], [], []
    base = 0
    for path in file_paths or []:
        if not os.path.exists(path):           # the reader logs a warning and goes on
            continue
        blob = np.fromfile(path, dtype=np.uint8)
        idx = RB.v1725_index(blob)
        if len(idx["channel"]) == 0:
            continue
        idx["board"] = np.full(len(idx["channel"]), RB._board_from_path(path), dtype=np.int16)
        idx["payload_offset"] = idx["payload_offset"] // 2 + base
        if blob.size % 2:
            blob = np.concatenate([blob, np.zeros(1, dtype=np.uint8)])
        idx_all.append(idx)
        blobs.append(blob)
        base += blob.size // 2
    if not idx_all:
        return empty_st(wave_length)
    cols = {k: np.concatenate([d[k] for d in idx_all]) for k in idx_all[0]}
    n = len(cols["channel"])
    lengths = cols["n_samples"].astype(np.int64)
    L = int(wave_length) if wave_length is not None else int(lengths.max())
    check_st_layout(L)
    board, channel = cols["board"], cols["channel"].astype(np.int16)
    polarity = polarity_of(board, channel) if polarity_of is not None else "unknown"
    codes, table = _polarity_codes(polarity, n)
    sess = RB._session(session)
    pool = np.concatenate(blobs).view(np.uint16)
    return sess.st_pack(L, cols["payload_offset"], lengths.astype(np.int32), {
        "baseline": cols["baseline"].astype(np.float64), "baseline_upstream": np.nan,
        "timestamp": cols["timestamp"] * np.int64(int(dt_ns) * 1000), "record_id": np.arange(n, dtype=np.int64),
        "dt": np.int32(dt_ns), "event_length": np.minimum(lengths, L), "board": board, "channel": channel},
        codes, table, source="host", src_pool=pool, batch_bytes=pack_batch_bytes)


__all__ = ["build_st_waveforms_from_vx2730_files", "build_st_waveforms_from_v1725_files", "sniff_csv_layout",
           "detect_wave_length", "decode_plan", "check_st_layout", "empty_st", "ST_FIELD_OFFSETS",
           "DEFAULT_WAVE_LENGTH", "DEFAULT_PACK_BATCH_BYTES"]
