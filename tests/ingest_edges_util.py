"""Inputs that put the ingest stages of wfa_hits.hip (k_csv_newlines / k_csv_lines / k_csv_count / k_csv_decode,
k_pool_gather, k_st_pack) and the host walk host::v1725_index on their tile, chunk and range edges, and an independent
plain-Python statement of what they must give.

`decode_reference` is the contract of wfa_csv_decode_* as include/wfa_hip.h states it, written with bytes.split and a
regex; `v1725_walk` is the DAW_DEMO header walk with int.from_bytes.  Neither shares code with oracle/wfa_oracle.py, so
the expected tables the GPU is compared with are cross-checked on the CPU by something written a second time.
`decode_reference` also carries switches (`MUTANTS`) for the ways the decode kernel could be subtly wrong;
tests/test_ingest_edges_cpu.py proves with them that the builder texts reach their edges and tell right from wrong,
tests/test_hip_ingest_edges.py runs the texts through the kernels.

Every CSV builder returns (cases, counters): cases is a list of dicts {name, text, delimiter, samples_start, meta_cols}
(one decode call each -- a builder needs more than one text wherever it needs more than one column layout), an invalid
case also carries `error`, the message the library must raise; counters says how often each edge was reached.  A
leading filler row sets the absolute offset of a row under test: the decode tile origin is absolute (row_start & ~15).

Everything is deterministic; no GPU, no torch.
"""

from __future__ import annotations

import os
import random
import re

import numpy as np

TILE = 1024       # kCsvTile
LOOK = 32         # kCsvLook
NL_THREAD = 16    # bytes per thread of k_csv_newlines
NL_BLOCK = 4096   # bytes per block of k_csv_newlines
I63 = 2**63 - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_MAX_SAMPLE = 32767   # the reference's readers store samples as int16

MUTANTS = (
    "drop_after_1023",      # the field after a delimiter at tile byte 1023 is dropped
    "look16",               # the lookahead is 16 bytes
    "no_field_base",        # the field index is not carried into the next tile
    "field0_aligned_only",  # field 0 is parsed only when row_start % 16 == 0
    "clip_lo",              # the clip drops the delimiter at byte lo
    "clip_hi",              # the clip drops the delimiter at byte hi - 1
    "keep_cr",              # the '\r' before '\n' stays in the row
    "ignore_sign",          # '-' is skipped, the value stays positive
    "range_65536",          # the range test is > 65536
    "digits_18",            # the digit cap is 18
    "digits_20",            # the digit cap is 20
    "err_field_first",      # the error minimum is taken over (field, row)
)


# ---- the decode contract once more, in plain Python ----------------------------------------------------------------------
def _split_rows(text: bytes, keep_cr: bool = False):
    """[(lo, hi)] of every row: split on '\\n', one trailing '\\r' dropped, a last row without '\\n' counts."""
    parts = text.split(b"\n")
    if parts[-1] == b"":
        parts.pop()   # the text ends with '\n' (or is empty): no row after it
    rows, pos = [], 0
    for p in parts:
        hi = pos + len(p)
        if p.endswith(b"\r") and not keep_cr:
            hi -= 1
        rows.append((pos, hi))
        pos += len(p) + 1
    return rows


def decode_reference(text: bytes, delimiter: str = ";", samples_start: int = 7, meta_cols=(0, 1, 2), mutant: str | None = None):
    """-> {n_fields, row_offset, sample_offset, n_samples, meta, samples}, or {"error": message} with the message of
    the smallest (row, field).  mutant: one of MUTANTS, the same tables as a subtly wrong kernel would give them."""
    assert mutant is None or mutant in MUTANTS, mutant
    delim = delimiter.encode()
    meta_cols = [int(c) for c in meta_cols]
    cap = {"digits_18": 18, "digits_20": 20}.get(mutant, 19)
    number = re.compile(rb"([+-]?)([0-9]{1,%d})" % cap)
    look = 16 if mutant == "look16" else LOOK
    rows = _split_rows(text, keep_cr=(mutant == "keep_cr"))
    n_rows = len(rows)
    n_fields = np.zeros(n_rows, dtype=np.int32)
    row_offset = np.array([lo for lo, _hi in rows], dtype=np.int64).reshape(n_rows)
    meta = np.zeros((n_rows, len(meta_cols)), dtype=np.int64)
    per_row, errors = [], []
    for r, (lo, hi) in enumerate(rows):
        if hi <= lo:
            per_row.append({})
            continue
        body = text[lo:hi]
        fields, starts, pos = [], [], lo
        for f in body.split(delim):
            fields.append(f)
            starts.append(pos)
            pos += len(f) + 1
        if mutant == "clip_lo" and len(fields) > 1 and fields[0] == b"":
            # the delimiter at byte lo is not seen: the row starts with what then looks like one field
            fields[:2] = [delim + fields[1]]
            starts[:2] = [lo]
        if mutant == "clip_hi" and len(fields) > 1 and fields[-1] == b"":
            fields[-2:] = [fields[-2] + delim]
            starts.pop()
        n_fields[r] = len(fields)
        t0 = lo & ~15
        delims = [s - 1 for s in starts[1:]]   # absolute offsets of the row's delimiters
        got = {}
        for i, (f, q) in enumerate(zip(fields, starts)):
            fidx = i
            if i == 0:
                if mutant == "field0_aligned_only" and lo % 16:
                    continue
                tile_start = t0
            else:
                d = q - 1
                tile_start = t0 + (d - t0) // TILE * TILE
                if mutant == "drop_after_1023" and d - tile_start == TILE - 1:
                    continue
                if mutant == "no_field_base":
                    fidx = i - sum(1 for x in delims if x < tile_start)
            is_sample = fidx >= samples_start
            if fidx not in meta_cols and not is_sample:
                continue
            seen = text[q:min(q + len(f), hi, tile_start + TILE + look)]   # (never shorter than f without a mutant)
            if mutant == "clip_hi":
                seen = seen.split(delim)[0]   # the parser still stops at the delimiter the count did not see
            m = number.fullmatch(seen)
            if m is None or int(m.group(2)) > I63:
                errors.append((r, fidx, 1))
                continue
            val = int(m.group(2))
            if m.group(1) == b"-" and mutant != "ignore_sign":
                val = -val
            for j, c in enumerate(meta_cols):
                if c == fidx:
                    meta[r, j] = val
            if is_sample:
                if val < 0 or val > (65536 if mutant == "range_65536" else 65535):
                    errors.append((r, fidx, 2))
                else:
                    got[fidx - samples_start] = val & 0xFFFF
        per_row.append(got)
    if errors:
        key = (lambda e: (e[1], e[0], e[2])) if mutant == "err_field_first" else (lambda e: e)
        r, f, code = min(errors, key=key)
        what = "sample outside the uint16 range" if code == 2 else "not a decimal integer"
        return {"error": f"row {r} field {f}: {what}"}
    counts = np.maximum(n_fields.astype(np.int64) - samples_start, 0)
    sample_offset = np.concatenate(([0], np.cumsum(counts)[:-1])).astype(np.int64) if n_rows else np.zeros(0, np.int64)
    samples = np.zeros(int(counts.sum()), dtype=np.uint16)
    for r, got in enumerate(per_row):
        for k, v in got.items():
            if k < counts[r]:
                samples[sample_offset[r] + k] = v
    return {"n_fields": n_fields, "row_offset": row_offset, "sample_offset": sample_offset, "n_samples": int(counts.sum()),
            "meta": meta, "samples": samples}


TABLE_KEYS = ("n_fields", "row_offset", "sample_offset", "meta", "samples")


def tables_equal(a: dict, b: dict) -> bool:
    if ("error" in a) or ("error" in b):
        return a.get("error") == b.get("error")
    return a["n_samples"] == b["n_samples"] and all(np.array_equal(a[k], b[k]) for k in TABLE_KEYS)


def first_difference(got: dict, want: dict) -> str:
    """Names the first table and row that differ (for failure messages)."""
    if int(got["n_samples"]) != int(want["n_samples"]):
        return f"n_samples {got['n_samples']} != {want['n_samples']}"
    for k in TABLE_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape:
            return f"{k}: shape {g.shape} != {w.shape}"
        if w.size == 0:
            continue
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1)) if len(w) else []
        if len(bad):
            i = int(bad[0])
            if k == "samples":
                row = int(np.searchsorted(want["sample_offset"], i, side="right") - 1)
                return f"samples[{i}] (row {row}, sample {i - int(want['sample_offset'][row])}): {g[i]} != {w[i]}"
            return f"{k}: first differing row {i}: {g[i]} != {w[i]}"
    return ""


def sample_count(case: dict) -> int:
    """What the count pass finds in a text, valid or not: sum over rows of max(n_fields - samples_start, 0)."""
    d = case["delimiter"].encode()
    return sum(max(case["text"][lo:hi].count(d) + 1 - case["samples_start"], 0) for lo, hi in _split_rows(case["text"]) if hi > lo)


def samples_text(src: np.ndarray, per_row: int = 97) -> bytes:
    """A text whose every field is a sample and whose decoded samples are `src` (the CSV-resident and arena sources)."""
    v = [str(int(x)) for x in src]
    return ("\n".join(";".join(v[i:i + per_row]) for i in range(0, len(v), per_row)) + "\n").encode()


def decode_case(case: dict, mutant: str | None = None) -> dict:
    return decode_reference(case["text"], case["delimiter"], case["samples_start"], case["meta_cols"], mutant)


# ---- row makers ---------------------------------------------------------------------------------------------------------
VX = dict(delimiter=";", samples_start=7, meta_cols=(0, 1, 2))   # the VX2730 layout
JUNK = dict(delimiter=";", samples_start=7, meta_cols=(5,))      # five unparsed columns first: a meta field anywhere


def _case(name, text, layout, **extra):
    return {"name": name, "text": bytes(text), **layout, **extra}


def _digits(rng: random.Random, n: int) -> str:
    """A sample of exactly n characters, <= 32767 (leading zeros from six characters on)."""
    if n <= 4:
        return str(rng.randrange(10 ** (n - 1) if n > 1 else 0, 10**n))
    return str(rng.randrange(10000, FIXTURE_MAX_SAMPLE + 1)).rjust(n, "0")


PLAIN = "5"   # head of a row whose every field is a sample


def sized_row(rng: random.Random, n: int, head: str | None = None) -> bytes:
    """A valid row of exactly n bytes.  n >= 40: `head` (default: seven VX2730 meta fields) and samples of 1 to 5
    characters in random order; shorter rows are runs of one-digit fields.  It never ends with a delimiter."""
    assert n >= 1
    if n < 40 and head in (None, PLAIN):
        if n == 1:
            return b"7"
        k = (n + 1) // 2                      # k one-digit fields take 2k - 1 bytes; an even n has a two-digit last field
        f = [str(rng.randrange(10)) for _ in range(k)]
        if n % 2 == 0:
            f[-1] = str(rng.randrange(10, 100))
        row = ";".join(f).encode()
        assert len(row) == n, (len(row), n)
        return row
    if head is None:
        head = f"{rng.randrange(4)};{rng.randrange(16)};{rng.randrange(10**6, 10**13)};{rng.randrange(5000)};7;0x{rng.randrange(2**15):x};1"
    out, left = [head], n - len(head)
    assert left >= 2, (n, head)
    while left > 6:
        d = rng.randrange(1, 6)
        if left - (d + 1) == 1:
            d = d - 1 if d > 1 else d + 1
        out.append(_digits(rng, d))
        left -= d + 1
    out.append(_digits(rng, left - 1))
    row = ";".join(out).encode()
    assert len(row) == n, (len(row), n)
    return row


def _place(text: bytearray, rng: random.Random, phase: int) -> None:
    """Append one filler row so that the next row starts at an offset = phase (mod 16)."""
    n = (phase - len(text) - 1) % 16
    if n == 0:
        n = 16
    text += sized_row(rng, n) + b"\n"
    assert len(text) % 16 == phase


def row_tables(text: bytes, delimiter: str = ";"):
    """[(lo, hi, [absolute delimiter offsets])] of every row (for the counters)."""
    d = delimiter.encode()[0]
    return [(lo, hi, [lo + i for i, ch in enumerate(text[lo:hi]) if ch == d]) for lo, hi in _split_rows(text)]


# ---- CSV builders --------------------------------------------------------------------------------------------------------
PHASE_LENGTHS = (1, 2, 15, 16, 17)


def csv_phases():
    """Every row_start % 16 crossed with row lengths 1, 2, 15, 16, 17 and TILE * k - phase + d, k = 1..3, d = -2..2 (the
    row then ends within two bytes of the end of its k-th tile)."""
    rng = random.Random(1601)
    text = bytearray()
    want = []   # (offset, length) of the rows under test
    for phase in range(16):
        for n in list(PHASE_LENGTHS) + [TILE * k - phase + d for k in (1, 2, 3) for d in (-2, -1, 0, 1, 2)]:
            _place(text, rng, phase)
            want.append((len(text), n))
            text += sized_row(rng, n) + b"\n"
    rows = {lo: (hi, ds) for lo, hi, ds in row_tables(bytes(text))}
    c = {"phases": set(), "lengths": set(), "delim_lane_bytes": set(), "end_tile_bytes": set(), "rows": len(rows)}
    for lo, n in want:
        hi, ds = rows[lo]
        assert hi - lo == n
        c["phases"].add(lo % 16)
        c["lengths"].add((lo % 16, n))
        c["delim_lane_bytes"].update(d % 16 for d in ds)
        c["end_tile_bytes"].add((hi - (lo & ~15)) % TILE)   # 0: the row's last byte is the tile's last byte
    return [_case("phases", text, VX)], c


SEAM_DELIMS = (1007, 1008, 1022, 1023, 1024, 1039)
SEAM_LAST_ENDS = (1023, 1024, 1055)


def csv_tile_seams():
    """Rows built backwards from a tile seam: a delimiter at tile byte D of the row's s-th tile (s = 1, 2, 3, so the
    field index is carried up to twice), followed by each kind of field; with and without fields after it."""
    rng = random.Random(1602)
    vx, junk = bytearray(), bytearray()
    c = {"delim_at": set(), "in_lookahead": 0, "straddle20": 0, "last_field_end": set(), "seams": set(), "rows": 0,
         "sign_at_seam": 0}
    big = ["9223372036854775807", "1234567890123456789", "4000000000000000019"]

    def add(buf, layout, phase, s, D, field, tail):
        _place(buf, rng, phase)
        rel = TILE * (s - 1) + D - phase         # the row-relative offset of the delimiter
        if layout is JUNK:                       # five columns nobody parses, then the meta field as column 5
            head = b"0xdead;ab cd;-;1.5e3;" + b"z" * (rel - 21)
        else:
            head = sized_row(rng, rel)
        row = head + b";" + field.encode() + tail.encode()
        lo = len(buf)
        buf += row + b"\n"
        start = D + 1                            # tile byte of the field's first character
        end = start + len(field) - 1
        c["delim_at"].add(D)
        c["seams"].add(s)
        c["rows"] += 1
        c["in_lookahead"] += D == TILE - 1
        c["straddle20"] += len(field) == 20 and start <= TILE - 1 < end
        c["sign_at_seam"] += field[0] in "+-" and start in (TILE - 1, TILE)
        if not tail:
            c["last_field_end"].add(end)
        assert bytes(buf[lo + rel:lo + rel + 1]) == b";" and (lo & ~15) + TILE * (s - 1) + D == lo + rel

    for phase, seams in ((0, (1, 2, 3)), (9, (1,))):
        for s in seams:
            for D in SEAM_DELIMS:
                k = rng.randrange(3)
                add(vx, VX, phase, s, D, _digits(rng, 1), "")
                add(vx, VX, phase, s, D, _digits(rng, 1), ";1;22;333")
                add(vx, VX, phase, s, D, _digits(rng, 5), ";4")
                add(vx, VX, phase, s, D, "+65535", ";0")
                add(junk, JUNK, phase, s, D, big[k], "")
                add(junk, JUNK, phase, s, D, big[k], ";junk;7;8")
                add(junk, JUNK, phase, s, D, "-" + big[(k + 1) % 3], ";x;9")
            # the row's last field ending at tile bytes 1023, 1024 and 1055 (the last byte of the lookahead)
            add(vx, VX, phase, s, 1022, _digits(rng, 1), "")
            add(vx, VX, phase, s, 1023, _digits(rng, 1), "")
            add(vx, VX, phase, s, 1039, _digits(rng, 16), "")
            add(vx, VX, phase, s, 1023, _digits(rng, 19), ";3")   # 19 characters, all of them in the lookahead
            add(junk, JUNK, phase, s, 1035, "-" + big[0], "")
            add(junk, JUNK, phase, s, 1023, "+" + big[1], "")
    return [_case("seams_vx", vx, VX), _case("seams_meta", junk, JUNK)], c


ALL = dict(delimiter=";", samples_start=0, meta_cols=())   # every field is a sample


def csv_shared_chunks():
    """Rows that start and end inside one 16-byte chunk, rows that share a chunk, line ends on chunk seams."""
    crlf = b"1;2;3;4;5;6;7;8\r\n" + b"11;12;13;14;15\r\n" + b"21;22;23;24;2\r\n9\r\n"
    cases = [
        _case("sixteen_newlines", b"\n" * 16, ALL),
        _case("eight_rows_one_chunk", b"1\n2\n3\n4\n5\n6\n7\n8\n", ALL),
        _case("crlf_on_chunk_seam", crlf, ALL),
        _case("lone_cr_row", b"1;2\n\r\n3;4\n\r\n", ALL),
        _case("no_newline", b"1;2;3", ALL),
        _case("one_byte", b"7", ALL),
        _case("one_newline", b"\n", ALL),
        _case("one_cr", b"\r", ALL),
        _case("bytes_15", b"1;2;3;4;5;6;7;8", ALL),
        _case("bytes_16", b"1;2;3;4;5;6;7;88", ALL),
        _case("bytes_17", b"1;2;3;4;5;6;7;8;9", ALL),
        _case("rows_inside_one_chunk", b"100;200\n3;4\n5\n\n66;77;88;99\n1;2;3;4;5;6;7;8;9;10;11;12\n", ALL),
    ]
    c = {"sizes": {len(x["text"]) for x in cases}, "max_rows_per_chunk": 0, "cr_at_15": 0, "empty_rows": 0}
    for x in cases:
        t = x["text"]
        rows = _split_rows(t)
        c["empty_rows"] += sum(hi == lo for lo, hi in rows)
        per_chunk = {}
        for lo, _hi in rows:
            per_chunk[lo // 16] = per_chunk.get(lo // 16, 0) + 1
        c["max_rows_per_chunk"] = max([c["max_rows_per_chunk"], *per_chunk.values()])
        c["cr_at_15"] += sum(1 for i in range(15, len(t) - 1, 16) if t[i:i + 2] == b"\r\n")
    return cases, c


def _filled(rng: random.Random, n: int, end_nl: bool) -> bytearray:
    """n bytes of short rows; the last byte is '\\n' iff end_nl."""
    text = bytearray()
    body = n - 1 if end_nl else n
    while body - len(text) > 60:
        text += sized_row(rng, rng.randrange(1, 40)) + b"\n"
    text += sized_row(rng, body - len(text), PLAIN)
    if end_nl:
        text += b"\n"
    assert len(text) == n
    return text


def csv_newline_blocks():
    """k_csv_newlines: 16 bytes per thread, 4096 per block, a scan over the block counts."""
    rng = random.Random(1604)
    a = _filled(rng, NL_BLOCK, True)                                  # 4096 bytes, '\n' at 4095
    b = _filled(rng, NL_BLOCK, True) + b"\n"                          # 4097 bytes, '\n' at 4095 and 4096
    c_ = _filled(rng, NL_BLOCK, True) + b"7"                          # 4097 bytes, last byte no '\n'
    d = _filled(rng, NL_BLOCK, False)                                 # 4096 bytes, last byte no '\n'
    e = _filled(rng, NL_BLOCK - 1, False) + b";" + b"\n" + _filled(rng, 50, True)   # (never decoded: n_fields only)
    long_row = bytearray(sized_row(rng, 9000, PLAIN) + b"\n" + _filled(rng, 300, False))  # blocks 0 and 1 hold no '\n'
    sixteen = _filled(rng, 160, True) + b"\n" * 16 + _filled(rng, NL_BLOCK - 176, True) + b"\n" * 16 + b"5;6\n"
    cases = [_case("len4096_nl_last", a, ALL), _case("len4097_nl_4095_4096", b, ALL),
             _case("len4097_no_final_nl", c_, ALL), _case("len4096_no_final_nl", d, ALL),
             _case("row_over_two_blocks", long_row, ALL), _case("sixteen_nl_in_a_thread", sixteen, ALL),
             _case("nl_4096_after_delim", e, dict(delimiter=";", samples_start=10**6, meta_cols=()))]
    c = {"sizes": set(), "nl_at": set(), "empty_blocks": 0, "full_threads": 0, "final_nl": set()}
    for x in cases:
        t = x["text"]
        c["sizes"].add(len(t))
        c["final_nl"].add(t.endswith(b"\n"))
        c["nl_at"].update(i for i in (NL_BLOCK - 1, NL_BLOCK) if t[i:i + 1] == b"\n")
        c["empty_blocks"] += sum(1 for k in range(0, len(t) - NL_BLOCK + 1, NL_BLOCK) if b"\n" not in t[k:k + NL_BLOCK])
        c["full_threads"] += sum(1 for k in range(0, len(t), 16) if t[k:k + 16] == b"\n" * 16)
    return cases, c


NUM = dict(delimiter=";", samples_start=3, meta_cols=(0, 1, 2))


def csv_numbers():
    """The integer parser at its limits -> (valid cases, invalid cases, counters)."""
    valid = _case("numbers_valid", b"-3;-7;9223372036854775807;0;00;007;+5;-0;65535\n"
                                   b"1;2;-9223372036854775807;1;65535;0;+0;-00;00000\n"
                                   b"-32768;+15;+" + b"1".rjust(19, b"0") + b";" + b"65535".rjust(19, b"0") + b";+" +
                                   b"65535".rjust(18, b"0") + b";2;3;4;5\n", NUM)
    ok = b"1;2;3;4;5\n"

    def bad(name, row, field, what="not a decimal integer"):
        return _case("bad_" + name, ok + row + b"\n" + ok, NUM, error=f"row 1 field {field}: {what}")

    rng = random.Random(1605)
    rge = "sample outside the uint16 range"
    invalid = [
        bad("65536", b"1;2;3;65536", 3, rge), bad("minus_1", b"1;2;3;4;-1", 4, rge),
        bad("2_63", b"1;2;9223372036854775808;4", 2), bad("minus_2_63", b"1;2;-9223372036854775808;4", 2),
        bad("19_nines", b"1;2;9999999999999999999;4", 2),
        bad("20_digits_meta", b"1;00000000000000000001;3;4", 1), bad("20_digits_sample", b"1;2;3;00000000000000000001", 3),
        bad("19_digit_sample", b"1;2;3;1000000000000000000", 3, rge),
        bad("minus", b"1;2;3;-", 3), bad("plus", b"1;2;3;+;5", 3), bad("minus_minus", b"1;2;3;--1", 3),
        bad("inner_sign", b"1;2;3;1-2", 3), bad("blank_after", b"1;2;3;1 ;5", 3), bad("blank_before", b"1;2;3; 1", 3),
        bad("hex", b"1;2;3;0x1f", 3), bad("underscore", b"1;2;3;1_0", 3), bad("empty_meta", b"1;;3;4", 1),
        bad("empty_sample", b"1;2;3;;5", 3), bad("trailing_delimiter", b"1;2;3;4;", 4),
        bad("sign_after_digits", b"1;2;3;5+", 3), bad("nul_byte", b"1;2;3;5\x00", 3),
    ]
    # several errors: the winner sits in a later tile of an earlier row than the others
    long_bad = bytearray(sized_row(rng, 2500, "1;2;3"))
    cut = long_bad.rfind(b";", 0, 2300)
    nxt = long_bad.find(b";", cut + 1)
    long_bad[cut + 1:nxt] = b"x"
    f_long = long_bad[:cut + 1].count(b";")
    multi_a = bytes(long_bad) + b"\n" + b"1;2;3;70000\n" + b"x;2;3;4\n"
    invalid.append(_case("bad_multi_a", multi_a, NUM, error=f"row 0 field {f_long}: not a decimal integer"))
    long2 = bytearray(sized_row(rng, 3300, "1;2;3"))
    cut2 = long2.rfind(b";", 0, 3200)
    nxt2 = long2.find(b";", cut2 + 1)
    long2[cut2 + 1:nxt2] = b"65536"
    f2 = long2[:cut2 + 1].count(b";")
    cut3 = long2.rfind(b";", 0, 1500)   # and a syntax error in an earlier tile of the same row: the smaller field wins
    nxt3 = long2.find(b";", cut3 + 1)
    two = bytearray(long2)
    two[cut3 + 1:nxt3] = b"-"
    f3 = two[:cut3 + 1].count(b";")
    multi_b = ok * 3 + bytes(long2) + b"\n" + ok + b"1;y;3;4\n" + b";2;3;4\n"
    multi_c = ok * 2 + bytes(two) + b"\n" + b"q;2;3;4\n"
    invalid.append(_case("bad_multi_b", multi_b, NUM, error=f"row 3 field {f2}: sample outside the uint16 range"))
    invalid.append(_case("bad_multi_c", multi_c, NUM, error=f"row 2 field {f3}: not a decimal integer"))
    c = {"valid_rows": 3, "invalid": len(invalid), "multi": 3,
         "winner_tile": [(cut + 1) // TILE, (cut2 + 1) // TILE, (cut3 + 1) // TILE]}
    return [valid], invalid, c


def csv_layouts():
    """Column layouts and delimiters other than the VX2730 default."""
    body = b"1;2;3;4;5;6;7;8;9;10\n11;12\n13\n21;22;23;24;25;26;27;28;29\n"
    cases = [
        _case("all_samples", b"1;2;3\n4;5\n\n6\n", ALL),
        _case("samples_start_above_every_row", body, dict(delimiter=";", samples_start=50, meta_cols=(0, 1, 2))),
        _case("rows_shorter_than_meta", body, dict(delimiter=";", samples_start=7, meta_cols=(0, 1, 2, 5))),
        _case("comma", body.replace(b";", b","), dict(delimiter=",", samples_start=7, meta_cols=(0, 1, 2))),
        _case("tab", body.replace(b";", b"\t"), dict(delimiter="\t", samples_start=2, meta_cols=(0, 1))),
        _case("space", body.replace(b";", b" "), dict(delimiter=" ", samples_start=1, meta_cols=(0,))),
        _case("meta_decreasing", body, dict(delimiter=";", samples_start=7, meta_cols=(2, 1, 0))),
        _case("meta_repeated", body, dict(delimiter=";", samples_start=7, meta_cols=(2, 2, 0))),
        _case("eight_meta", body, dict(delimiter=";", samples_start=8, meta_cols=(7, 6, 5, 4, 3, 2, 1, 0))),
        _case("leading_delimiter", b";5;6\n;7\n1;8\n", dict(delimiter=";", samples_start=1, meta_cols=())),
        _case("unparsed_trailing_delimiter", b"1;2;\n3;\n4;5;6;\n", dict(delimiter=";", samples_start=9, meta_cols=(0,))),
        _case("other_delimiter_is_text", b"1;2,3;4\n", dict(delimiter=";", samples_start=2, meta_cols=(0,))),
    ]
    c = {"delimiters": {x["delimiter"] for x in cases},
         "non_increasing": sum(1 for x in cases if any(a >= b for a, b in zip(x["meta_cols"], x["meta_cols"][1:]))),
         "missing_meta": sum(1 for x in cases if x["meta_cols"] and
                             min(len(r.split(x["delimiter"].encode())) for r in x["text"].split(b"\n") if r) <= max(x["meta_cols"]))}
    return cases, c


def valid_cases():
    """Every valid case of every builder, as [(builder name, case)]."""
    out = []
    for name, fn in (("csv_phases", csv_phases), ("csv_tile_seams", csv_tile_seams), ("csv_shared_chunks", csv_shared_chunks),
                     ("csv_newline_blocks", csv_newline_blocks), ("csv_layouts", csv_layouts)):
        out += [(name, x) for x in fn()[0]]
    out += [("csv_numbers", x) for x in csv_numbers()[0]]
    return out


def invalid_cases():
    return csv_numbers()[1]


def vx_rows_by_width(max_sample: int | None = None):
    """The VX2730-layout rows of csv_phases and csv_tile_seams with at least three fields, grouped by field count:
    {n_fields: [row bytes]} in text order (a reference file is one 2-D array: one width per file).  max_sample drops
    rows holding a larger sample."""
    out: dict[int, list[bytes]] = {}
    for text in (csv_phases()[0][0]["text"], csv_tile_seams()[0][0]["text"]):
        for lo, hi in _split_rows(text):
            f = text[lo:hi].split(b";")
            if len(f) < 3:
                continue
            if max_sample is not None and any(int(x) > max_sample for x in f[7:]):
                continue
            out.setdefault(len(f), []).append(text[lo:hi])
    return out


VX_HEADER = b"BOARD;CHANNEL;TIMETAG;ENERGY;ENERGYSHORT;FLAGS;PROBE_CODE;SAMPLES\n"


def vx_files(max_sample: int | None = None, max_bytes: int | None = None):
    """-> per-channel lists of (file name, file bytes): one file per width, widths dealt over three channel lists; the
    first file of a list carries the header row.  Widths 8..46 give records shorter than the 40-sample baseline
    window, widths 3..7 records with no sample at all (baseline NaN).  max_bytes keeps the widths with the fewest
    bytes first until the budget is used (the fixture)."""
    groups = vx_rows_by_width(max_sample)
    widths = sorted(groups)
    if max_bytes is not None:
        keep, used = [], 0
        for w in sorted(widths, key=lambda w: (sum(map(len, groups[w])), w)):
            size = sum(map(len, groups[w])) + len(groups[w])
            if used + size <= max_bytes:
                keep.append(w)
                used += size
        widths = sorted(keep)
    lists = [[], [], []]
    for k, w in enumerate(widths):
        g = lists[k % 3]
        body = b"\n".join(groups[w]) + (b"\n" if k % 4 else b"")   # every fourth file has no final newline
        g.append((f"edge_w{w}@CH{k % 3}_{len(g)}.CSV", (VX_HEADER if not g else b"") + body))
    return lists


# ---- V1725 DAW_DEMO streams ----------------------------------------------------------------------------------------------
def v1725_stream(events, h3_noise: int = 0, size_high_bits: int = 0, header_fill: int = 0) -> bytes:
    """DAW_DEMO bytes of [(mask, [(timestamp, trunc, baseline, samples), ...])], one wave per set mask bit in channel
    order.  The knobs set bits the walker must ignore: h3_noise = bits of the channel header's byte 3 other than bit 6,
    size_high_bits = the two bits above the 22-bit size, header_fill = the event-header bytes other than 4 and 11."""
    out = bytearray()
    for mask, waves in events:
        assert bin(mask).count("1") == len(waves) and 0 <= mask < 1 << 16
        eh = bytearray([header_fill & 0xFF] * 16)
        eh[4], eh[11] = mask & 0xFF, mask >> 8
        out += eh
        for ts, trunc, baseline, samples in waves:
            s = np.asarray(samples, dtype=np.int16)
            assert len(s) % 2 == 0 and 0 <= ts < 1 << 48
            size = (3 + len(s) // 2) | ((size_high_bits & 3) << 22)
            h = bytearray(12)
            h[0:3] = size.to_bytes(3, "little")
            h[3] = (h3_noise & 0xBF) | (0x40 if trunc else 0)
            h[4:10] = int(ts).to_bytes(6, "little")
            h[10:12] = int(baseline).to_bytes(2, "little")
            out += h + s.astype("<i2").tobytes()
    return bytes(out)


def v1725_walk(blob: bytes):
    """[(channel, timestamp, trunc, baseline, payload_offset, n_samples)] of every complete wave; a short event header,
    channel header or payload ends the stream.  Raises ValueError for a channel block of fewer than 3 words."""
    blob = bytes(blob)
    n, pos, out = len(blob), 0, []
    while pos + 16 <= n:
        mask = blob[pos + 4] + 256 * blob[pos + 11]
        pos += 16
        for ch in range(16):
            if not mask & (1 << ch):
                continue
            if pos + 12 > n:
                return out
            words = int.from_bytes(blob[pos:pos + 3], "little") % (1 << 22)
            if words < 3:
                raise ValueError(f"V1725 channel size {words} < 3 words at byte {pos}")
            size = 4 * (words - 3)
            if pos + 12 + size > n:
                return out
            out.append((ch, int.from_bytes(blob[pos + 4:pos + 10], "little"), (blob[pos + 3] & 0x40) >> 6,
                        int.from_bytes(blob[pos + 10:pos + 12], "little"), pos + 12, size // 2))
            pos += 12 + size
    return out


def prefix_sweep_digest(blob: bytes) -> dict:
    """What `host_check v1725-prefixes` prints: the plain walk over every prefix 0..n, one running 64-bit digest over
    every column of every wave."""
    m = (1 << 64) - 1
    d = total = 0
    for cut in range(len(blob) + 1):
        waves = v1725_walk(blob[:cut])
        total += len(waves)
        for k, (ch, ts, trunc, bl, off, ns) in enumerate(waves):
            d = (d * 1000003 + (ch + 31 * ts + 131 * trunc + 8191 * bl + 65537 * off + 1000033 * ns) * (k + 1)) & m
    return {"prefixes": len(blob) + 1, "waves": total, "digest": d}


def v1725_cases():
    """{name: (blob, board)}: the walker's edges.  Payload samples keep their int16 bit pattern in the pool."""
    rng = np.random.default_rng(1725)

    def wave(n, ts, trunc=0, bl=None):
        return (ts, trunc, int(rng.integers(0, 65536)) if bl is None else bl, rng.integers(-32768, 32768, n).astype(np.int16))

    top = (1 << 48) - 1
    mixed = [(0x0005, [wave(6, 100), wave(10, 100)]), (0, []), (0x8100, [wave(4, 50, 1), wave(2, top, 0, 65535)]),
             (0x0002, [wave(0, 70)]), (0xFFFF, [wave(2 * (k % 3), 60 + k % 2, k % 2) for k in range(16)]),
             (0x0200, [wave(18, 0, 1, 0)]), (0x0041, [wave(20, 9), wave(8, 9)])]
    one_ts = [(0x00F0, [wave(4, 777) for _ in range(4)]), (0x0F00, [wave(2, 777) for _ in range(4)]),
              (0x000F, [wave(0, 777), wave(6, 777), wave(0, 777), wave(2, 777)])]
    high = [(0xFF00, [wave(2 + 2 * k, 1000 - k) for k in range(8)])]
    cases = {
        "mixed": (v1725_stream(mixed), 0),
        "mixed_noise": (v1725_stream(mixed, h3_noise=0xBF, size_high_bits=3, header_fill=0xFF), 1),
        "one_timestamp": (v1725_stream(one_ts, h3_noise=0x80, header_fill=0x5A), 0),
        "channels_8_15": (v1725_stream(high, size_high_bits=2), 1),
        "mask_zero_only": (v1725_stream([(0, []), (0, [])], header_fill=0xEE), 0),
        "odd_length": (v1725_stream(mixed[:3]) + b"\x7f", 1),
        "zero_sample_waves": (v1725_stream([(0x0003, [wave(0, 5), wave(0, 4)]), (0x8000, [wave(0, 4)])]), 0),
        "cut_in_channel_header": (v1725_stream(mixed)[:16 + 12 + 12 + 5], 0),
        "cut_in_payload": (v1725_stream(one_ts)[:-3], 1),
    }
    return cases


def v1725_prefix_stream() -> bytes:
    """About 600 bytes whose prefixes end in every kind of place: event header, channel header, payload, 0-sample wave."""
    cases = v1725_cases()
    blob = cases["mixed_noise"][0]
    assert 500 <= len(blob) <= 700, len(blob)
    return blob


def v1725_file_groups():
    """-> [(file name, blob)] of two boards (the name carries _b<N>) for build_records_from_v1725_files."""
    cases = v1725_cases()
    order = ("mixed", "mixed_noise", "one_timestamp", "channels_8_15", "odd_length", "zero_sample_waves", "mask_zero_only",
             "cut_in_payload")
    return [(f"edges_b{cases[k][1]}_seg{i}.bin", cases[k][0]) for i, k in enumerate(order)]


# ---- k_pool_gather ---------------------------------------------------------------------------------------------------------
GATHER_LENGTHS = (0, 1, 7, 8, 9, 1023, 1024, 1025, 1031, -3)   # 1024 = 128 lanes x 8 samples; 1031 = + a 7-sample tail


def gather_cases(src_samples: int = 6000):
    """-> (src_offset, length, counters).  Every length x source offset mod 8 in (0, 1, 7) x destination offset mod 8 in
    0..7: a record of 8 - (cursor % 8) + want_dst_mod samples in front of each record under test sets the destination."""
    so, ln = [], []
    cursor = 0
    c = {"co_aligned": 0, "co_aligned_tail": 0, "co_aligned_no_tail": 0, "records": 0, "dst_mods": set(), "negative": 0}
    k = 0
    combos = [(length, smod, dmod) for length in GATHER_LENGTHS for smod in (0, 1, 7) for dmod in range(8)]
    combos += [(length, 0, 0) for length in GATHER_LENGTHS if length > 0] * 3   # co-aligned: far more than chance gives
    if True:
        if True:
            for length, smod, dmod in combos:
                pad = (dmod - cursor) % 8           # 0..7 samples: a record of its own
                so.append((k * 37) % 1000)
                ln.append(pad)
                cursor += pad
                base = 8 * ((k * 53) % ((src_samples - 1040) // 8)) + smod
                so.append(base)
                ln.append(length)
                eff = max(length, 0)
                c["records"] += 1
                c["dst_mods"].add(cursor % 8)
                c["negative"] += length < 0
                if eff > 0 and smod == 0 and cursor % 8 == 0:
                    c["co_aligned"] += 1
                    c["co_aligned_tail" if eff % 8 else "co_aligned_no_tail"] += 1
                cursor += eff
                k += 1
    # the last record ends on the last sample of the source
    so.append(src_samples - 9)
    ln.append(9)
    return np.array(so, dtype=np.int64), np.array(ln, dtype=np.int32), c


def gather_reference(src: np.ndarray, so, ln):
    n = np.maximum(ln, 0).astype(np.int64)
    off = np.concatenate(([0], np.cumsum(n)[:-1])).astype(np.int64)
    parts = [src[int(s):int(s) + int(k)] for s, k in zip(so, n) if k > 0]
    return off, (np.concatenate(parts) if parts else np.zeros(0, np.uint16))


# ---- k_st_pack ---------------------------------------------------------------------------------------------------------------
ST_LENGTHS = (0, 1, 3, 7, 8, 9, 16, 61)
ST_ROWS = (1, 2, 37)
ST_HEADER = 76
POLARITIES = ("unknown", "positive", "negative")


def st_pack_cases(src_samples: int = 4001):
    """-> [case]: wave_length L x row count; a case holds src_offset, src_len, the header columns, the polarity codes and
    `kinds`, the number of 16-byte chunks of each kind over the whole table (fast: eight samples of one row; slow:
    header bytes or a row seam; pad: the chunk holding the bytes after the last row).  src_samples is odd and the last
    row's slice ends on the source's last sample."""
    assert src_samples % 2 == 1
    out = []
    for L in ST_LENGTHS:
        for n in ST_ROWS:
            rng = np.random.default_rng(1000 * L + n)
            lens = np.array([(L, L + 9, 0, 1, L - 1, L + 1)[i % 6] for i in range(n)], dtype=np.int32)
            if n > 2:
                lens[n // 2] = -2                                   # a negative length packs nothing
            off = rng.integers(0, src_samples - (L + 9), n).astype(np.int64)
            off[::2] &= ~1                                          # even and odd source offsets
            off[1::2] |= 1
            eff = int(min(max(int(lens[-1]), 0), L))
            off[-1] = src_samples - eff                             # ends on the last sample of an odd-sized source
            if n > 3:
                assert lens[2] == 0
                off[2] = -5                                         # a row of length 0 may carry any offset
            cols = {"baseline": rng.normal(8000, 50, n), "baseline_upstream": np.where(np.arange(n) % 3, rng.normal(0, 1, n), np.nan),
                    "timestamp": rng.integers(-2**62, 2**62, n), "record_id": np.arange(n, dtype=np.int64)[::-1] * 3,
                    "dt": rng.integers(1, 9, n).astype(np.int32), "event_length": rng.integers(0, 2**31 - 1, n).astype(np.int32),
                    "board": rng.integers(-32768, 32768, n).astype(np.int16), "channel": rng.integers(-32768, 32768, n).astype(np.int16)}
            stride = ST_HEADER + 2 * L
            kinds = {"fast": 0, "slow": 0, "pad": 0, "phases": set()}
            for b in range(0, n * stride, 16):
                p = b % stride
                if b + 16 > n * stride:
                    kinds["pad"] += 1
                elif p >= ST_HEADER and p + 16 <= stride:
                    kinds["fast"] += 1
                else:
                    kinds["slow"] += 1
            kinds["phases"] = {(r * stride) % 16 for r in range(n)}
            out.append({"L": L, "n": n, "src_offset": off, "src_len": lens, "columns": cols,
                        "polarity_code": (np.arange(n) % 3).astype(np.uint8), "kinds": kinds, "src_samples": src_samples})
    return out


def st_source(src_samples: int = 4001) -> np.ndarray:
    return np.random.default_rng(76).integers(0, 65536, src_samples).astype(np.uint16)


def st_reference(case: dict, src: np.ndarray) -> np.ndarray:
    """The rows by numpy structured assignment into create_record_dtype(L)."""
    from waveformanalysis_amd.dtypes import create_record_dtype

    L, n = case["L"], case["n"]
    want = np.zeros(n, dtype=create_record_dtype(L))
    for k, v in case["columns"].items():
        want[k] = v
    want["polarity"] = np.array(POLARITIES)[case["polarity_code"]]
    for r in range(n):
        m = int(min(max(int(case["src_len"][r]), 0), L))
        if m:
            o = int(case["src_offset"][r])
            want["wave"][r, :m] = src[o:o + m].view(np.int16)
    return want


# ---- the reference-made fixture --------------------------------------------------------------------------------------------
FIXTURE = os.path.join(GOLDEN, "ingest_edges.npz")


def load_fixture() -> dict:
    z = np.load(FIXTURE, allow_pickle=False)
    return {k: z[k] for k in z.files}


def fixture_names(fx: dict, key: str) -> list[str]:
    raw = bytes(fx[key]).decode()
    return raw.split("\n") if raw else []
