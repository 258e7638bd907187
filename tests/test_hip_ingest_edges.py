"""The ingest kernels of wfa_hits.hip (k_csv_newlines / k_csv_lines / k_csv_count / k_csv_decode, k_pool_gather,
k_st_pack) and the V1725 route on the edge tables of tests/ingest_edges_util.py: every comparison is exact, integers and
bytes.  tests/test_ingest_edges_cpu.py proves on the CPU that the tables reach their edges and that the expected values
(decode_reference, v1725_walk, numpy) agree with the oracle and with the reference-made fixture."""

import functools

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests import ingest_edges_util as U
from waveformanalysis_amd import records_builder as RB
from waveformanalysis_amd.device import DeviceSession

pytestmark = pytest.mark.gpu

BUILDERS = ("csv_phases", "csv_tile_seams", "csv_shared_chunks", "csv_newline_blocks", "csv_numbers", "csv_layouts")


@functools.lru_cache(maxsize=None)
def _valid(builder):
    """[(case, expected tables)] of one builder: computed once, shared, never written to."""
    return [(case, U.decode_case(case)) for b, case in U.valid_cases() if b == builder]


def _decode(sess, case, **kw):
    return sess.csv_decode(case["text"], case["delimiter"], case["samples_start"], case["meta_cols"], **kw)


def _assert_tables(got, want, what):
    diff = U.first_difference(got, want)
    for k in U.TABLE_KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {diff}")
    assert got["n_samples"] == want["n_samples"], what


@pytest.mark.parametrize("builder", BUILDERS)
def test_builder_texts_decode(builder):
    with DeviceSession(0) as sess:
        for case, want in _valid(builder):
            assert "error" not in want
            _assert_tables(_decode(sess, case, download_samples=True), want, f"{builder} / {case['name']}")


def test_invalid_texts_are_refused_and_leave_nothing_resident():
    good, want_good = _valid("csv_numbers")[0]
    with DeviceSession(0) as sess:
        for case in U.invalid_cases():
            assert U.decode_case(case) == {"error": case["error"]}
            with pytest.raises(ValueError) as e:
                _decode(sess, case, download_samples=True)
            assert str(e.value) == case["error"], case["name"]
            n = U.sample_count(case)
            assert n > 0
            with pytest.raises(ValueError, match="no decoded CSV samples of that size are resident"):
                sess.pool_gather([0], [1], None, src_samples=n)
            _assert_tables(_decode(sess, good, download_samples=True), want_good, f"after {case['name']}")
            off, pool = sess.pool_gather([0], [want_good["n_samples"]], None, src_samples=want_good["n_samples"])
            np.testing.assert_array_equal(pool, want_good["samples"], err_msg=case["name"])


@pytest.mark.parametrize("sample_base", [0, 1, 7])
def test_valid_texts_through_the_arena(sample_base):
    filler = np.arange(100, 100 + sample_base, dtype=np.uint16)
    with DeviceSession(0) as sess:
        for builder in BUILDERS:
            for case, want in _valid(builder):
                what = f"{builder} / {case['name']} at base {sample_base}"
                sess.csv_arena_reserve(sample_base + want["n_samples"] + 1, keep_filled=False)
                if sample_base:
                    d = sess.csv_decode_part(U.samples_text(filler), 0, ";", 0, ())
                    assert d["n_samples"] == sample_base
                assert sess.csv_arena_filled()[0] == sample_base
                got = sess.csv_decode_part(case["text"], sample_base, case["delimiter"], case["samples_start"], case["meta_cols"])
                shifted = dict(want, sample_offset=want["sample_offset"] + sample_base)
                _off, arena = sess.csv_arena_gather([0, sample_base], [sample_base, want["n_samples"]])
                got["samples"] = arena[sample_base:]
                _assert_tables(got, shifted, what)
                np.testing.assert_array_equal(arena[:sample_base], filler, err_msg=what)
                assert sess.csv_arena_filled()[0] == sample_base + want["n_samples"]


# ---- end to end: files -> records + wave_pool ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_bundle():
    lists = U.vx_files()
    rec, pool = O.build_records_from_vx2730_texts([[t for _n, t in g] for g in lists], default_dt_ns=2)
    rec.flags.writeable = pool.flags.writeable = False
    return lists, rec, pool


def _write(tmp_path, lists):
    paths = []
    for g in lists:
        paths.append([])
        for name, data in g:
            p = tmp_path / name
            p.write_bytes(data)
            paths[-1].append(str(p))
    return paths


@pytest.mark.parametrize("part_bytes", [None, 1500])
def test_edge_files_to_records(tmp_path, part_bytes):
    lists, rec, pool = _edge_bundle()
    widths = {int(n.split("@")[0][6:]) for g in lists for n, _t in g}
    assert min(widths) < 7 and any(7 < w < 47 for w in widths) and max(widths) > 700   # no sample / short of the baseline window / three tiles
    assert np.isnan(rec["baseline"]).any() and (rec["event_length"] < 40).any()
    paths = _write(tmp_path, lists)
    with DeviceSession(0) as sess:
        b = RB.build_records_from_vx2730_files(paths, default_dt_ns=2, session=sess, part_bytes=part_bytes)
    G.assert_struct_equal(b.records, rec, what=f"part_bytes={part_bytes}")
    assert b.wave_pool.tobytes() == pool.tobytes()


def test_fixture_files_to_records(tmp_path):
    """The reference-made bundles of tests/golden/ingest_edges.npz (the oracle stands in where the reference raised)."""
    fx = U.load_fixture()
    raises = set(U.fixture_names(fx, "reference_raises"))
    lists = U.vx_files(max_sample=U.FIXTURE_MAX_SAMPLE, max_bytes=int(fx["csv_max_bytes"]))
    if "csv_bundle" in raises:
        rec, pool = O.build_records_from_vx2730_texts([[t for _n, t in g] for g in lists], default_dt_ns=2)
    else:
        rec, pool = fx["csv_records"], fx["csv_wave_pool"]
    files = U.v1725_file_groups()
    if "v1725_bundle" in raises:
        vrec, vpool = O.build_records_from_v1725_blobs([b for _n, b in files], [RB._board_from_path(n) for n, _b in files], 4)
    else:
        vrec, vpool = fx["v1725_records"], fx["v1725_wave_pool"]
    paths = _write(tmp_path, lists)
    vpaths = [p for g in _write(tmp_path, [files]) for p in g]
    with DeviceSession(0) as sess:
        for part_bytes in (None, 700):
            b = RB.build_records_from_vx2730_files(paths, default_dt_ns=2, session=sess, part_bytes=part_bytes)
            G.assert_struct_equal(b.records, rec, what=f"csv fixture, part_bytes={part_bytes}")
            assert b.wave_pool.tobytes() == np.asarray(pool, dtype=np.uint16).tobytes()
        v = RB.build_records_from_v1725_files(vpaths, 4, session=sess)
        G.assert_struct_equal(v.records, vrec, what="v1725 fixture")
        assert v.wave_pool.tobytes() == np.asarray(vpool, dtype=np.uint16).tobytes()


# ---- k_pool_gather ---------------------------------------------------------------------------------------------------------------
def test_pool_gather_alignment_cases():
    n_src = 6000
    src = np.random.default_rng(8).integers(0, 65536, n_src).astype(np.uint16)
    so, ln, _c = U.gather_cases(n_src)
    want_off, want = U.gather_reference(src, so, ln)
    text = U.samples_text(src)
    refusals = (([n_src - 4], [5]), ([-1], [1]), ([0, n_src], [3, 1]))
    with DeviceSession(0) as sess:
        def check(off, pool, what):
            np.testing.assert_array_equal(off, want_off, err_msg=what)
            assert pool.tobytes() == want.tobytes(), what

        check(*sess.pool_gather(so, ln, src), "host source")
        for bad_so, bad_ln in refusals:
            with pytest.raises(ValueError, match="outside the source pool of 6000 samples"):
                sess.pool_gather(bad_so, bad_ln, src)
        d = sess.csv_decode(text, ";", 0, ())
        assert d["n_samples"] == n_src
        check(*sess.pool_gather(so, ln, None, src_samples=n_src), "csv-resident source")
        for bad_so, bad_ln in refusals:
            with pytest.raises(ValueError, match="outside the source pool of 6000 samples"):
                sess.pool_gather(bad_so, bad_ln, None, src_samples=n_src)
        check(*sess.pool_gather(so, ln, None, src_samples=n_src), "csv-resident source after the refusals")
        sess.csv_arena_reserve(n_src, keep_filled=False)
        assert sess.csv_decode_part(text, 0, ";", 0, ())["n_samples"] == n_src
        check(*sess.csv_arena_gather(so, ln), "arena source")
        for bad_so, bad_ln in refusals:
            with pytest.raises(ValueError, match="outside the source pool of 6000 samples"):
                sess.csv_arena_gather(bad_so, bad_ln)
        # the packed pool is the resident wave_pool: gathered once more from itself through st_pack's pool source below,
        # here read back through a second gather of the whole of it
        off, again = sess.pool_gather([0], [len(want)], want)
        assert again.tobytes() == want.tobytes() and off.tolist() == [0]


# ---- k_st_pack -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "csv", "arena", "pool"])
def test_st_pack_small_wave_lengths(source):
    src = U.st_source()
    cases = U.st_pack_cases(len(src))
    text = U.samples_text(src)
    with DeviceSession(0) as sess:
        if source == "arena":
            sess.csv_arena_reserve(len(src), keep_filled=False)
            assert sess.csv_decode_part(text, 0, ";", 0, ())["n_samples"] == len(src)
        elif source == "csv":
            assert sess.csv_decode(text, ";", 0, ())["n_samples"] == len(src)
        elif source == "pool":
            sess.upload_pool(src)
        for case in cases:
            want = U.st_reference(case, src)
            stride = want.dtype.itemsize
            for batch_bytes in (1, stride, 3 * stride + 5):
                got = sess.st_pack(case["L"], case["src_offset"], case["src_len"], case["columns"], case["polarity_code"],
                                   U.POLARITIES, source=source, src_pool=src if source == "host" else None,
                                   src_samples=len(src), batch_bytes=batch_bytes)
                assert got.dtype == want.dtype
                if got.tobytes() != want.tobytes():
                    bad = [n for n in want.dtype.names if got[n].tobytes() != want[n].tobytes()]
                    rows = np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(len(want))])
                    raise AssertionError(f"L={case['L']} n={case['n']} source={source} batch_bytes={batch_bytes}: fields {bad}, "
                                         f"first differing row {int(rows[0])}")


# ---- V1725 ---------------------------------------------------------------------------------------------------------------------
def test_v1725_streams_to_records(tmp_path):
    cases = U.v1725_cases()
    with DeviceSession(0) as sess:
        for name, (blob, board) in cases.items():
            rec, pool = O.build_records_from_v1725_blobs([blob], [board], 4)
            b = RB.build_records_from_v1725_blob(np.frombuffer(blob, dtype=np.uint8), board, 4, session=sess)
            G.assert_struct_equal(b.records, rec, what=name)
            assert b.wave_pool.tobytes() == pool.tobytes(), name
        assert len(RB.build_records_from_v1725_blob(np.frombuffer(cases["mask_zero_only"][0], dtype=np.uint8), 0, 4, session=sess).records) == 0
        files = U.v1725_file_groups()
        boards = [RB._board_from_path(n) for n, _b in files]
        assert set(boards) == {0, 1}
        rec, pool = O.build_records_from_v1725_blobs([b for _n, b in files], boards, 2)
        assert (rec["event_length"] == 0).sum() >= 6 and len(np.unique(rec["timestamp"])) < len(rec) // 2
        paths = [p for g in _write(tmp_path, [files]) for p in g]
        b = RB.build_records_from_v1725_files(paths + [str(tmp_path / "missing_b1.bin")], 2, session=sess)
        G.assert_struct_equal(b.records, rec, what="files of two boards")
        assert b.wave_pool.tobytes() == pool.tobytes()
