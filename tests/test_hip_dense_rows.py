"""Dense rows unpacked on the device (wfa_upload_dense_rows / k_dense_unpack) and kept resident between the dense
plugins: exact pool content over shapes x layouts x batch sizes x element types, negative int16 samples, the five-plugin
chain and the filtered chain against the host route (DeviceSession.dense_rows = False), and the layouts that fall back."""

import numpy as np
import pytest

from tests import golden_util as G
from waveformanalysis_amd import _lib, dense
from waveformanalysis_amd.device import DeviceSession, default_pool
from waveformanalysis_amd.dtypes import create_record_dtype
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import (
    HipBasicFeaturesPlugin,
    HipFilteredWaveformsPlugin,
    HipHitFinderPlugin,
    HipThresholdHitPlugin,
    HipWaveformWidthIntegralPlugin,
    HipWaveformWidthPlugin,
)

pytestmark = pytest.mark.gpu

SHAPES = [(0, 5), (1, 1), (3, 7), (5, 8), (4, 9), (7, 33), (64, 800)]
ELEMS = {"<i2": 2, "<u2": 2, "<f4": 4}
F32_SPECIALS = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff],
                        dtype=np.uint32)


@pytest.fixture(scope="module")
def sess():
    with DeviceSession(0) as s:
        yield s


def _dtype(kind, L, elem):
    """st: the ST_WAVEFORM_DTYPE fields with `wave` at byte 76; first: `wave` at byte 0; shifted: one element-sized field
    before `wave`, stride (1 + L) elements -- for 16-bit samples and even L the rows alternate between 4-byte aligned
    and not."""
    if kind == "st":
        descr = [(n, (elem, (L,)) if n == "wave" else create_record_dtype(L).fields[n][0]) for n in create_record_dtype(L).names]
        dt = np.dtype(descr)
        assert dt.fields["wave"][1] == 76 and dt.itemsize == 76 + ELEMS[elem] * L
        return dt
    if kind == "first":
        return np.dtype([("wave", elem, (L,))])
    dt = np.dtype([("pad", "<i2" if ELEMS[elem] == 2 else "<i4"), ("wave", elem, (L,))])
    assert dt.fields["wave"][1] == ELEMS[elem] and dt.itemsize == ELEMS[elem] * (1 + L)
    return dt


def _fill(data, elem, rng):
    """Every byte of the rows random (the fields around `wave` must not leak into the pool), then `wave` over the whole
    range of its type with the extremes placed at the two ends of the array."""
    n, L = data["wave"].shape
    data.view(np.uint8).reshape(-1)[:] = rng.integers(0, 256, data.nbytes, dtype=np.uint8)
    if elem == "<f4":
        bits = rng.integers(0, 2**32, (n, L), dtype=np.uint64).astype(np.uint32)
        flat = bits.reshape(-1)
        k = min(len(F32_SPECIALS), flat.size)
        flat[rng.permutation(flat.size)[:k]] = F32_SPECIALS[:k]
        data["wave"] = bits.view(np.float32)
        assert np.array_equal(data["wave"].view(np.uint32), bits)  # the assignment itself kept every bit
        return
    hi = 32768 if elem == "<i2" else 65536
    wave = rng.integers(0, hi, (n, L)).astype(elem)
    if wave.size:
        wave.reshape(-1)[0] = hi - 1
        wave.reshape(-1)[-1] = 0 if wave.size > 1 else hi - 1
    data["wave"] = wave


def _readback(sess, n, L, elem):
    """The device pool as an (n, L) matrix of bit patterns: the uint16 pool through view_gather (WAVES, U16) with the
    records (r L, L), the float32 pool through download_filtered."""
    if elem == "<f4":
        return sess.download_filtered().view(np.uint32).reshape(n, L)
    rec = np.zeros(n, dtype=dense.DENSE_RECORD_DTYPE)
    rec["record_id"] = np.arange(n)
    rec["wave_offset"] = np.arange(n, dtype=np.int64) * L
    rec["event_length"] = L
    sess.upload_records(rec)
    return sess.view_gather(np.arange(n), mode="waves", source="u16", out_dtype=np.uint16, pad_len=L)


@pytest.mark.parametrize("kind", ["st", "first", "shifted"])
@pytest.mark.parametrize("n,L", SHAPES)
def test_pool_holds_exactly_the_rows(sess, n, L, kind):
    rng = np.random.default_rng(1000 * n + L)
    for elem in ELEMS:
        data = np.zeros(n, dtype=_dtype(kind, L, elem))
        _fill(data, elem, rng)
        want = np.ascontiguousarray(data["wave"]).view(np.uint16 if ELEMS[elem] == 2 else np.uint32)
        row = data.dtype.itemsize
        for batch in (1, 3 * row, 1 << 30):  # one row per batch / three (n = 7: a partial last batch) / everything
            before = sess.uploads
            sess.upload_dense(data, batch_bytes=batch)
            assert sess.uploads == before + 1 and sess.n_samples == n * L and sess.first_negative_row == -1
            if n == 0:
                continue
            got = _readback(sess, n, L, elem)
            assert np.array_equal(got, want), (elem, batch, np.argwhere(got != want)[:4])


def _st(n, L, rng):
    st = np.zeros(n, dtype=create_record_dtype(L))
    st["wave"] = rng.integers(0, 32768, (n, L)).astype(np.int16)
    return st


TEXT = r"st_waveforms\['wave'\] holds negative samples; the HIP backend reads unsigned ADC codes"


@pytest.mark.parametrize("spots,first", [([(0, 0)], 0), ([(6, 32)], 6), ([(4, 5)], 4), ([(6, 32), (4, 5), (5, 0)], 4)])
def test_negative_samples_are_refused(sess, spots, first):
    n, L = 7, 33
    st = _st(n, L, np.random.default_rng(3))
    for r, j in spots:
        st["wave"][r, j] = -1
    batch = 3 * st.dtype.itemsize  # rows 3..5 are the second batch
    with pytest.raises(ValueError, match=TEXT):
        sess.ensure_dense(st)
    with pytest.raises(ValueError, match=TEXT):
        sess.upload_dense(st, batch_bytes=batch)
    assert sess.first_negative_row == first and not sess.holds_dense(st)
    with pytest.raises(_lib.WfaError, match="upload a pool before the records"):  # no pool is left on the device
        sess.upload_records(dense.dense_records(st, L))
    # the same bit patterns as uint16 rows are samples like any other
    as_u16 = st.view(np.dtype([(k, ("<u2", (L,)) if k == "wave" else st.dtype.fields[k][0]) for k in st.dtype.names]))
    sess.upload_dense(as_u16, batch_bytes=batch)
    assert np.array_equal(_readback(sess, n, L, "<u2"), st["wave"].view(np.uint16))
    # and a valid int16 upload on the same session succeeds
    good = _st(n, L, np.random.default_rng(4))
    assert sess.ensure_dense(good) and sess.holds_dense(good) and sess.first_negative_row == -1
    assert np.array_equal(_readback(sess, n, L, "<i2"), good["wave"].view(np.uint16))


def test_arguments_are_checked_before_any_launch(sess):
    lib, h = sess._lib, sess._h
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    for args in ((p, -1, 16, 0, 4, 0), (p, 2, 16, 0, -1, 0), (p, 2, 16, -2, 4, 0), (p, 2, 16, 10, 4, 0), (p, 2, 16, 1, 4, 0),
                 (p, 2, 15, 0, 4, 0), (p, 2, 16, 2, 4, 2), (p, 2, 18, 0, 4, 2), (p, 2, 16, 4, 4, 2), (p, 2, 16, 0, 4, 7),
                 (None, 2, 16, 0, 4, 0)):
        assert lib.wfa_upload_dense_rows(h, *args, 1 << 20, None) == _lib.WFA_E_INVALID, args
    assert lib.wfa_upload_dense_rows(h, p, 2, 16, 8, 4, 0, 1 << 20, None) == 0  # the wave may end with the row
    sess.forget_resident()  # (the call above went past the session's bookkeeping)


def _records_table(case, tag="st"):
    rec = np.zeros(len(case[f"recid_{tag}"]), dtype=[("record_id", "i8"), ("event_length", "i4"), ("wave_offset", "i8")])
    rec["record_id"], rec["event_length"] = case[f"recid_{tag}"], case[f"reclen_{tag}"]
    return rec


CHAIN = ("hit_threshold", "basic_features", "waveform_width_integral", "hit", "waveform_width")


def _chain(case, st):
    """The five dense plugins over one st_waveforms array in one context -> (tables, pool uploads of the chain)."""
    peak = dict(case["options"]["peak"][3], use_filtered=False)
    ctx = SimpleContext({"hit": peak}, {"st_waveforms": st, "records": _records_table(case)},
                        plugins=[HipThresholdHitPlugin(), HipBasicFeaturesPlugin(), HipWaveformWidthIntegralPlugin(),
                                 HipHitFinderPlugin(), HipWaveformWidthPlugin()])
    s = default_pool().session()
    before = s.uploads
    tables = {name: ctx.get_data("run", name) for name in CHAIN}
    return tables, s.uploads - before


def _assert_same_tables(got, want):
    for name in want:
        assert got[name].dtype == want[name].dtype and len(got[name]) == len(want[name]), name
        assert got[name].tobytes() == want[name].tobytes(), name


def test_chain_uploads_the_samples_once(monkeypatch):
    case = G.load_densehit("densehit_v1725")
    st = case["st_waveforms"]
    got, uploads = _chain(case, st)
    assert uploads == 1 and all(len(got[name]) > 0 for name in CHAIN)
    G.assert_struct_equal(got["hit_threshold"], case["hits_st_0"], float_rtol=1e-6)
    G.assert_struct_equal(got["waveform_width_integral"], case["wi_st_0"])
    G.assert_struct_equal(got["hit"], case["peak_st_3"])
    monkeypatch.setattr(DeviceSession, "dense_rows", False)
    want, uploads = _chain(case, st)
    assert uploads == len(CHAIN)
    _assert_same_tables(got, want)


def _filtered_chain(st):
    peak = {"use_filtered": True, "height": 8.0, "distance": 6, "prominence": 0.5, "width": 1}
    ctx = SimpleContext({"hit": peak, "waveform_width": {"use_filtered": True}}, {"st_waveforms": st},
                        plugins=[HipFilteredWaveformsPlugin(), HipHitFinderPlugin(), HipWaveformWidthPlugin()])
    s = default_pool().session()
    tables = {"filtered_waveforms": ctx.get_data("run", "filtered_waveforms")}
    before = s.uploads
    for name in ("hit", "waveform_width"):
        tables[name] = ctx.get_data("run", name)
    return tables, s.uploads - before, s


def test_filtered_rows_stay_on_the_device(monkeypatch):
    st = G.load_dense("dense_v1725")["st_waveforms"]
    got, uploads, s = _filtered_chain(st)
    assert uploads == 0 and len(got["hit"]) > 0 and len(got["waveform_width"]) > 0
    assert s.holds_dense(got["filtered_waveforms"]) and s.holds_dense(st)  # the filters left the uint16 pool as it was
    G.assert_struct_equal(got["filtered_waveforms"], G.load_dense("dense_v1725")["filtered_waveforms"])
    monkeypatch.setattr(DeviceSession, "dense_rows", False)
    want, uploads, _s = _filtered_chain(st)
    assert uploads == 2
    _assert_same_tables(got, want)


def test_layouts_that_fall_back(tmp_path):
    st = G.load_densehit("densehit_v1725")["st_waveforms"]
    plugins = (HipBasicFeaturesPlugin, HipWaveformWidthIntegralPlugin)

    def run(arr):
        ctx = SimpleContext({}, {"st_waveforms": arr}, plugins=[p() for p in plugins])
        s = default_pool().session()
        before = s.uploads
        return {p.provides: ctx.get_data("run", p.provides) for p in plugins}, s.uploads - before

    want, uploads = run(st)
    assert uploads == 1
    view = np.repeat(st, 2)[::2]                        # rows with gaps: the host route, uploaded by every plugin
    assert DeviceSession._dense_layout(view) is None and view.tobytes() == st.tobytes()
    got, uploads = run(view)
    assert uploads == len(plugins)
    _assert_same_tables(got, want)
    path = tmp_path / "st_waveforms.bin"
    path.write_bytes(st.tobytes())
    mapped = np.memmap(path, dtype=st.dtype, mode="r", shape=st.shape)
    assert not mapped.flags.writeable and DeviceSession._dense_layout(mapped) is not None
    got, uploads = run(mapped)
    assert uploads == 1
    _assert_same_tables(got, want)
