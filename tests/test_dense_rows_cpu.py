"""Dense rows on the device, the parts that need no GPU: which arrays DeviceSession._dense_layout lets through as they
are, the residency rule of a dense array (the object, compared with `is`, dropped by every call that replaces a device
pool), and the per-lane body of k_dense_unpack run on the host under AddressSanitizer + UndefinedBehaviorSanitizer
(csrc/host_check.cpp `dense`: every lane of every batch over exactly-sized buffers)."""

import json
import os
import subprocess

import numpy as np
import pytest

from waveformanalysis_amd import _lib
from waveformanalysis_amd import device as D
from waveformanalysis_amd.dtypes import create_filtered_waveform_dtype, create_record_dtype
from waveformanalysis_amd.plugins import _common as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "waveformanalysis_amd", "csrc")

layout = D.DeviceSession._dense_layout


@pytest.mark.parametrize("L", [1, 7, 8, 9, 800])
def test_layout_of_the_st_dtype(L):
    st = np.zeros(5, dtype=create_record_dtype(L))
    assert st.dtype.fields["wave"][1] == 76 and st.dtype.itemsize == 76 + 2 * L
    assert layout(st) == (76, L, 76 + 2 * L, _lib.DENSE_I16)
    filt = np.zeros(5, dtype=create_filtered_waveform_dtype(st.dtype))
    off = filt.dtype.fields["wave"][1]
    want = (off, L, filt.dtype.itemsize, _lib.DENSE_F32) if off % 4 == 0 and filt.dtype.itemsize % 4 == 0 else None
    assert layout(filt) == want
    assert layout(np.zeros(0, dtype=st.dtype)) == (76, L, 76 + 2 * L, _lib.DENSE_I16)


def test_layouts_accepted_and_refused():
    L = 12
    first = np.zeros(4, dtype=[("wave", "<u2", (L,)), ("timestamp", "<i8")])
    assert layout(first) == (0, L, 2 * L + 8, _lib.DENSE_U16)
    after_i2 = np.zeros(4, dtype=[("channel", "<i2"), ("wave", "<i2", (L,))])
    assert layout(after_i2) == (2, L, 2 + 2 * L, _lib.DENSE_I16)
    f32 = np.zeros(4, dtype=[("baseline", "<f8"), ("wave", "<f4", (L,))])
    assert layout(f32) == (8, L, 8 + 4 * L, _lib.DENSE_F32)
    st = np.zeros(6, dtype=create_record_dtype(L))
    assert layout(st[::2]) is None and layout(st[1:]) is not None          # a view with gaps / a contiguous slice
    assert layout(np.zeros(4, dtype=[("wave", "<i2", (3, 4))])) is None    # 2-D subarray
    assert layout(np.zeros(4, dtype=[("wave", "<i4", (L,))])) is None      # another integer width
    assert layout(np.zeros(4, dtype=[("wave", ">i2", (L,))])) is None      # big-endian
    assert layout(np.zeros(4, dtype=[("wave", "<i2")])) is None            # scalar field
    assert layout(np.zeros((4, L), dtype=np.int16)) is None                # a plain matrix
    assert layout(np.zeros(4, dtype=[("samples", "<i2", (L,))])) is None   # no `wave`
    assert layout(np.zeros(4, dtype=[("channel", "<i2"), ("wave", "<f4", (L,))])) is None  # float32 at byte 2
    odd = np.dtype({"names": ["wave"], "formats": [("<i2", (L,))], "offsets": [1], "itemsize": 2 * L + 2})
    assert layout(np.zeros(4, dtype=odd)) is None                          # offset no multiple of the element size
    assert layout(np.zeros((2, 2), dtype=st.dtype)) is None                # 2-D array of rows


class FakeSession(D.DeviceSession):
    """DeviceSession with the C calls replaced: counts uploads, remembers what the 'device' holds."""

    def __init__(self):  # no wfa_ctx
        self._h = None
        self._res_pool = self._res_filtered = self._res_records = None
        self.uploads = 0
        self.n_samples = self.n_records = 0
        self.dev = None

    def upload_pool(self, wave_pool):
        self.forget_resident()
        self.uploads += 1
        self.dev = ("pool", np.array(wave_pool, copy=True))

    def upload_dense(self, data, batch_bytes=None, what="st_waveforms"):
        assert self._dense_layout(data) is not None
        self.forget_resident()
        self.uploads += 1
        self.dev = ("dense", np.array(data["wave"], copy=True))

    def close(self):
        self.forget_resident()


class Ctx:
    class _Pool:
        def __init__(self):
            self.s = FakeSession()

        def session(self):
            return self.s

    def __init__(self):
        self.wfa_device_pool = Ctx._Pool()


def _st(n=6, L=16, fill=3):
    st = np.zeros(n, dtype=create_record_dtype(L))
    st["wave"] = fill
    return st


def test_same_object_uploads_once_a_copy_again():
    ctx = Ctx()
    st = _st()
    s, source, L = K.dense_session(ctx, st, "st_waveforms")
    assert (s.uploads, source, L) == (1, K.SRC_RAW, 16) and s.holds_dense(st)
    K.dense_session(ctx, st, "st_waveforms")
    assert s.uploads == 1                                  # the very same array object: still resident
    twin = st.copy()
    K.dense_session(ctx, twin, "st_waveforms")
    assert s.uploads == 2 and s.holds_dense(twin) and not s.holds_dense(st)
    filt = np.zeros(6, dtype=create_filtered_waveform_dtype(st.dtype))
    assert K.dense_session(ctx, filt, "filtered_waveforms")[1] == K.SRC_F32 and s.uploads == 3
    assert not s.holds_dense(twin)                         # a dense upload replaces whatever was resident


def test_records_route_and_dense_route_evict_each_other():
    ctx = Ctx()
    st, pool = _st(), np.arange(96, dtype=np.uint16)
    s = K.dense_session(ctx, st, "st_waveforms")[0]
    K.resident_session(ctx, pool)                          # ensure_pool of the records route
    assert s.uploads == 2 and not s.holds_dense(st) and s.holds_pool(pool)
    K.dense_session(ctx, st, "st_waveforms")
    assert s.uploads == 3 and s.dev[0] == "dense" and not s.holds_pool(pool)
    s.note_records(st)
    K.dense_session(ctx, st.copy(), "st_waveforms")
    assert not s.holds_records(st)                         # the records of the previous pool went with it
    for drop in (s.forget_resident, s.close):
        K.dense_session(ctx, st, "st_waveforms")
        drop()
        assert not s.holds_dense(st)


def test_float32_rows_follow_the_float32_buffer():
    s = FakeSession()
    st = _st()
    filt = np.zeros(6, dtype=create_filtered_waveform_dtype(st.dtype))
    assert s.ensure_dense(st) and not s.ensure_dense(st)
    s.note_dense(filt)                                     # what filtered_waveforms does after its filters ran
    assert s.holds_dense(st) and s.holds_dense(filt) and s.uploads == 1
    s._drop_f32_tags()                                     # savgol / sosfiltfilt / upload_filtered_pool
    assert s.holds_dense(st) and not s.holds_dense(filt)
    assert not s.holds_dense(None)


def test_switch_off_takes_the_host_route_every_time(monkeypatch):
    monkeypatch.setattr(D.DeviceSession, "dense_rows", False)
    ctx = Ctx()
    st = _st(fill=9)
    for k in range(3):
        s, source, L = K.dense_session(ctx, st, "st_waveforms")
        assert s.uploads == k + 1 and s.dev[0] == "pool" and s.dev[1].shape == (6 * 16,) and s.dev[1][0] == 9
        assert not s.holds_dense(st) and (source, L) == (K.SRC_RAW, 16)


def test_arrays_the_layout_refuses_take_the_host_route_with_its_messages():
    ctx = Ctx()
    st = _st(n=8)
    view = st[::2]
    for k in range(2):
        s = K.dense_session(ctx, view, "st_waveforms")[0]
        assert s.uploads == k + 1 and s.dev[0] == "pool"
    with pytest.raises(ValueError, match="st_waveforms missing required 'wave' field"):
        K.dense_session(ctx, np.zeros(3, dtype=[("x", "i2")]), "st_waveforms")
    with pytest.raises(ValueError, match=r"must be int16 or float32, got int32"):
        K.dense_session(ctx, np.zeros(3, dtype=[("wave", "<i4", (4,))]), "st_waveforms")
    bad = np.repeat(st, 2)[::2]
    bad["wave"][1, 2] = -1
    with pytest.raises(ValueError, match=r"st_waveforms\['wave'\] holds negative samples; the HIP backend reads unsigned ADC codes"):
        K.dense_session(ctx, bad, "st_waveforms")


def test_binding_declares_the_export():
    header = open(os.path.join(REPO, "include", "wfa_hip.h")).read()
    assert "int wfa_upload_dense_rows(" in header and "wfa_upload_dense_rows" in _lib.SIGNATURES
    assert "#define WFA_ABI_VERSION %d" % _lib.ABI_VERSION in header and _lib.ABI_VERSION >= 2
    for name, code in (("I16", _lib.DENSE_I16), ("U16", _lib.DENSE_U16), ("F32", _lib.DENSE_F32)):
        assert f"#define WFA_DENSE_{name} {code}" in header


def test_unpack_lanes_under_sanitizers():
    """The body of k_dense_unpack (wfa_host.hpp dense_unpack_lane) over exactly-sized heap buffers: shapes with L below,
    at and above a 16-byte chunk, batches of one row / three rows / everything, wave at byte 76 / 0 / one element /
    16-byte aligned, int16 (with and without sign bits), uint16 and float32."""
    res = subprocess.run(["make", "-C", CSRC, "SANITIZE=1", "host_check"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([os.path.join(CSRC, "build_tmp", "host_check_asan"), "dense"], capture_output=True, text=True,
                         timeout=600, env=env)
    assert "AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["cases"] > 500 and min(got[f"load{w}"] for w in (2, 4, 8, 16)) > 0  # every load width was exercised
    assert "host::dense_unpack_lane" in open(os.path.join(CSRC, "wfa_capi.hip")).read()  # the kernel runs that body
