"""The `devices` option of wave_pool_filtered and hit on the GPU: the sharded filtered pool is bit-identical to
devices=None (gaps included), hit rows are byte-identical, and a whole chain on the filtered pool uploads one raw slice
per shard and no float32 pool.

Device sets as tests/test_hip_multidevice.py: three sessions on GPU 0, and every visible device when there are two or
more.  Every input is well below 10^8 samples."""

import contextlib

import numpy as np
import pytest

from oracle import wfa_oracle as O
from tests import golden_util as G
from tests.test_multidevice_filter_cpu import CHANNEL_FILTERS, _hand_made
from waveformanalysis_amd import multidevice as MD
from waveformanalysis_amd.device import DeviceSession, device_count
from waveformanalysis_amd.filter_engine import design_bw
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import (
    HipBasicFeaturesPlugin,
    HipHitFinderPlugin,
    HipThresholdHitPlugin,
    HipWavePoolFilteredPlugin,
)

pytestmark = pytest.mark.gpu

FLOAT_RTOL = 1e-6  # against the reference, as tests/test_hip_parity.py; sharded vs devices=None is bit-exact
FILTER_CASES = ["v1725_default", "v1725_bw", "v1725_channel_cfg", "ragged_mixed", "sgbw_bw1", "sgbw_bw12",
                "sgbw_sg15_13", "sgbw_sg63_12", "interleaved"]


def _device_sets():
    return [pytest.param("three_on_0", id="0,0,0"), pytest.param("all", id="all-visible")]


def _ids(which):
    if which == "three_on_0":
        return [0, 0, 0]
    n = device_count()
    if n < 2:
        pytest.skip(f"{n} device visible: the every-device set needs two or more")
    return list(range(n))


@contextlib.contextmanager
def _ctx(data, plugins, **config):
    ctx = SimpleContext({"wave_source": "records", **config}, data, plugins=[p() for p in plugins])
    try:
        yield ctx
    finally:
        MD.close_sharded_runs(ctx)


def _filter_inputs(name):
    """(records, wave_pool, wave_pool_filtered options, expected pool or None)."""
    if name == "interleaved":
        rec, pool = _hand_made("interleaved")
        return rec, pool, {}, O.filter_wave_pool(rec, pool)
    case = G.load_case(name)
    cfg = G.filter_params(case)
    if name == "v1725_channel_cfg":
        cfg["channel_config"] = CHANNEL_FILTERS
        sos = {c: design_bw(v["lowcut"], v["highcut"], v["fs"], v["filter_order"])[0]
               for c, v in ((3, CHANNEL_FILTERS["0:3"]), (12, CHANNEL_FILTERS["0:12"]))}
        rec = case["records"]

        def per_record(i):
            c = int(rec["channel"][i])
            if c in sos:
                return {"filter_type": "BW", "bw_sos": sos[c]}
            if c == 7:
                return {"sg_window_size": 21, "sg_poly_order": 4}
            return {}

        want = O.filter_wave_pool(rec, case["wave_pool"], per_record_cfg=per_record)
        return rec, case["wave_pool"], cfg, want
    return case["records"], case["wave_pool"], cfg, case["wave_pool_filtered"]


def _filtered(rec, pool, cfg, devices):
    with _ctx({"records": rec, "wave_pool": pool}, [HipWavePoolFilteredPlugin], devices=devices,
              **{f"wave_pool_filtered.{k}": v for k, v in cfg.items()}) as ctx:
        out = ctx.get_data("run", "wave_pool_filtered")
        runs = MD.peek_sharded_runs(ctx)
    return out, runs


@pytest.mark.parametrize("which", _device_sets())
@pytest.mark.parametrize("name", FILTER_CASES)
def test_wave_pool_filtered_bit_identical(name, which):
    ids = _ids(which)
    rec, pool, cfg, want = _filter_inputs(name)
    ref, none_runs = _filtered(rec, pool, cfg, None)
    got, runs = _filtered(rec, pool, cfg, ids)
    assert none_runs == [] and len(runs) == 1 and runs[0].n_shards == len(ids)
    assert got.dtype == np.float32 and got.shape == ref.shape == (len(pool),)
    diff = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
    assert diff.size == 0, f"{name}: {diff.size} samples differ from devices=None, first at {diff[:5]}"
    np.testing.assert_allclose(got, want, rtol=FLOAT_RTOL, atol=0, err_msg=f"{name} vs reference")


@pytest.mark.parametrize("which", _device_sets())
@pytest.mark.parametrize("name", G.peaks_case_names())
def test_hit_rows_byte_identical(name, which):
    ids = _ids(which)
    case = G.load_peaks(name)
    data = {k: case[k] for k in ("records", "wave_pool", "wave_pool_filtered")}
    for k, cfg in enumerate(case["configs"]):
        out = []
        for dev in (None, ids):
            with _ctx(data, [HipHitFinderPlugin], devices=dev, **{f"hit.{a}": b for a, b in cfg.items()}) as ctx:
                out.append(ctx.get_data("run", "hit"))
                assert (MD.peek_sharded_runs(ctx) != []) == (dev is not None)
        ref, got = out
        assert got.dtype == ref.dtype and len(got) == len(ref) and got.tobytes() == ref.tobytes(), f"{name} cfg {k}"
        G.assert_struct_equal(got, case[f"hit_{k}"], what=f"{name} cfg {k} vs reference")


CHAIN = ("wave_pool_filtered", "hit_threshold", "basic_features", "hit")


def _chain(data, devices):
    with _ctx(data, [HipWavePoolFilteredPlugin, HipThresholdHitPlugin, HipBasicFeaturesPlugin, HipHitFinderPlugin],
              devices=devices, use_filtered=True) as ctx:
        out = {name: ctx.get_data("run", name) for name in CHAIN}
        runs = MD.peek_sharded_runs(ctx)
        sessions = [id(s) for s in runs[0].sessions] if runs else []
    return out, runs, sessions


@pytest.mark.parametrize("which", _device_sets())
@pytest.mark.parametrize("name", ["v1725_default", "ragged_mixed"])
def test_filtered_chain_uploads_one_raw_slice_per_shard(name, which, monkeypatch):
    ids = _ids(which)
    case = G.load_case(name)
    data = {"records": case["records"], "wave_pool": case["wave_pool"]}
    want, _runs, _s = _chain(data, None)

    uploads = []
    raw, filt = DeviceSession.upload_pool, DeviceSession.upload_filtered_pool

    def upload_pool(self, wave_pool):
        uploads.append((id(self), np.dtype(wave_pool.dtype).name))
        return raw(self, wave_pool)

    def upload_filtered_pool(self, pool_f32):
        uploads.append((id(self), "filtered"))
        return filt(self, pool_f32)

    monkeypatch.setattr(DeviceSession, "upload_pool", upload_pool)
    monkeypatch.setattr(DeviceSession, "upload_filtered_pool", upload_filtered_pool)
    got, runs, sessions = _chain(data, ids)
    monkeypatch.undo()

    assert len(runs) == 1 and runs[0].n_shards == len(ids)
    shards = MD.split_records(case["records"], len(ids))
    busy = [s for s, sh in zip(sessions, shards) if sh.n_records > 0]
    assert sorted(uploads) == sorted((s, "uint16") for s in busy), uploads
    for name_ in CHAIN:
        assert got[name_].tobytes() == want[name_].tobytes(), f"{name} {name_}: differs from devices=None"
    np.testing.assert_array_equal(got["wave_pool_filtered"], case["wave_pool_filtered"])
    G.assert_struct_equal(got["hit_threshold"], case["hits_filt"], float_rtol=FLOAT_RTOL, what=f"{name} hits_filt")
    G.assert_struct_equal(got["basic_features"], case["bf_filt"], what=f"{name} bf_filt")


def test_ranged_download_of_the_filtered_pool():
    case = G.load_case("ragged_mixed")
    with DeviceSession(0) as sess:
        sess.upload_pool(case["wave_pool"])
        sess.upload_records(case["records"])
        with pytest.raises(Exception, match="no float32 pool"):
            sess.download_filtered(np.empty(4, dtype=np.float32), start=1)
        sess.set_sg_plan(11, 2)
        sess.savgol(download=False)
        whole = sess.download_filtered()
        np.testing.assert_array_equal(whole, case["wave_pool_filtered"])
        n = len(whole)
        for start, count in ((0, n), (1, 7), (805, 1000), (n - 3, 3), (n, 0), (1234, 1)):
            part = np.full(count, np.nan, dtype=np.float32)
            assert sess.download_filtered(part, start=start) is part
            assert part.tobytes() == whole[start:start + count].tobytes(), (start, count)
        tail = sess.download_filtered(start=n - 10)
        assert tail.tobytes() == whole[n - 10:].tobytes()
        big = np.zeros(n + 1, dtype=np.float32)
        for start, count in ((-1, 2), (n - 2, 3), (n + 1, 0)):
            with pytest.raises(ValueError):
                sess.download_filtered(big[:count], start=start)
        with pytest.raises(ValueError):
            sess.download_filtered(np.zeros(4, dtype=np.float64))
