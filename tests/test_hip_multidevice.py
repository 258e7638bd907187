"""The `devices` option of hit_threshold, basic_features and waveform_width_integral on the GPU: every sharded output is
byte-identical to the same plugin with devices=None and equal to the reference's stored tables.

Device sets: three sessions on GPU 0 ([0, 0, 0]: contiguous record ranges, each on its own context and worker thread),
and every visible device when there are two or more.  Every input is well below 10^8 samples."""

import contextlib

import numpy as np
import pytest

from tests import golden_util as G
from tests.test_replay_cpu import load_fixture
from waveformanalysis_amd import multidevice as MD
from waveformanalysis_amd.device import device_count
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipBasicFeaturesPlugin, HipThresholdHitPlugin, HipWaveformWidthIntegralPlugin

pytestmark = pytest.mark.gpu

FLOAT_RTOL = 1e-6  # hit rows against the reference, as tests/test_hip_parity.py; sharded vs unsharded is bit-exact
CASES = ["v1725_default", "vx2730_default", "ragged_mixed", "kat_padded_width"]


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
def _ctx(data, **config):
    ctx = SimpleContext({"wave_source": "records", **config}, data)
    try:
        yield ctx
    finally:
        MD.close_sharded_runs(ctx)


def _both(plugin_cls, data, devices, **config):
    """(devices=None output, sharded output) of one plugin on the same inputs; cleanup() after each, as a Context does."""
    out = []
    for dev in (None, devices):
        with _ctx(data, devices=dev, **config) as ctx:
            p = plugin_cls()
            try:
                out.append(p.compute(ctx, "run"))
            finally:
                p.cleanup(ctx)
    return out


def _same_bytes(got, want, what):
    assert got.dtype == want.dtype and len(got) == len(want), what
    assert got.tobytes() == want.tobytes(), f"{what}: sharded output differs from devices=None"


def _data(case):
    d = {"records": case["records"], "wave_pool": case["wave_pool"]}
    if "wave_pool_filtered" in case:
        d["wave_pool_filtered"] = case["wave_pool_filtered"]
    return d


@pytest.mark.parametrize("which", _device_sets())
@pytest.mark.parametrize("name", CASES)
def test_hits_every_records_route(name, which):
    ids = _ids(which)
    case = G.load_case(name)
    data = _data(case)
    routes = [("raw", {}, "hits_raw"), ("use_filtered", {"use_filtered": True}, "hits_filt"),
              ("fuse_filter", {"use_filtered": True, "fuse_filter": True}, "hits_filt")]
    for tag, cfg, key in routes:
        if key not in case:
            continue
        ref, got = _both(HipThresholdHitPlugin, data, ids, **cfg)
        _same_bytes(got, ref, f"{name} {tag}")
        G.assert_struct_equal(got, case[key], float_rtol=FLOAT_RTOL, what=f"{name} {tag} vs reference")
    # the baseline re-estimated in the pass: fused with the filter, and alone on the raw pool
    rec = case["records"].copy()
    rec["baseline"] = -1.0
    bdata = dict(data, records=rec)
    for tag, cfg, key in (("fuse_filter+fuse_baseline", {"use_filtered": True, "fuse_filter": True}, "hits_filt"),
                          ("fuse_baseline", {}, "hits_raw")):
        ref, got = _both(HipThresholdHitPlugin, bdata, ids, fuse_baseline=(0, 40), **cfg)
        _same_bytes(got, ref, f"{name} {tag}")
        if name in ("v1725_default", "vx2730_default"):  # synthetic baselines: the mean of the first 40 samples
            G.assert_struct_equal(got, case[key], float_rtol=FLOAT_RTOL, what=f"{name} {tag} vs reference")


@pytest.mark.parametrize("which", _device_sets())
@pytest.mark.parametrize("name", CASES)
def test_features_records_route(name, which):
    ids = _ids(which)
    case = G.load_case(name)
    data = _data(case)
    for tag, cfg in (("raw", {}), ("filt", {"use_filtered": True})):
        if f"bf_{tag}" in case:
            ref, got = _both(HipBasicFeaturesPlugin, data, ids, **cfg)
            _same_bytes(got, ref, f"{name} basic_features {tag}")
            G.assert_struct_equal(got, case[f"bf_{tag}"], what=f"{name} basic_features {tag} vs reference")
        if f"wi_{tag}" in case:
            ref, got = _both(HipWaveformWidthIntegralPlugin, data, ids, **cfg)
            _same_bytes(got, ref, f"{name} width_integral {tag}")
            G.assert_struct_equal(got, case[f"wi_{tag}"], what=f"{name} width_integral {tag} vs reference")


@pytest.mark.parametrize("which", _device_sets())
def test_per_channel_thresholds_and_fixed_baseline(which):
    ids = _ids(which)
    case = G.load_case("v1725_channel_cfg")
    data = _data(case)
    ref, got = _both(HipThresholdHitPlugin, data, ids, **case["options"]["hit"])
    _same_bytes(got, ref, "per-channel thresholds")
    G.assert_struct_equal(got, case["hits_raw"], float_rtol=FLOAT_RTOL, what="per-channel thresholds vs reference")
    ref, got = _both(HipBasicFeaturesPlugin, data, ids, **case["options"]["bf"])
    _same_bytes(got, ref, "per-channel fixed_baseline")
    G.assert_struct_equal(got, case["bf_raw"], what="per-channel fixed_baseline vs reference")


@pytest.mark.parametrize("which", _device_sets())
def test_c5_replay_256_channels_against_the_reference(which):
    ids = _ids(which)
    d, rec, pool = load_fixture()
    ref, got = _both(HipThresholdHitPlugin, {"records": rec, "wave_pool": pool}, ids)
    _same_bytes(got, ref, "c5_replay hit_threshold")
    G.assert_struct_equal(got, d["hit_threshold"], float_rtol=FLOAT_RTOL, what="c5_replay hit_threshold vs reference")


def test_second_call_on_the_same_pool_uploads_nothing():
    case = G.load_case("v1725_default")
    with _ctx(_data(case), devices=[0, 0, 0]) as ctx:
        HipThresholdHitPlugin().compute(ctx, "run")
        run = MD.sharded_run(ctx, [0, 0, 0])
        before = [s.uploads for s in run.sessions]
        assert before == [1, 1, 1]
        bf = HipBasicFeaturesPlugin().compute(ctx, "run")
        wi = HipWaveformWidthIntegralPlugin().compute(ctx, "run")
        HipThresholdHitPlugin().cleanup(ctx)              # scratch released, residency kept
        hits = HipThresholdHitPlugin().compute(ctx, "run")
        assert [s.uploads for s in run.sessions] == before
        G.assert_struct_equal(bf, case["bf_raw"], what="basic_features after hit_threshold")
        G.assert_struct_equal(wi, case["wi_raw"], what="width_integral after hit_threshold")
        G.assert_struct_equal(hits, case["hits_raw"], float_rtol=FLOAT_RTOL, what="hits, second call")


def test_more_devices_than_records():
    case = G.load_case("kat_padded_width")
    data = _data(case)
    ref, got = _both(HipThresholdHitPlugin, data, [0] * 5)
    _same_bytes(got, ref, "5 shards, 2 records")
    G.assert_struct_equal(got, case["hits_raw"], float_rtol=FLOAT_RTOL, what="5 shards, 2 records vs reference")
    ref, got = _both(HipBasicFeaturesPlugin, data, [0] * 5)
    _same_bytes(got, ref, "5 shards, 2 records (basic_features)")


def test_a_shard_with_no_hits():
    case = G.load_case("v1725_default")
    rec, pool = case["records"].copy(), case["wave_pool"].copy()
    half = len(rec) // 2
    L = int(rec["event_length"][0])
    pool[: half * L] = 8000                                 # the first shard's records are flat at their baseline
    rec["baseline"][:half] = 8000.0
    data = {"records": rec, "wave_pool": pool}
    assert [sh.n_records for sh in MD.split_records(rec, 2)] == [half, len(rec) - half]
    ref, got = _both(HipThresholdHitPlugin, data, [0, 0])
    _same_bytes(got, ref, "a shard with no hits")
    assert len(got) and np.all(got["record_id"] >= half)
