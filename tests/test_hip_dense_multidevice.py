"""The `devices` option on the dense routes (wave_source auto / st_waveforms / filtered_waveforms) of hit_threshold, hit,
basic_features, waveform_width_integral, filtered_waveforms and waveform_width on the GPU: every sharded output is
byte-identical to the same plugin with devices=None and equal to the reference's stored tables.

Device sets as tests/test_hip_multidevice.py: three sessions on GPU 0 ([0, 0, 0]: contiguous row ranges, each on its own
context and worker thread), and every visible device when there are two or more.  Inputs are the 40 x 800 dense
fixtures and synthetic arrays of a few hundred samples."""

import numpy as np
import pytest

from tests import golden_util as G
from tests.test_dense_multidevice_cpu import NEGATIVE, _st
from tests.test_hip_densehit import _data as densehit_data
from waveformanalysis_amd import multidevice as MD
from waveformanalysis_amd.device import DeviceSession, default_pool, device_count
from waveformanalysis_amd.dtypes import HIT_DTYPE, RECORDS_DTYPE, create_record_dtype
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

FLOAT_RTOL = 1e-6  # threshold-hit height / integral against the reference, as tests/test_hip_densehit.py
THREE = [0, 0, 0]


def _device_sets():
    return [pytest.param("three_on_0", id="0,0,0"), pytest.param("all", id="all-visible")]


def _ids(which):
    if which == "three_on_0":
        return THREE
    n = device_count()
    if n < 2:
        pytest.skip(f"{n} device visible: the every-device set needs two or more")
    return list(range(n))


class Pair:
    """One context with devices=None and one with a device list over the same data; both() runs one plugin on each
    (cleanup() after it, as a Context does) and returns (devices=None output, sharded output)."""

    def __init__(self, data, ids):
        self.one = SimpleContext({}, dict(data))
        self.many = SimpleContext({"devices": list(ids)}, dict(data))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        MD.close_sharded_runs(self.many)

    def set(self, name, one, many=None):
        self.one._data[name] = one
        self.many._data[name] = one if many is None else many

    def both(self, plugin_cls, **config):
        out = []
        for ctx in (self.one, self.many):
            p = plugin_cls()
            ctx.config[p.provides] = dict(config)
            try:
                out.append(p.compute(ctx, "run"))
            finally:
                p.cleanup(ctx)
        return out

    def same(self, plugin_cls, what, **config):
        want, got = self.both(plugin_cls, **config)
        assert got.dtype == want.dtype and got.shape == want.shape, what
        assert got.tobytes() == want.tobytes(), f"{what}: sharded output differs from devices=None"
        return got

    @property
    def run(self):
        (run,) = MD.peek_sharded_runs(self.many)
        return run


def _records_for(st):
    L = st.dtype["wave"].shape[0]
    rec = np.zeros(len(st), dtype=[("record_id", "i8"), ("event_length", "i4"), ("wave_offset", "i8")])
    rec["record_id"] = st["record_id"]
    rec["event_length"] = st["event_length"] if "event_length" in st.dtype.names else L
    return rec


# ---- 1. byte identity and golden equality ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", _device_sets())
@pytest.mark.parametrize("name", G.dense_case_names())
def test_filtered_waveforms_basic_features_and_waveform_width(name, which):
    ids = _ids(which)
    case = G.load_dense(name)
    data = {"st_waveforms": case["st_waveforms"], "filtered_waveforms": case["filtered_waveforms"], "hit": case["hit"]}
    with Pair(data, ids) as pair:
        got = pair.same(HipFilteredWaveformsPlugin, f"{name} filtered_waveforms")
        G.assert_struct_equal(got, case["filtered_waveforms"], what=f"{name} filtered_waveforms vs reference")
        with pytest.warns(UserWarning, match="已调整为奇数"):
            got = pair.same(HipFilteredWaveformsPlugin, f"{name} filtered_cc", channel_config=case["options"]["filter_cc"])
        G.assert_struct_equal(got, case["filtered_cc"], what=f"{name} filtered_cc vs reference")
        got = pair.same(HipBasicFeaturesPlugin, f"{name} bf st")
        G.assert_struct_equal(got, case["bf_st"], what=f"{name} bf st vs reference")
        got = pair.same(HipBasicFeaturesPlugin, f"{name} bf filt", use_filtered=True, height_range=(30, 400),
                        area_range=(10, 700))
        G.assert_struct_equal(got, case["bf_filt"], what=f"{name} bf filt vs reference")
        for k, cfg in enumerate(case["options"]["width"]):
            got = pair.same(HipWaveformWidthPlugin, f"{name} width cfg {k}", **cfg)
            G.assert_struct_equal(got, case[f"width_{k}"], what=f"{name} width cfg {k} vs reference")


@pytest.mark.parametrize("which", _device_sets())
@pytest.mark.parametrize("tag", list(G.DENSEHIT_SOURCES))
@pytest.mark.parametrize("name", G.densehit_case_names())
def test_hit_threshold_width_integral_and_hit(name, tag, which):
    ids = _ids(which)
    case = G.load_densehit(name)
    base = G.DENSEHIT_SOURCES[tag][1]
    with Pair(densehit_data(case, tag), ids) as pair:
        for k, cfg in enumerate(case["options"]["hit"]):  # cfg 1: per-channel thresholds
            got = pair.same(HipThresholdHitPlugin, f"{name} hits {tag} {k}", **base, **cfg)
            G.assert_struct_equal(got, case[f"hits_{tag}_{k}"], float_rtol=FLOAT_RTOL, what=f"{name} hits {tag} {k}")
        for k, cfg in enumerate(case["options"]["wi"]):
            if f"wi_{tag}_{k}" in case:
                got = pair.same(HipWaveformWidthIntegralPlugin, f"{name} wi {tag} {k}", **base, **cfg)
                G.assert_struct_equal(got, case[f"wi_{tag}_{k}"], what=f"{name} wi {tag} {k}")
        for k, cfg in enumerate(case["options"]["peak"]):
            if f"peak_{tag}_{k}" in case:
                got = pair.same(HipHitFinderPlugin, f"{name} peak {tag} {k}", **{"use_filtered": False, **base, **cfg})
                G.assert_struct_equal(got, case[f"peak_{tag}_{k}"], what=f"{name} peak {tag} {k}")


@pytest.mark.parametrize("which", _device_sets())
def test_per_channel_fixed_baseline(which):
    ids = _ids(which)
    st = _st(21, 13)
    cc = {"0:1": {"fixed_baseline": 990.0}, "0:2": {"fixed_baseline": 1004.5}}
    with Pair({"st_waveforms": st}, ids) as pair:
        plain = pair.same(HipBasicFeaturesPlugin, "no fixed baseline")
        fixed = pair.same(HipBasicFeaturesPlugin, "per-channel fixed_baseline", channel_config=cc)
    assert plain.tobytes() != fixed.tobytes()  # the option reached the shards' rows


# ---- 2. the run really is sharded ------------------------------------------------------------------------------------
def test_the_default_route_runs_on_the_shards():
    case = G.load_densehit(G.densehit_case_names()[0])
    data = densehit_data(case, "st")
    st = data["st_waveforms"]
    L = st.dtype["wave"].shape[0]
    own = default_pool().session()
    before = own.uploads
    with Pair(data, THREE) as pair:
        hits = HipThresholdHitPlugin().compute(pair.many, "run")  # wave_source="auto": nothing else was changed
        assert len(hits) == len(case["hits_st_0"])
        run = pair.run
        assert run.device_ids == THREE
        assert sum(s.n_samples for s in run.sessions) == len(st) * L
        for (r0, r1), sess in zip(MD.split_rows(len(st), L, 3), run.sessions):
            assert sess.uploads == (1 if r1 > r0 else 0) and sess.n_samples == (r1 - r0) * L
    assert default_pool().peek_session() is own and own.uploads == before  # the calling thread's session stayed out


# ---- 3. chain residency ----------------------------------------------------------------------------------------------
def test_a_chain_uploads_every_row_once_and_no_filtered_sample():
    case = G.load_dense(G.dense_case_names()[0])
    st = case["st_waveforms"]
    plugins = lambda: [HipFilteredWaveformsPlugin(), HipHitFinderPlugin(), HipWaveformWidthPlugin(),  # noqa: E731
                       HipBasicFeaturesPlugin()]
    config = {"devices": THREE, "waveform_width": {"use_filtered": True}, "basic_features": {"use_filtered": True}}
    data = {"st_waveforms": st, "records": _records_for(st)}
    want = SimpleContext({k: v for k, v in config.items() if k != "devices"}, data, plugins=plugins())
    ctx = SimpleContext(config, data, plugins=plugins())
    try:
        for name in ("filtered_waveforms", "hit", "waveform_width", "basic_features"):
            got = ctx.get_data("run", name)
            assert got.tobytes() == want.get_data("run", name).tobytes(), name
        assert len(ctx.get_data("run", "hit")) and len(ctx.get_data("run", "basic_features")) == len(st)
        (run,) = MD.peek_sharded_runs(ctx)
        assert [s.uploads for s in run.sessions] == [1, 1, 1]  # the uint16 rows, once; no float32 sample went up
        fw = ctx.get_data("run", "filtered_waveforms")
        for k, (r0, r1) in enumerate(MD.split_rows(len(st), st.dtype["wave"].shape[0], 3)):
            assert run._dense[k][0] is st and run._dense_f32[k][0] is fw and run._dense_f32[k][1:3] == (r0, r1)
        HipThresholdHitPlugin().compute(ctx, "run")  # st_waveforms kept its own tag beside the filtered rows
        assert [s.uploads for s in run.sessions] == [1, 1, 1]
    finally:
        MD.close_sharded_runs(ctx)
    again = SimpleContext(config, {"st_waveforms": st.copy()}, plugins=plugins())  # equal contents, another object
    try:
        again.get_data("run", "hit")
        (run,) = MD.peek_sharded_runs(again)
        assert [s.uploads for s in run.sessions] == [1, 1, 1]
    finally:
        MD.close_sharded_runs(again)


# ---- 4. alignment and edges ------------------------------------------------------------------------------------------
SHAPES = [pytest.param(21, 13, [(0, 8), (8, 16), (16, 21)], id="L13-unit8"),
          pytest.param(10, 12, [(0, 2), (2, 6), (6, 10)], id="L12-unit2"),
          pytest.param(2, 800, [(0, 0), (0, 1), (1, 2)], id="L800-empty-shard"),
          pytest.param(0, 13, [(0, 0)] * 3, id="no-rows")]


@pytest.mark.parametrize("n,L,parts", SHAPES)
def test_alignment_and_edge_shapes(n, L, parts):
    assert MD.split_rows(n, L, 3) == parts
    st = _st(n, L)
    with Pair({"st_waveforms": st, "records": _records_for(st)}, THREE) as pair:
        hits = pair.same(HipThresholdHitPlugin, "hit_threshold raw")
        assert len(hits) >= n  # every row carries a pulse
        pair.same(HipBasicFeaturesPlugin, "basic_features", height_range=(0, L), area_range=(0, None))
        fw_one, fw_many = pair.both(HipFilteredWaveformsPlugin)
        assert fw_many.dtype == fw_one.dtype and fw_many.tobytes() == fw_one.tobytes(), "filtered_waveforms"
        pair.set("filtered_waveforms", fw_one, fw_many)
        pair.same(HipThresholdHitPlugin, "hit_threshold on the filtered rows", use_filtered=True)
        if n:
            run = pair.run
            assert [s.n_samples for s in run.sessions if s.n_samples] == [(r1 - r0) * L for r0, r1 in parts if r1 > r0]
            assert [s.uploads for s in run.sessions] == [1 if r1 > r0 else 0 for r0, r1 in parts]
    bare = _st(n, L, baseline=False)  # no `baseline` field: the pass takes the row mean on the device
    with Pair({"st_waveforms": bare, "records": _records_for(bare)}, THREE) as pair:
        pair.same(HipThresholdHitPlugin, "hit_threshold, baseline_mean leg")
        pair.same(HipBasicFeaturesPlugin, "basic_features without baseline", height_range=(0, L))


# ---- 5. waveform_width hit placement ---------------------------------------------------------------------------------
def _width_inputs():
    n, L = 24, 64
    st = np.zeros(n, dtype=create_record_dtype(L))
    t = np.arange(L)
    for r in range(n):
        st["wave"][r] = 1000 + np.maximum(0, (200 + 10 * r) - (12 + r % 5) * np.abs(t - (20 + r)))
    st["baseline"], st["dt"], st["event_length"] = 1000.0, 2, L
    st["record_id"] = np.arange(n)
    st["timestamp"] = 10**6 * np.arange(n)
    st["channel"] = np.arange(n) % 4
    # last row of shard 0, first of shard 1, one more in shard 1, none in shard 2 (rows 16..23); unsorted; two no-row ids
    rows = np.array([8, 3, 7, 999, 12, 0, -2, 7, 15], dtype=np.int64)
    hits = np.zeros(len(rows), dtype=HIT_DTYPE)
    hits["record_id"] = rows
    hits["position"] = np.where((rows >= 0) & (rows < n), 20 + rows, 5)
    hits["timestamp"] = 17 * np.arange(len(rows))
    hits["channel"] = np.arange(len(rows)) % 4
    rec = np.zeros(n, dtype=RECORDS_DTYPE)
    rec["record_id"], rec["event_length"], rec["wave_offset"] = np.arange(n), L, np.arange(n) * L
    rec["baseline"], rec["dt"], rec["timestamp"], rec["channel"] = 1000.0, 2, st["timestamp"], st["channel"]
    pool = np.ascontiguousarray(st["wave"]).reshape(-1).view(np.uint16).copy()
    return st, hits, rec, pool


@pytest.mark.parametrize("route", ["auto", "records", "no_record_id_field"])
def test_waveform_width_hit_placement(route):
    st, hits, rec, pool = _width_inputs()
    assert MD.split_rows(len(st), 64, 3) == [(0, 8), (8, 16), (16, 24)]
    assert [(sh.r0, sh.r1) for sh in MD.split_records(rec, 3)] == [(0, 8), (8, 16), (16, 24)]
    if route == "no_record_id_field":  # the row is then the hit's record_id itself, range-checked
        st = np.ascontiguousarray(st[[f for f in st.dtype.names if f != "record_id"]])
        st = st.astype(np.dtype([(f, st.dtype.fields[f][0]) for f in st.dtype.names]))  # packed again
    data = {"st_waveforms": st, "hit": hits, "records": rec, "wave_pool": pool}
    config = {"wave_source": "records"} if route == "records" else {}
    with Pair(data, THREE) as pair:
        got = pair.same(HipWaveformWidthPlugin, f"waveform_width {route}", **config)
        assert list(got["record_id"]) == [8, 3, 7, 12, 0, 7, 15]  # hit order, the two no-row hits dropped
        assert [s.uploads for s in pair.run.sessions] == [1, 1, 0]  # the shard with no hits uploaded nothing


# ---- 6. a negative int16 sample --------------------------------------------------------------------------------------
def test_negative_sample_in_the_second_shard():
    st = _st(21, 13)
    bad = st.copy()
    bad["wave"][11, 4] = -5  # rows 8..15 are the second shard's
    with Pair({"st_waveforms": bad, "records": _records_for(bad)}, THREE) as pair:
        with pytest.raises(MD.ShardError, match="shard 1 on device 0") as err:
            HipThresholdHitPlugin().compute(pair.many, "run")
        assert isinstance(err.value.__cause__, ValueError) and NEGATIVE in str(err.value.__cause__)
        assert err.value.shard == 1
        assert [s.first_negative_row for s in pair.run.sessions] == [-1, 11, -1]  # the row of the whole array
        pair.set("st_waveforms", st)
        pair.same(HipThresholdHitPlugin, "a good call after the refused one")
        assert [s.first_negative_row for s in pair.run.sessions] == [-1, -1, -1]


# ---- 7. layouts the device cannot take as they are -------------------------------------------------------------------
@pytest.mark.parametrize("how", ["view_with_gaps", "dense_rows_off"])
def test_fallback_layout_is_sharded_and_leaves_nothing_resident(how, monkeypatch):
    st = _st(42, 13)
    if how == "view_with_gaps":
        st = st[::2]
        assert DeviceSession._dense_layout(st) is None
    else:
        st = st[:21].copy()
        monkeypatch.setattr(DeviceSession, "dense_rows", False)
    with Pair({"st_waveforms": st, "records": _records_for(st)}, THREE) as pair:
        pair.same(HipThresholdHitPlugin, f"hit_threshold {how}")
        pair.same(HipBasicFeaturesPlugin, f"basic_features {how}", height_range=(0, 13))
        pair.same(HipFilteredWaveformsPlugin, f"filtered_waveforms {how}")
        pair.same(HipHitFinderPlugin, f"hit {how}", use_filtered=False, height=10.0, width=1, distance=1)
        run = pair.run
        assert sum(s.uploads for s in run.sessions) >= 4 * 2  # sharded, and uploaded by every call
        assert run._dense == run._dense_f32 == run._resident == run._filtered == [None] * 3
        assert not any(s._res_dense is not None or s._res_dense_f32 is not None or s._res_pool is not None
                       for s in run.sessions)
