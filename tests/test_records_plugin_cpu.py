"""HipRecordsPlugin / HipWavePoolPlugin without a GPU: the contract they share with the reference's RecordsPlugin /
WavePoolPlugin (options, dependencies, lineage, dt rule), the packaging, the host part splitting of the multi-part
CSV build, and the channel_metadata polarity against records the reference's plugins made
(tests/golden/vx2730csv_records_plugin.npz)."""

import json
import os

import numpy as np
import pytest

from tests import golden_util as G
from waveformanalysis_amd import records_builder as RB
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import hip_default, hip_with_records
from waveformanalysis_amd.plugins import records as R

OPTIONS = {  # name: (default, track)
    "daq_adapter": ("vx2730", True),
    "channel_workers": (None, False),
    "channel_executor": ("thread", False),
    "n_jobs": (None, False),
    "use_process_pool": (False, False),
    "chunksize": (None, False),
    "parse_engine": ("auto", False),
    "records_part_size": (250_000, True),
    "dt": (None, True),
    "baseline_samples": (None, True),
}


def load_fixture():
    z = np.load(os.path.join(G.GOLDEN, "vx2730csv_records_plugin.npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["options"] = json.loads(bytes(d.pop("options_json")).decode())
    return d


class RunCtx(SimpleContext):
    def __init__(self, *a, run_config=None, **kw):
        super().__init__(*a, **kw)
        self.run_config = run_config or {}

    def get_run_config(self, run_id):
        return self.run_config


@pytest.mark.parametrize("cls,provides,dtype", [(R.HipRecordsPlugin, "records", RB.RECORDS_DTYPE),
                                                (R.HipWavePoolPlugin, "wave_pool", np.dtype(np.uint16))])
def test_contract(cls, provides, dtype):
    p = cls()
    assert p.provides == provides
    assert np.dtype(p.output_dtype) == dtype
    assert p.version == "0.10.0+hip1"
    assert p.depends_on == ["raw_files"]
    assert p.save_when == "always" and p.uses_run_config is True
    assert {k: (o.default, o.track) for k, o in p.options.items()} == OPTIONS
    v = p.options["baseline_samples"].validate
    assert v(None) and v(40) and v((1, 5)) and v([0, 800])
    assert not v((1, 2, 3)) and not v(1.5) and not v(("a", 2))
    ctx = SimpleContext({"daq_adapter": "V1725", "n_jobs": 8}, {"raw_files": []}, [p])
    assert p.resolve_depends_on(ctx) == ["raw_files"]
    lin = p.get_lineage(ctx)
    assert set(lin) == {"plugin_class", "plugin_version", "description", "config", "depends_on", "dtype"}
    assert lin["plugin_class"] == cls.__name__ and lin["plugin_version"] == "0.10.0+hip1"
    assert lin["config"] == {"daq_adapter": "v1725", "records_part_size": 250_000, "dt": None, "baseline_samples": None}
    assert lin["depends_on"] == {"raw_files": {}}
    assert lin["dtype"] == dtype.descr


def test_dt_resolution():
    p = R.HipRecordsPlugin()

    def dt(config, adapter="vx2730"):
        return R.resolve_dt_ns(SimpleContext(config, plugins=[p]), p, adapter)

    assert dt({}) == 2
    assert dt({}, "v1725") == 4
    assert dt({}, "other") == 1
    assert dt({}, None) == 1
    assert dt({"daq_adapter": "V1725"}, None) == 4
    assert dt({"dt": 7}) == 7
    assert dt({"records": {"dt": 3}, "dt": 9}) == 3
    assert dt({"dt": 0}) == 0
    for key in ("records_dt_ns", "dt_ns", "sampling_interval_ns"):
        with pytest.warns(DeprecationWarning, match=f"Config '{key}' is deprecated"):
            assert dt({key: 5}) == 5
    with pytest.warns(DeprecationWarning):
        assert dt({"records_dt_ns": 6, "dt_ns": 8}) == 6
    for bad in (2**31, -1):
        with pytest.raises(ValueError, match=f"records_dt_ns out of int32 range: {bad}"):
            dt({"dt": bad})


def test_adapter_name():
    p = R.HipRecordsPlugin()
    assert R.resolve_adapter_name(SimpleContext({}, plugins=[p]), p) == "vx2730"
    assert R.resolve_adapter_name(SimpleContext({"daq_adapter": "V1725"}, plugins=[p]), p) == "v1725"
    assert R.resolve_adapter_name(SimpleContext({"records": {"daq_adapter": None}}, plugins=[p]), p) is None


def test_hip_with_records():
    base, full = hip_default(), hip_with_records()
    assert [type(p) for p in full] == [type(p) for p in base] + [R.HipRecordsPlugin, R.HipWavePoolPlugin]
    assert "records" not in {p.provides for p in base}


def _check_parts(bodies, budget):
    parts = R.RB.vx2730_parts(bodies, budget)
    joined = b"".join(b"".join(bodies[f][a:b] for f, a, b in part) for part in parts)
    assert joined == b"".join(bodies)
    last = {}
    for part in parts:
        size = sum(b - a for _f, a, b in part)
        assert size > 0
        for f, a, b in part:
            assert 0 <= a < b <= len(bodies[f]) and a == last.get(f, 0)  # in order, no gap, no overlap
            last[f] = b
            # a cut inside a file follows a line end
            assert b == len(bodies[f]) or bodies[f][b - 1:b] == b"\n"
        if size > budget:  # only one row longer than the budget overshoots it
            assert len(part) == 1
            f, a, b = part[0]
            assert bodies[f].count(b"\n", a, b - 1) == 0
    assert [f for part in parts for f, _a, _b in part] == sorted(f for part in parts for f, _a, _b in part)
    return parts


def test_part_splitting_fixture_texts():
    groups, _variants, _fx = G.load_vx2730csv()
    bodies = [RB.vx2730_body(text, k == 0) for g in groups for k, (_f, text) in enumerate(g)]
    bodies = [b for b in bodies if b]
    total = sum(len(b) for b in bodies)
    for budget in (1, 2, 7, 100, 400, 1000, 1024, 3000, 4096, 5000, 16384, total - 1, total, 65536):
        parts = _check_parts(bodies, budget)
        if budget >= total:
            assert len(parts) == 1
        if budget == 1:
            assert len(parts) == sum(b.count(b"\n") for b in bodies)   # one row per part
    # at 4 KiB some file is cut in the middle and the part then continues with the next file
    parts = _check_parts(bodies, 4096)
    assert any(b < len(bodies[f]) for part in parts for f, _a, b in part)


def test_part_splitting_edge_cases():
    hdr = b"BOARD;CHANNEL;TIMETAG;ENERGY;ENERGYSHORT;FLAGS;PROBE_CODE;SAMPLES\n"
    assert RB.vx2730_body(hdr, True) == b""                       # header-only files give nothing
    assert RB.vx2730_body(b"h1\r\nh2\r\n", True) == b""
    assert RB.vx2730_body(hdr + b"0;0;1;0;0;0;1;5", True) == b"0;0;1;0;0;0;1;5\n"   # missing final newline
    crlf = RB.vx2730_body(b"h1\r\nh2\r\n" + b"0;0;1;0;0;0;1;5;6\r\n0;0;2;0;0;0;1;7;8\r\n\r\n", True)
    assert crlf == b"0;0;1;0;0;0;1;5;6\r\n0;0;2;0;0;0;1;7;8\r\n\r\n"
    assert RB.vx2730_body(b"0;0;1;0;0;0;1;5\n", False) == b"0;0;1;0;0;0;1;5\n"   # later files keep their first row
    long_row = b"0;0;1;0;0;0;1;" + b";".join(b"123" for _ in range(300)) + b"\n"
    bodies = [crlf, b"", long_row + b"0;0;3;0;0;0;1;9\n", b"\n\n"]
    for budget in range(1, 80):
        _check_parts(bodies, budget)
    for budget in (100, 1000, 2000):
        _check_parts(bodies, budget)
    assert RB.vx2730_parts([b""], 10) == []
    with pytest.raises(ValueError, match="part_bytes must be >= 1"):
        RB.vx2730_parts([b"1\n"], 0)


def test_polarity_lookup_matches_reference():
    fx = load_fixture()
    opt = fx["options"]
    for name in ("vx2730_records", "v1725_records"):
        want = fx[name]
        ctx = RunCtx({"channel_metadata": opt["metadata_context"]}, run_config={"channel_metadata": opt["metadata_run"]})
        rec = want.copy()
        rec["polarity"] = "negative"
        R.apply_records_polarity(ctx, opt["run_id"], rec)
        np.testing.assert_array_equal(rec["polarity"], want["polarity"], err_msg=name)
    assert set(fx["vx2730_records"]["polarity"]) | set(fx["v1725_records"]["polarity"]) == {"positive", "negative",
                                                                                            "unknown"}
    # without metadata every record is "unknown"
    rec = fx["v1725_records"].copy()
    R.apply_records_polarity(SimpleContext({}), "r", rec)
    assert set(rec["polarity"]) == {"unknown"}
    # the run layer alone
    ctx = RunCtx({}, run_config={"channel_metadata": {"channels": {"0:3": {"polarity": "positive"}}}})
    rec = fx["v1725_records"].copy()
    R.apply_records_polarity(ctx, "r", rec)
    sel = (rec["board"] == 0) & (rec["channel"] == 3)
    assert sel.any() and set(rec["polarity"][sel]) == {"positive"} and set(rec["polarity"][~sel]) == {"unknown"}


def test_records_errors_before_the_device():
    p = R.HipRecordsPlugin()
    ctx = SimpleContext({}, {"raw_files": ("a.CSV",)}, [p])
    with pytest.raises(RuntimeError, match="records expects raw_files as a list of per-channel file groups"):
        ctx.get_data("r", "records")


def test_fixture_v1725_equals_builder_fixture():
    """The plugin fixture's v1725 bundle is the builder fixture's (dt 4 from the adapter, duplicate path dropped)
    with the metadata polarity."""
    fx = load_fixture()
    z = np.load(os.path.join(G.GOLDEN, "v1725bin_files.npz"), allow_pickle=False)
    want = z["records"].copy()
    want["polarity"] = fx["v1725_records"]["polarity"]
    G.assert_struct_equal(fx["v1725_records"], want)
    np.testing.assert_array_equal(fx["v1725_wave_pool"], z["wave_pool"])


def test_fuse_baseline_is_validated_like_baseline_samples():
    """HipThresholdHitPlugin's fuse_baseline: None, or two non-negative ints with start < end, with the messages of the
    records builder's (start, end) rule.  An empty window is refused because the plugin's two routes would read it
    differently (the fused pass skips the estimate, baseline_mean writes NaN)."""
    from waveformanalysis_amd.plugins import threshold_hit as T

    v = T.HipThresholdHitPlugin.options["fuse_baseline"].validate
    assert T.fuse_baseline_window(None) is None and v(None)
    for good in ((0, 40), [5, 29], (79, 2**31 - 1), (0, 2**31)):
        assert T.fuse_baseline_window(good) == tuple(good) and v(good)
    for bad, exc, msg in (((7, 7), ValueError, r"start must be less than end, got \(7, 7\)"),
                          ((9, 3), ValueError, r"start must be less than end, got \(9, 3\)"),
                          ((-1, 5), ValueError, r"indices must be non-negative, got \(-1, 5\)"),
                          ((0, -5), ValueError, r"indices must be non-negative, got \(0, -5\)"),
                          ((1, 2, 3), ValueError, "tuple must have 2 elements"),
                          ((0.0, 40), TypeError, r"tuple elements must be int, got \(float, int\)"),
                          (40, TypeError, "fuse_baseline must be None or a tuple"),
                          (True, TypeError, "fuse_baseline must be None or a tuple"),
                          ("0,40", TypeError, "fuse_baseline must be None or a tuple")):
        assert not v(bad), bad
        with pytest.raises(exc, match=msg):
            T.fuse_baseline_window(bad)
        # the same messages as the records builder, where it takes the value at all
        if isinstance(bad, tuple):
            with pytest.raises(exc, match=msg):
                RB._baseline_window(bad, 0, 0, 1)
    # compute() refuses the option before it reads any input
    rec = np.zeros(1, dtype=RB.RECORDS_DTYPE)
    ctx = SimpleContext({"wave_source": "records", "hit_threshold": {"fuse_baseline": (7, 7)}},
                        {"records": rec, "wave_pool": np.zeros(0, np.uint16)}, [T.HipThresholdHitPlugin()])
    with pytest.raises(RuntimeError, match=r"start must be less than end, got \(7, 7\)") as err:
        ctx.get_data("run", "hit_threshold")
    assert isinstance(err.value.__cause__, ValueError)


class _WindowLib:
    """Stand-in for libwfa_hip.so that records the window arguments as Python ints, before ctypes would narrow them."""

    def __init__(self):
        self.calls = []

    def wfa_ctx_create(self, device_id, handle):
        return 0

    def wfa_baseline_mean(self, h, start, end, update, out):
        self.calls.append((start, end))
        return 0

    def wfa_fused_baseline_filter_hits(self, h, start, end, le, re, max_len, n):
        self.calls.append((start, end))
        return 0

    def wfa_hits_enqueue(self, h, source, start, end, le, re, max_len):
        self.calls.append((start, end))
        return 0

    def wfa_threshold_hits_fill(self, h, out, n):
        return 0


def test_session_saturates_the_window_before_ctypes(monkeypatch):
    """DeviceSession passes the window through int32 arguments, which ctypes narrows silently: 2**31 as "to the end"
    would arrive as an empty window.  Both ends saturate at 2**31 - 1, a negative start is refused."""
    from waveformanalysis_amd import _lib, device

    lib = _WindowLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    sess = device.DeviceSession(0)
    i32max = 2**31 - 1
    table = {(0, 40): (0, 40), (5, 2**31): (5, i32max), (5, 2**40): (5, i32max), (2**31, 2**33): (i32max, i32max),
             (7, 7): (7, 7), (3, -2): (3, 0), (0, i32max): (0, i32max), (np.int64(2), np.int64(2**31)): (2, i32max)}
    for window, want in table.items():
        lib.calls.clear()
        sess.baseline_mean(*window)
        sess.fused_baseline_filter_hits(window, 2, 2)
        sess.hits_enqueue(_lib.SRC_SG_FUSED, window, 2, 2)
        assert lib.calls == [want] * 3, window
        assert all(type(x) is int and 0 <= x <= i32max for call in lib.calls for x in call)
    lib.calls.clear()
    for call in (lambda: sess.baseline_mean(-1, 5), lambda: sess.fused_baseline_filter_hits((-1, 5)),
                 lambda: sess.hits_enqueue(_lib.SRC_SG_FUSED, (-2**31, 5))):
        with pytest.raises(ValueError, match="baseline window start must be >= 0"):
            call()
    assert lib.calls == []
