"""HipS1S2Stream without a GPU: chunk boundaries, what a chunk hands to its session (through a recording double),
the host-side refusals, option precedence, the hip_streaming() profile and the declared entry points."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest

from tests import s1s2_chain_util as U
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DevicePool
from waveformanalysis_amd.dtypes import S1_S2_CLASSIFIER_DTYPE
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import hip_default, hip_streaming
from waveformanalysis_amd.plugins import s1_s2
from waveformanalysis_amd.s1s2_stream import HipS1S2Stream
from waveformanalysis_amd.streaming import HipThresholdHitStream

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RecordingSession:
    """Stands where a DeviceSession would: keeps every call with its arguments, computes nothing.  peak_chain answers
    one row per uploaded record so that the driver's bookkeeping can be followed."""

    def __init__(self, device_id, calls):
        self.device_id, self.calls = device_id, calls
        self.n = 0

    def upload_pool(self, pool):
        self.calls.append(("upload_pool", pool.copy()))

    def upload_records(self, records, thresholds=10.0, polarity=None):
        self.n = len(records)
        self.calls.append(("upload_records", records.copy()))

    def set_sg_plan(self, window, order):
        self.calls.append(("set_sg_plan", (window, order)))

    def savgol(self, download=True):
        self.calls.append(("savgol", download))

    def sosfiltfilt(self, sos, zi, padlen, download=True):
        self.calls.append(("sosfiltfilt", (np.asarray(sos).shape, int(padlen), download)))

    def find_peaks(self, source, download=True, **kw):
        self.calls.append(("find_peaks", dict(source=source, download=download, **kw)))
        return self.n

    def peak_chain(self, width_source, feature_source, **kw):
        self.calls.append(("peak_chain", dict(width_source=width_source, feature_source=feature_source, **kw)))
        out = np.zeros(self.n, dtype=S1_S2_CLASSIFIER_DTYPE)
        out["record_id"] = kw["record_id_base"] + np.arange(self.n)
        out["timestamp"] = self.calls_timestamp()
        return out

    def calls_timestamp(self):
        return [c for c in self.calls if c[0] == "upload_records"][-1][1]["timestamp"]

    def close(self):
        pass


def recording_pool():
    calls = []
    pool = DevicePool(device_ids=[0], session_factory=lambda dev: RecordingSession(dev, calls))
    pool.calls = calls
    return pool


def _context(name="ragged", **config):
    rec, pool, hit_kw = U.run(name)
    return rec, pool, SimpleContext({"wave_source": "records", **hit_kw, **U.C5_RANGES, **config},
                                    {"records": rec, "wave_pool": pool})


def _per_chunk(calls):
    """The call list cut at every upload_pool."""
    out = []
    for c in calls:
        if c[0] == "upload_pool":
            out.append([])
        out[-1].append(c)
    return out


@pytest.mark.parametrize("chunk_size", [1, 3, 7, 16, 40, 1000])
def test_chunks_rebased_inputs_and_call_sequence(chunk_size):
    rec, pool, ctx = _context()
    dp = recording_pool()
    outs = list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config={"chunk_size": chunk_size, "parallel": False}))
    bounds = list(range(0, len(rec), chunk_size))
    assert len(outs) == len(bounds) and all(o.data.dtype == S1_S2_CLASSIFIER_DTYPE for o in outs)
    with_samples = [lo for lo in bounds if rec["event_length"][lo : lo + chunk_size].sum() > 0]
    chunks = _per_chunk(dp.calls)
    assert len(chunks) == len(with_samples)
    for lo, calls in zip(with_samples, chunks):
        part = rec[lo : lo + chunk_size]
        assert [c[0] for c in calls] == ["upload_pool", "upload_records", "set_sg_plan", "savgol", "find_peaks", "peak_chain"]
        first = int(part["wave_offset"].min())
        last = int((part["wave_offset"] + part["event_length"]).max())
        assert np.array_equal(calls[0][1], pool[first:last])
        up = calls[1][1]
        assert np.array_equal(up["wave_offset"], part["wave_offset"] - first)
        assert np.array_equal(up["record_id"], np.arange(len(part)))
        for name in ("timestamp", "baseline", "event_length", "dt", "board", "channel", "polarity"):
            assert up[name].tobytes() == part[name].tobytes(), name  # (an empty record's baseline is NaN)
        assert calls[2][1] == (11, 2) and calls[3][1] is False
        peaks = calls[4][1]
        assert peaks["source"] == _lib.SRC_F32 and peaks["download"] is False
        assert {k: peaks[k] for k in U.RAGGED_HIT} == U.RAGGED_HIT and peaks["height_method"] == "minmax"
        chain = calls[5][1]
        assert chain["record_id_base"] == int(part["record_id"][0]) == lo
        assert (chain["width_source"], chain["feature_source"]) == (_lib.SRC_RAW, _lib.SRC_RAW)
        assert chain["sampling_rate"] == 0.5 and chain["height_range"] == (40, 90) and chain["area_range"] == (0, None)
        assert {k: chain[k] for k in U.C5_RANGES} == U.C5_RANGES and chain["conflict_policy"] == "unknown"
    # the rows carry the run's ids, every result spans the records it came from
    got = np.concatenate([o.data for o in outs])
    sampled = np.concatenate([np.arange(lo, min(lo + chunk_size, len(rec))) for lo in with_samples])
    assert np.array_equal(got["record_id"], sampled)
    for lo, o in zip(bounds, outs):
        part = rec[lo : lo + chunk_size]
        assert o.start == int(part["timestamp"][0])
        assert o.end > int((part["timestamp"] + part["dt"].astype(np.int64) * 1000 * part["event_length"]).max())
    dp.close()


def test_chunking_is_the_hit_streams():
    rec, _pool, _ctx = _context()
    a, b = HipS1S2Stream(), HipThresholdHitStream()
    for p in (a, b):
        p.chunk_size = 7
    mine, theirs = list(a._data_to_chunks(rec, "run")), list(b._data_to_chunks(rec, "run"))
    assert len(mine) == len(theirs) == 6
    for x, y in zip(mine, theirs):
        assert (x.start, x.end, x.metadata) == (y.start, y.end, y.metadata) and x.data.tobytes() == y.data.tobytes()
    assert HipS1S2Stream._data_to_chunks is HipThresholdHitStream._data_to_chunks


def test_raw_detection_skips_the_filter_and_butterworth_filters_on_the_device():
    _rec, _pool, ctx = _context(use_filtered=False)
    dp = recording_pool()
    list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config={"chunk_size": 40, "parallel": False}))
    assert [c[0] for c in dp.calls] == ["upload_pool", "upload_records", "find_peaks", "peak_chain"]
    assert dp.calls[2][1]["source"] == _lib.SRC_RAW
    dp.close()
    _rec, _pool, ctx = _context(filter_type="BW", lowcut=0.1, highcut=0.2, fs=0.5, filter_order=4, width_use_filtered=True)
    dp = recording_pool()
    list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config={"chunk_size": 40, "parallel": False}))
    assert [c[0] for c in dp.calls] == ["upload_pool", "upload_records", "sosfiltfilt", "find_peaks", "peak_chain"]
    assert dp.calls[2][1][0] == (4, 6) and dp.calls[2][1][2] is False
    assert dp.calls[4][1]["width_source"] == _lib.SRC_F32 and dp.calls[4][1]["feature_source"] == _lib.SRC_RAW
    dp.close()


def test_refusals_happen_before_any_session_call():
    rec, pool, _ctx = _context()
    dp = recording_pool()
    cfg = {"chunk_size": 16, "parallel": False}

    shuffled = rec.copy()
    shuffled["record_id"] = shuffled["record_id"][::-1]
    ctx = SimpleContext({**U.RAGGED_HIT}, {"records": shuffled, "wave_pool": pool})
    with pytest.raises(ValueError, match=r"arange\(len\(records\)\)"):
        list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config=cfg))
    shifted = rec.copy()
    shifted["record_id"] += 5
    ctx = SimpleContext({}, {"records": shifted, "wave_pool": pool})
    with pytest.raises(ValueError, match=r"arange\(len\(records\)\)"):
        list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config=cfg))

    no_dt = np.zeros(len(rec), dtype=[d for d in rec.dtype.descr if d[0] != "dt"])
    for name in no_dt.dtype.names:
        no_dt[name] = rec[name]
    ctx = SimpleContext({}, {"records": no_dt, "wave_pool": pool})
    plugin = HipS1S2Stream(device_pool=dp)
    chunk = HipThresholdHitStream()._data_to_chunks(rec, "run").__next__()
    chunk.data = no_dt[: len(chunk.data)]
    with pytest.raises(ValueError, match=r"\[hit\] records is missing required field 'dt'; provide explicit config 'dt'\."):
        plugin.compute_chunk(chunk, ctx, "run")
    assert dp.calls == []
    HipS1S2Stream(device_pool=dp, dt=4).compute_chunk(chunk, ctx, "run")  # the option stands in
    assert [c[0] for c in dp.calls][:2] == ["upload_pool", "upload_records"]
    assert np.all(dp.calls[1][1]["dt"] == 4)
    del dp.calls[:]
    # the same through compute(): the chunk rule needs dt, so it is resolved before the records are cut
    with pytest.raises(ValueError, match=r"\[hit\] records is missing required field 'dt'; provide explicit config 'dt'\."):
        list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config=cfg))
    assert dp.calls == []
    for plugin, context in ((HipS1S2Stream(device_pool=dp, dt=4), ctx),
                            (HipS1S2Stream(device_pool=dp), SimpleContext({"dt": 4}, {"records": no_dt, "wave_pool": pool})),
                            (HipS1S2Stream(device_pool=dp),
                             SimpleContext({"s1_s2_stream": {"dt": 4}}, {"records": no_dt, "wave_pool": pool}))):
        outs = list(plugin.compute(context, "run", streaming_config=cfg))
        assert len(outs) == 3 and [c[0] for c in dp.calls].count("peak_chain") == 3
        uploads = [c[1] for c in dp.calls if c[0] == "upload_records"]
        assert all(np.all(u["dt"] == 4) for u in uploads) and sum(len(u) for u in uploads) == len(rec)
        # the chunks are those of the records that carry the column
        with_dt = list(HipS1S2Stream(device_pool=dp).compute(SimpleContext({}, {"records": rec, "wave_pool": pool}), "run",
                                                              streaming_config=cfg))
        assert [(o.start, o.end) for o in outs] == [(o.start, o.end) for o in with_dt]
        del dp.calls[:]
    with pytest.raises(ValueError, match=r"\[hit\] dt must be > 0"):
        list(HipS1S2Stream(device_pool=dp, dt=0).compute(ctx, "run", streaming_config=cfg))
    assert dp.calls == []

    # records without a record_id column; settings of the static chain the stream does not implement
    no_id = np.zeros(len(rec), dtype=[d for d in rec.dtype.descr if d[0] != "record_id"])
    for name in no_id.dtype.names:
        no_id[name] = rec[name]
    with pytest.raises(ValueError, match="need a 'record_id' column"):
        list(HipS1S2Stream(device_pool=dp).compute(SimpleContext({}, {"records": no_id, "wave_pool": pool}), "run",
                                                   streaming_config=cfg))
    for config in ({"channel_config": {"0:1": {"sg_window_size": 7}}},
                   {"wave_pool_filtered": {"channel_config": {"0:1": {"filter_type": "BW"}}}},
                   {"basic_features": {"channel_config": {"0:1": {"fixed_baseline": 8000.0}}}},
                   {"basic_features.fixed_baseline": {"0:1": 8000.0}}):
        with pytest.raises(ValueError, match="outside the stream"):
            list(HipS1S2Stream(device_pool=dp).compute(SimpleContext(config, {"records": rec, "wave_pool": pool}), "run",
                                                       streaming_config=cfg))
    assert dp.calls == []

    ctx = SimpleContext({"height_method": "bogus"}, {"records": rec, "wave_pool": pool})
    with pytest.raises(ValueError, match="不支持的峰高计算方法: bogus"):
        list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config=cfg))
    ctx = SimpleContext({"strict": True}, {"records": rec, "wave_pool": pool})
    with pytest.raises(ValueError, match="No S1/S2 criteria configured"):
        list(HipS1S2Stream(device_pool=dp).compute(ctx, "run", streaming_config=cfg))
    assert dp.calls == []
    dp.close()


def test_empty_inputs_give_empty_chunks_of_the_output_dtype():
    rec, pool, ctx = _context()
    dp = recording_pool()
    plugin = HipS1S2Stream(device_pool=dp)
    assert list(plugin.compute(SimpleContext({}, {"records": rec[:0], "wave_pool": pool}), "run")) == []
    chunk = next(HipThresholdHitStream()._data_to_chunks(rec, "run"))
    chunk.data = rec[:0]
    out = plugin.compute_chunk(chunk, ctx, "run")
    assert out.data.dtype == S1_S2_CLASSIFIER_DTYPE and len(out.data) == 0
    plugin.chunk_size = 1
    one = list(plugin._data_to_chunks(rec, "run"))[1]  # record 1 holds no sample
    assert int(one.data["event_length"][0]) == 0
    out = plugin.compute_chunk(one, ctx, "run")
    assert out.data.dtype == S1_S2_CLASSIFIER_DTYPE and len(out.data) == 0 and dp.calls == []
    dp.close()


def test_option_precedence():
    _rec, _pool, ctx = _context(s1_s2_stream={"height": 12.0, "sampling_rate": 0.25}, prominence=0.9)
    p = HipS1S2Stream()
    assert p.cfg["peaks"]["height"] == 30.0 and p.cfg["use_filtered"] and p.cfg["chain"]["sampling_rate"] == 0.5
    cfg = p._configure(ctx)
    assert cfg["peaks"]["height"] == 12.0 and cfg["peaks"]["prominence"] == 0.9 and cfg["peaks"]["width"] == 2
    assert cfg["chain"]["sampling_rate"] == 0.25 and cfg["chain"]["s2_area_range"] == (500.0, 1e12)
    cfg = HipS1S2Stream(height=5.0, conflict_policy="prefer_s2", width_use_filtered=True)._configure(ctx)
    assert cfg["peaks"]["height"] == 5.0 and cfg["chain"]["conflict_policy"] == "prefer_s2"
    assert cfg["width_source"] == _lib.SRC_F32 and cfg["feature_source"] == _lib.SRC_RAW
    with pytest.raises(TypeError, match="unknown options"):
        HipS1S2Stream(bogus=1)
    # names and defaults are the static plugins'
    static = {p.provides: p for p in hip_default()}
    for provides, skip in (("hit", ("wave_source", "parallel", "n_workers", "chunk_size", "parallel_min_events", "devices")),
                           ("s1_s2", ()), ("waveform_width", ("use_filtered", "wave_source", "devices"))):
        for name, opt in static[provides].options.items():
            if name not in skip:
                assert HipS1S2Stream.options[name].default == opt.default, (provides, name)
    for name in ("filter_type", "lowcut", "highcut", "fs", "filter_order", "sg_window_size", "sg_poly_order"):
        assert HipS1S2Stream.options[name].default == static["wave_pool_filtered"].options[name].default
    for name in ("height_range", "area_range"):
        assert HipS1S2Stream.options[name].default == static["basic_features"].options[name].default


def test_profile_and_contract():
    streams = hip_streaming()
    assert sorted(p.provides for p in streams) == ["hit_threshold_stream", "s1_s2_stream", "signal_peaks_stream"]
    p = [q for q in streams if q.provides == "s1_s2_stream"][0]
    assert isinstance(p, HipS1S2Stream) and p.depends_on == ["records", "wave_pool"] and p.save_when == "never"
    assert p.output_dtype == S1_S2_CLASSIFIER_DTYPE and p.output_data_kind == "peaks"
    assert "s1_s2_stream" not in [q.provides for q in hip_default()]


def test_ranges_and_strict_are_the_static_plugins():
    ranges = s1_s2.class_ranges(s1_width_range=(0, 80), s2_area_range=(None, None), s2_height_range=(5, None))
    assert ranges == ((0.0, 80.0), None, None, None, None, (5.0, None))
    with pytest.raises(ValueError, match="range must be a tuple"):
        s1_s2.class_ranges(s1_width_range=[0, 1])
    with pytest.raises(ValueError, match="No S1/S2 criteria configured"):
        s1_s2.class_ranges(strict=True, s1_area_range=(None, None))


def test_header_declares_the_entry_points():
    header = open(os.path.join(REPO, "include", "wfa_hip.h")).read()
    for name in ("wfa_peak_chain_count", "wfa_peak_chain_fill"):
        assert re.search(rf"^int {name}\(wfa_ctx\* ctx", header, flags=re.M), name
        assert name in _lib.SIGNATURES
    assert int(re.search(r"#define WFA_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 6
    assert len(_lib.SIGNATURES["wfa_peak_chain_count"][1]) == 21
