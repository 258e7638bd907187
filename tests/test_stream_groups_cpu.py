"""HipThresholdHitStream under per-channel settings, without a GPU: option precedence, the once-per-run resolution,
the refusals, the rows of every driver against the run-wide oracle through a device double that computes
(tests/stream_groups_util.GroupOracleSession), and the device calls of the default path."""

from __future__ import annotations

import numpy as np
import pytest

from tests import fused_groups_util as F
from tests import golden_util as G
from tests import stream_groups_util as U
from tests import stream_hits_util as S
from waveformanalysis_amd import _lib, streaming
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.streaming import HipThresholdHitStream

FLOAT_RTOL = 1e-6
# rows per channel of the run-wide oracle under FILTER_CC / HIT_CC, and under the uniform SG(11, 2) with one threshold
ROWS = {"ragged": (100, 472, 198, 127), "mixed": (175, 407, 526, 156), "shuffled": (100, 472, 198, 127),
        "sparse": (150, 371, 300, 135)}
UNIFORM_ROWS = {"ragged": 596, "mixed": 822}


# ---- inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.RUN_NAMES)
def test_inputs_are_what_the_tests_rely_on(name):
    rows = U.want(name)
    assert tuple(np.bincount(rows["channel"], minlength=4)) == ROWS[name]
    run = U.run(name)
    if name in UNIFORM_ROWS:
        assert len(run.want(True)) == UNIFORM_ROWS[name]
    if name == "ragged":
        assert int(run.in_padding(rows).sum()) == 183
    if name != "sparse":  # padding every chunk to its own longest record changes the table
        c = run.chunk_sizes[0]
        filtered = U.oracle_filtered(run.records, run.pool, U.KEYS["full"])
        parts = [S.O.threshold_hits(ch.data, filtered, thresholds=U.THRESHOLDS[ch.data["channel"]], left_extension=U.LE,
                                    right_extension=U.RE) for ch in run.chunks(c)]
        assert np.concatenate(parts).tobytes() != rows.tobytes()
    else:  # the per-group counts jump between blocks: a bound sized by the previous chunk is exceeded
        per_chunk = np.array([[int(((rows["channel"] == g) & np.isin(rows["record_id"], ch.data["record_id"])).sum())
                               for g in range(4)] for ch in run.chunks(S.SPARSE_BLOCK)])
        assert np.any(per_chunk[1:] > per_chunk[:-1] + per_chunk[:-1] // 8 + 4096) or np.any(per_chunk == 0)


def test_missing_groups_run_and_the_sg_only_variant():
    assert len(U.want("missing")) > 300 and len(U.want("missing", "sg_only")) > 300
    assert U.want("ragged", "sg_only").tobytes() != U.want("ragged").tobytes()


# ---- options --------------------------------------------------------------------------------------------------------
def test_option_precedence_and_refusals():
    run = U.run("ragged")
    ctx = U.context(run.records, run.pool)
    p = HipThresholdHitStream()
    assert (p.channel_config, p.filter_source) == (None, "own")
    p._configure(ctx)
    assert p.channel_config == U.HIT_CC and p.filter_source == "wave_pool_filtered" and p.use_filtered
    p = HipThresholdHitStream(channel_config={"0:1": {"threshold": 5.0}}, filter_source="own")
    p._configure(ctx)
    assert p.channel_config == {"0:1": {"threshold": 5.0}} and p.filter_source == "own"
    with pytest.raises(ValueError, match="filter_source"):
        HipThresholdHitStream(filter_source="bogus")
    with pytest.raises(ValueError, match="contradict"):
        HipThresholdHitStream(sg_window_size=7, filter_source="wave_pool_filtered")
    with pytest.raises(ValueError, match="contradict"):       # the Context says wave_pool_filtered, the constructor an SG pair
        HipThresholdHitStream(sg_poly_order=3)._configure(ctx)
    # filter_source applies only with use_filtered: the raw samples, per-channel thresholds
    p = HipThresholdHitStream(use_filtered=False)
    p._configure(ctx)
    plan = p._run_plan(ctx, "run")
    assert plan.keys == [] and sorted(set(plan.threshold_of_key.tolist())) == [2.0, 3.0, 10.0]


def test_resolution_happens_once_per_run(monkeypatch):
    run = U.run("ragged")
    ctx = U.context(run.records, run.pool)
    calls = []
    resolve = streaming._RunPlan.resolve.__func__
    monkeypatch.setattr(streaming._RunPlan, "resolve", classmethod(lambda cls, *a: (calls.append(1), resolve(cls, *a))[1]))
    pool = U.oracle_pool()
    p = HipThresholdHitStream(device_pool=pool)
    outs = list(p.compute(ctx, "run", streaming_config={"chunk_size": 100, "max_workers": 2}))
    assert len(outs) == 6 and len(calls) == 1
    p.run_chunks(run.chunks(150), ctx, "run", max_workers=1)
    for ch in run.chunks(150)[:2]:
        p.compute_chunk(ch, ctx, "run")
    assert len(calls) == 1
    plan = p._run_plan(ctx, "run")
    assert plan.keys == U.KEYS["full"] or sorted(plan.keys, key=repr) == sorted(U.KEYS["full"], key=repr)
    gor, thr = plan.lookup(run.records[:8])
    assert [plan.keys[g] for g in gor[:4]] == F.KEYS and thr[:4].tolist() == F.THRESHOLDS
    # another configuration, or another records array, resolves again
    other = U.context(run.records, run.pool, "sg_only")
    p.run_chunks(run.chunks(150), other, "run", max_workers=2)
    assert len(calls) == 2
    p.run_chunks(run.chunks(150), U.context(run.records.copy(), run.pool, "sg_only"), "run", max_workers=2)
    assert len(calls) == 3
    pool.close()


def test_too_many_filter_settings_are_refused_before_any_upload():
    run = U.run("ragged")
    rec = run.records.copy()
    rec["channel"] = np.arange(len(rec)) % 9
    cc = {f"0:{c}": {"sg_window_size": 5 + 2 * c, "sg_poly_order": 2} for c in range(9)}
    ctx = U.context(rec, run.pool, extra={"wave_pool_filtered": {"channel_config": cc}})
    pool = U.oracle_pool()
    with pytest.raises(ValueError, match="distinct filter settings"):
        HipThresholdHitStream(device_pool=pool).run_chunks(S.records_to_chunks(rec, 100, "run"), ctx, "run", max_workers=2)
    assert pool.calls == [] and pool.uploads == []
    # a chunk with a channel the run's records do not hold
    ctx = U.context(run.records, run.pool)
    with pytest.raises(ValueError, match="the run's records do not"):
        HipThresholdHitStream(device_pool=pool).run_chunks(S.records_to_chunks(rec, 100, "run"), ctx, "run", max_workers=2)
    pool.close()


# ---- rows -----------------------------------------------------------------------------------------------------------
def _drivers(plugin, run, ctx, c):
    chunks = run.chunks(c)
    yield "compute serial", chunks, list(plugin.compute(ctx, "run", streaming_config={"chunk_size": c, "parallel": False}))
    yield "compute parallel", chunks, list(plugin.compute(ctx, "run", streaming_config={"chunk_size": c, "max_workers": 3}))
    for w in (1, 2, 8):
        yield f"run_chunks workers={w}", chunks, plugin.run_chunks(chunks, ctx, "run", max_workers=w)


@pytest.mark.parametrize("config", ["full", "sg_only"])
@pytest.mark.parametrize("name", U.RUN_NAMES)
def test_rows_equal_the_run_wide_oracle(name, config):
    run = U.run(name)
    want = U.want(name, config)
    ctx = U.context(run.records, run.pool, config)
    pool = U.oracle_pool()
    plugin = HipThresholdHitStream(device_pool=pool)
    for c in run.chunk_sizes:
        for what, chunks, outs in _drivers(plugin, run, ctx, c):
            got = S.check_bookkeeping(run, chunks, outs, want, f"{name} {config} c={c} {what}")
            G.assert_struct_equal(got, want, float_rtol=FLOAT_RTOL, what=f"{name} {config} c={c} {what}")
            for k, (ch, o) in enumerate(zip(chunks, outs)):
                assert len(o.data) == int(np.isin(want["record_id"], ch.data["record_id"]).sum()), (what, k)
    grouped = [e for e in pool.log if "groups" in e]
    assert grouped and all(e["max_len"] == run.width for e in pool.log)
    assert all(len(e["groups"]) == 4 for e in grouped)        # groups are numbered over the run, not over the chunk
    assert all([s for s, _slot in e["groups"]] == [_lib.SRC_F32 if k[0] == "BW" else _lib.SRC_SG_FUSED
                                                   for k in plugin._run_plan(ctx, "run").keys] for e in grouped)
    assert ("sosfiltfilt_group" in pool.calls) == (config == "full")
    if name == "missing":
        present = {len(np.unique(e["group_of_record"])) for e in grouped}
        assert {1, 2, 4} <= present
    pool.close()


def test_one_sg_group_with_thresholds_takes_the_single_pass():
    run = U.run("ragged")
    ctx = SimpleContext({"wave_source": "records", "hit_threshold_stream": {"use_filtered": True, "channel_config": U.HIT_CC}},
                        {"records": run.records, "wave_pool": run.pool})
    pool = U.oracle_pool()
    outs = HipThresholdHitStream(device_pool=pool).run_chunks(run.chunks(150), ctx, "run", max_workers=2)
    want = S.O.threshold_hits(run.records, run.filtered, thresholds=U.THRESHOLDS[run.records["channel"]],
                              left_extension=U.LE, right_extension=U.RE)
    G.assert_struct_equal(np.concatenate([o.data for o in outs]), want, float_rtol=FLOAT_RTOL, what="own filter")
    assert pool.calls == ["upload_pool", "upload_records[]", "set_sg_plan", "hits_enqueue"] * 4
    pool.close()


# ---- the default path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_filtered", [False, True])
def test_default_path_makes_the_parent_commits_device_calls(use_filtered, monkeypatch):
    run = U.run("ragged")
    ctx = SimpleContext({"wave_source": "records"}, {"records": run.records, "wave_pool": run.pool})
    monkeypatch.setattr(streaming._RunPlan, "resolve", classmethod(lambda cls, *a: pytest.fail("resolved on the default path")))
    monkeypatch.setattr(streaming, "_channel_keys", lambda data: pytest.fail("per-record host work on the default path"))
    per_chunk = ["upload_pool", "upload_records"] + (["set_sg_plan"] if use_filtered else []) + ["hits_enqueue"]
    for driver in ("compute serial", "compute parallel", "run_chunks", "compute_chunk"):
        pool = U.oracle_pool()
        plugin = HipThresholdHitStream(use_filtered=use_filtered, device_pool=pool)
        if driver.startswith("compute "):
            cfg = {"chunk_size": 100, "parallel": driver.endswith("parallel"), "max_workers": 2}
            outs = list(plugin.compute(ctx, "run", streaming_config=cfg))
        elif driver == "run_chunks":
            outs = plugin.run_chunks(run.chunks(100), ctx, "run", max_workers=2)
        else:
            outs = [plugin.compute_chunk(ch, ctx, "run") for ch in run.chunks(100)]
        assert pool.calls == per_chunk * 6, (driver, pool.calls[:8])
        assert all(e["max_len"] == run.width and "groups" not in e for e in pool.log)
        assert all(e["source"] == (_lib.SRC_SG_FUSED if use_filtered else _lib.SRC_RAW) for e in pool.log)
        G.assert_struct_equal(np.concatenate([o.data for o in outs]), run.want(use_filtered), float_rtol=FLOAT_RTOL, what=driver)
        pool.close()
